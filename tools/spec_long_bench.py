#!/usr/bin/env python
"""Denoiser evaluations/s of spectrogram inpainting of whole recordings (Sampler.predict_spectrogram_inpainting_long) at the BASELINE.json
configs[1] shape (L = 184184, T = 36, xi = 0.25; n_fft 1024, hop_length 256, data consistency as make_args sets it), next to
predict_spectrogram_inpainting at batch 8 on segments of the same recordings measured IN THE SAME PROCESS: --recordings recordings of
--samples samples each (2 x 1151150).  The overlap 46046 is widened to end' = 46200, so the step is 137984 and a recording of 1151150 samples
has NINE windows; the ninth holds the last 47278 samples and owns the last 45232.  The mask puts a rectangle of masked bins (bins 14-92, 40
frames) into the owned range of each of the first eight windows and none into the ninth's, so both passes are full chunks of 8 (8 + 8 jobs)
and the ninth window costs nothing.  One warm-up of each mode and one complete predict_spectrogram_inpainting run, reported apart as
``seg_first_complete_run``, then --rounds alternating pairs (segments, whole recordings) of COMPLETE runs; then the same recordings one
window at a time (max_batch = 1); last a mask that touches windows 2 and 5 only, which must cost two windows' worth of evaluations per
recording.  The yardstick is predict_spectrogram_inpainting in the same process: a pass is "at rate" when it lies no further below than the
spread of the identical segment runs plus 0.5 %.  Per-pass times come from events recorded on the stream around every Sampler.predict call --
no host synchronisation inside a run; what a run spends outside the sampler calls (the mask reduction and its read-back, the plan, the
envelope table, one gather and one scatter launch per pass) is its wall time minus the spans.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MARGIN = 0.005


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--recordings", type=int, default=2)
    ap.add_argument("--samples", type=int, default=1151150)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--T", type=int, default=36)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_spec_long_bench.json"))
    a = ap.parse_args()
    import torch
    from audio_inpainting_diffusion_amd import spec_long
    from audio_inpainting_diffusion_amd.config import make_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.init import seeded_init_, seeded_normal
    from audio_inpainting_diffusion_amd.restore import aligned_end
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    from audio_inpainting_diffusion_amd.sampler import Sampler, autoregressive_overlap
    from audio_inpainting_diffusion_amd.stft import SpectralMask
    dev = torch.device("cuda", 0)
    B, L, R, N, T = a.batch, 184184, a.recordings, a.samples, a.T
    args = make_args("maestro22k", audio_len=L, T=T, xi=0.25)
    net = seeded_init_(Unet_CQT_oct_with_attention(args, dev), 0)
    net.prepare()
    smp = Sampler(model=net, diff_params=EDM(args), args=args)
    st = args.tester.spectrogram_inpainting.stft
    n_fft, hop = st.n_fft, st.hop_length
    end = int(autoregressive_overlap(args) * L)
    end2 = aligned_end(L, end, hop)
    clean = torch.stack([torch.from_numpy(seeded_normal(7, g, N)) for g in range(R)]).float().mul_(0.063).to(dev)
    per_item = 2 * T - 1                                         # T first evaluations + T - 1 Heun corrections (the last step is Euler)
    F, T_rec = n_fft // 2 + 1, spec_long.rec_frames(N, n_fft, hop)
    wins = spec_long.spec_windows(N, L, end, n_fft, hop)
    f_lo, f_hi, half_t = 14, 93, 20                              # about 300 Hz ... 2 kHz at 22.05 kHz, 40 frames (0.46 s)

    def mask_over(windows):
        m = torch.ones(F, T_rec)
        for w in windows:
            c = (wins[w][0] + L // 2) // hop                     # the middle of a window lies in its owned range, even or odd
            m[f_lo:f_hi, c - half_t:c + half_t] = 0
        return m.to(dev)
    mask_all, mask_two = mask_over(range(8)), mask_over((2, 5))
    plans = {k: spec_long.spec_plan(spec_long.touched_frames(m), R, N, L, end, n_fft, hop) for k, m in (("all", mask_all), ("two", mask_two))}
    jobs_A, jobs_B = plans["all"]
    # the recordings masked as a whole: SpectralMask over all N samples
    whole = SpectralMask(mask_all, N, n_fft, hop, st.win_length, st.window, dev)
    rec = whole.apply(clean)
    rec_two = SpectralMask(mask_two, N, n_fft, hop, st.win_length, st.window, dev).apply(clean)
    del whole
    starts = [(r, s) for r, s, *_ in (jobs_A + jobs_B)][:B]
    T_seg = spec_long.rec_frames(L, n_fft, hop)
    seg_mask = torch.ones(F, T_seg)
    c = (L // 2) // hop
    seg_mask[f_lo:f_hi, c - half_t:c + half_t] = 0
    seg_mask = seg_mask.to(dev)
    y_seg = SpectralMask(seg_mask, L, n_fft, hop, st.win_length, st.window, dev).apply(torch.stack([clean[r, s:s + L] for r, s in starts]))
    assert tuple(y_seg.shape) == (B, L)

    spans = []
    inner = smp.predict

    def timed_predict(shape, device):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        x = inner(shape, device)
        e1.record()
        spans.append((e0, e1, int(shape[0])))
        return x
    smp.predict = timed_predict
    r2 = lambda v: [round(x, 2) for x in v]                      # noqa: E731

    def run(mode, max_batch=B):
        spans.clear()
        torch.cuda.synchronize()
        n0, t0 = smp.n_evals, time.perf_counter()
        if mode == "seg":
            smp.seeds = list(range(B))
            out = smp.predict_spectrogram_inpainting(y_seg, seg_mask)
        else:
            y, m = (rec_two, mask_two) if mode == "two" else (rec, mask_all)
            out = smp.predict_spectrogram_inpainting_long(y, m, max_batch=max_batch, seeds=list(range(R)))
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        assert torch.isfinite(out).all()
        print(f"{mode} max_batch {max_batch} steps {smp.nb_steps}: {wall:.2f} s", file=sys.stderr, flush=True)
        return {"evals": smp.n_evals - n0, "wall_s": wall, "call_s": [s.elapsed_time(e) / 1e3 for s, e, _ in spans], "call_batch": [b for _, _, b in spans]}

    modes = ("seg", "long")
    smp.nb_steps = 2                                             # warm-up: plans and pinned buffers of every batch size the timed runs use
    for mode in modes:
        run(mode)
    run("long", 1)
    run("two")
    smp.nb_steps = T
    first = run("seg")                                           # one complete run, reported apart: the first complete run after the short ones is slow
    res = {mode: [] for mode in modes}
    for _ in range(a.rounds):
        for mode in modes:
            res[mode].append(run(mode))
    seq = run("long", 1)
    two = run("two")
    nA, nB = -(-len(jobs_A) // B), -(-len(jobs_B) // B)
    ref = [r["evals"] / r["call_s"][0] for r in res["seg"]]      # the same stream-event span as the passes below
    spread = (max(ref) - min(ref)) / max(ref)
    runs = res["long"]
    pa = [len(jobs_A) * per_item / sum(r["call_s"][:nA]) for r in runs]
    pb = [len(jobs_B) * per_item / sum(r["call_s"][nA:nA + nB]) for r in runs]
    whole_call = [r["evals"] / r["wall_s"] for r in runs]
    outside = [r["wall_s"] - sum(r["call_s"]) for r in runs]
    rel_a, rel_b = max(pa) / max(ref), max(pb) / max(ref)
    two_jobs = sum(len(j) for j in plans["two"])
    dc = args.tester.data_consistency
    line = json.dumps({"metric": "denoiser evaluations/s", "segment": L, "T": T, "xi": 0.25, "degradation": "stft mask", "n_fft": n_fft, "hop_length": hop,
                       "data_consistency": dc.type if dc.use else "off", "norm": args.tester.posterior_sampling.norm, "recordings": R,
                       "samples_per_recording": N, "frames_per_recording": T_rec, "requested_overlap_samples": end, "overlap_samples": end2, "step": L - end2,
                       "windows_per_recording": len(wins), "masked_windows_per_recording": 8, "mask_bins": [f_lo, f_hi], "mask_frames_per_window": 2 * half_t,
                       "max_batch": B, "seg_batch": B, "rounds": a.rounds, "evals_per_window": per_item,
                       "jobs_pass_A": len(jobs_A), "jobs_pass_B": len(jobs_B), "pass_batches": runs[0]["call_batch"],
                       "chunk_evals_per_s": [r2([b * per_item / c for b, c in zip(r["call_batch"], r["call_s"])]) for r in runs],
                       "seg_first_complete_run": round(first["evals"] / first["call_s"][0], 2), "seg_complete_run": r2(ref), "seg_spread": round(spread, 4),
                       "pass_A": r2(pa), "pass_B": r2(pb), "long_whole_call": r2(whole_call), "outside_sampler_calls_ms": [round(c * 1e3, 2) for c in outside],
                       "pass_A_vs_seg": round(rel_a, 4), "pass_B_vs_seg": round(rel_b, 4), "margin": round(spread + MARGIN, 4),
                       "pass_A_at_rate": bool(rel_a >= 1 - spread - MARGIN), "pass_B_at_rate": bool(rel_b >= 1 - spread - MARGIN),
                       "long_spread": round((max(whole_call) - min(whole_call)) / max(whole_call), 4),
                       "one_window_at_a_time": round(seq["evals"] / seq["wall_s"], 2), "one_window_at_a_time_wall_s": round(seq["wall_s"], 2),
                       "batched_wall_s": [round(r["wall_s"], 2) for r in runs], "batching_gain": round(seq["wall_s"] / min(r["wall_s"] for r in runs), 3),
                       "two_windows_jobs": two_jobs, "two_windows_evals": two["evals"], "two_windows_evals_expected": two_jobs * per_item,
                       "two_windows_pass_batches": two["call_batch"], "two_windows_wall_s": round(two["wall_s"], 2),
                       "two_windows_outside_sampler_calls_ms": round((two["wall_s"] - sum(two["call_s"])) * 1e3, 2)})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
