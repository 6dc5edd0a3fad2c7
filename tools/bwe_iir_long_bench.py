#!/usr/bin/env python
"""Denoiser evaluations/s of bandwidth extension of whole recordings through an IIR filter (Sampler.predict_bwe_iir_long) at the BASELINE.json
configs[1] shape (L = 184184, T = 36, xi = 0.25), next to predict_bwe "cheby1" at batch 8 on segments of the same recordings measured IN THE
SAME RUN: --recordings recordings of --windows windows each (2 x 8: 1151150 samples), low-passed as a whole (scipy.signal.lfilter, float64,
rounded to float32) with a Chebyshev type I filter of --order (8) and 0.05 dB ripple at --cutoff Hz (4000).  Every window is a job, so pass A and pass B are one batch of
recordings * windows / 2 windows each (8 by default: the same batch as the predict_bwe runs).  One warm-up of each and one complete
predict_bwe run, reported apart as ``bwe_first_complete_run`` (the first complete run after the two-step ones is slower than every later
one), then --rounds alternating pairs (predict_bwe, whole recordings) of COMPLETE runs; last, the same recordings one window at a time
(max_batch = 1).  The yardstick is predict_bwe in the same run: a pass is "at rate" when it is no slower than predict_bwe by more than
the spread of the identical predict_bwe runs plus 0.5 %.  Per-pass times come from events recorded on the stream around every Sampler.predict call -- no host synchronisation
inside a run; what a run spends outside the sampler calls (the plan, one gather and one scatter launch per pass) is its wall time minus
the spans.  (The segments of the predict_bwe runs are cut out of the filtered recording: predict_bwe takes them as if filtered from a zero
state, which changes what it restores but not what an evaluation costs.)  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--recordings", type=int, default=2)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--T", type=int, default=36)
    ap.add_argument("--order", type=int, default=8)
    ap.add_argument("--cutoff", type=float, default=4000.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_bwe_iir_long_bench.json"))
    a = ap.parse_args()
    import scipy.signal
    import torch
    from audio_inpainting_diffusion_amd import bwe_iir_long
    from audio_inpainting_diffusion_amd.config import make_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.init import seeded_init_, seeded_normal
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    from audio_inpainting_diffusion_amd.sampler import Sampler, autoregressive_length, autoregressive_overlap
    dev = torch.device("cuda", 0)
    B, L, R, W, T = a.batch, 184184, a.recordings, a.windows, a.T
    args = make_args("maestro22k", audio_len=L, T=T, xi=0.25)
    args.tester.data_consistency.use = False                    # guidance only
    net = seeded_init_(Unet_CQT_oct_with_attention(args, dev), 0)
    net.prepare()
    smp = Sampler(model=net, diff_params=EDM(args), args=args)
    end = int(autoregressive_overlap(args) * L)
    N = autoregressive_length(L, end, W)
    filt = scipy.signal.cheby1(a.order, 0.05, a.cutoff, fs=args.exp.sample_rate)
    table = bwe_iir_long.IIRTable(filt, "cheby1")
    clean = torch.stack([torch.from_numpy(seeded_normal(7, g, N)) for g in range(R)]).float().mul_(0.063)
    rec = torch.from_numpy(scipy.signal.lfilter(table.b, table.a, clean.double().numpy(), axis=-1)).float().to(dev)     # the whole recording through the filter
    jobs_A, jobs_B = bwe_iir_long.iir_plan(R, N, L, end, table.order)
    assert len(jobs_A) + len(jobs_B) == R * W
    starts = [(r, s) for r, s, *_ in (jobs_A + jobs_B) if s + L <= N][:B]
    y_seg = torch.stack([rec[r, s:s + L] for r, s in starts]).contiguous()
    assert y_seg.shape[0] == B
    per_item = 2 * T - 1                                         # T first evaluations + T - 1 Heun corrections (the last step is Euler)

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

    def run(mode, max_batch=B):
        spans.clear()
        torch.cuda.synchronize()
        n0, t0 = smp.n_evals, time.perf_counter()
        if mode == "bwe":
            smp.seeds = list(range(B))
            out = smp.predict_bwe(y_seg, filt, "cheby1")
        else:
            out = smp.predict_bwe_iir_long(rec, filt, "cheby1", max_batch=max_batch, seeds=list(range(R)))
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        assert torch.isfinite(out).all()
        return {"evals": smp.n_evals - n0, "wall_s": wall, "call_s": [s.elapsed_time(e) / 1e3 for s, e, _ in spans], "call_batch": [b for _, _, b in spans]}

    modes = ("bwe", "long")
    smp.nb_steps = 2                                             # warm-up: plans and pinned buffers of every batch size the timed runs use
    for mode in modes:
        run(mode)
    run("long", 1)
    smp.nb_steps = T
    first = run("bwe")                                           # one complete run, reported apart: the first complete run after the short ones is slow
    res = {mode: [] for mode in modes}
    for _ in range(a.rounds):
        for mode in modes:
            res[mode].append(run(mode))
    seq = run("long", 1)
    nA, nB = -(-len(jobs_A) // B), -(-len(jobs_B) // B)
    ref = [r["evals"] / r["call_s"][0] for r in res["bwe"]]      # the same stream-event span as the passes below
    spread = (max(ref) - min(ref)) / max(ref)
    r2 = lambda v: [round(x, 2) for x in v]                      # noqa: E731
    runs = res["long"]
    pa = [len(jobs_A) * per_item / sum(r["call_s"][:nA]) for r in runs]
    pb = [len(jobs_B) * per_item / sum(r["call_s"][nA:nA + nB]) for r in runs]
    whole = [r["evals"] / r["wall_s"] for r in runs]
    outside = [r["wall_s"] - sum(r["call_s"]) for r in runs]
    rel_a, rel_b = max(pa) / max(ref), max(pb) / max(ref)
    line = json.dumps({"metric": "denoiser evaluations/s", "segment": L, "T": T, "xi": 0.25, "filter": "cheby1, 0.05 dB", "order": table.order, "cutoff_hz": a.cutoff,
                       "amplification": round(table.amplification, 2), "seed_error_bound": table.seed_error_bound,
                       "recordings": R, "windows_per_recording": W, "samples_per_recording": N, "overlap_samples": end,
                       "jobs_pass_A": len(jobs_A), "jobs_pass_B": len(jobs_B), "max_batch": B, "rounds": a.rounds, "evals_per_window": per_item,
                       "pass_batches": runs[0]["call_batch"],
                       "bwe_batch": B, "bwe_first_complete_run": round(first["evals"] / first["call_s"][0], 2),
                       "bwe_complete_run": r2(ref), "bwe_spread": round(spread, 4),
                       "pass_A": r2(pa), "pass_B": r2(pb), "long_whole_call": r2(whole), "outside_sampler_calls_ms": [round(c * 1e3, 2) for c in outside],
                       "pass_A_vs_bwe": round(rel_a, 4), "pass_B_vs_bwe": round(rel_b, 4),
                       "margin": round(spread + 0.005, 4), "pass_A_at_rate": bool(rel_a >= 1 - spread - 0.005), "pass_B_at_rate": bool(rel_b >= 1 - spread - 0.005),
                       "long_spread": round((max(whole) - min(whole)) / max(whole), 4),
                       "one_window_at_a_time": round(seq["evals"] / seq["wall_s"], 2), "one_window_at_a_time_wall_s": round(seq["wall_s"], 2),
                       "batched_wall_s": [round(r["wall_s"], 2) for r in runs],
                       "batching_gain": round(seq["wall_s"] / min(r["wall_s"] for r in runs), 3)})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
