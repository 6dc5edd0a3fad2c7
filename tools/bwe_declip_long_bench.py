#!/usr/bin/env python
"""Denoiser evaluations/s of bandwidth extension of whole recordings that are also clipped and have dropouts
(Sampler.predict_bwe_declip_long) at the BASELINE.json configs[1] shape (L = 184184, T = 36, xi = 0.25), next to predict_bwe_long on the
SAME filtered recordings measured IN THE SAME RUN: --recordings recordings of --windows windows each (2 x 8: 1151150 samples), low-passed as
a whole with a Hamming-windowed sinc of --taps taps at --cutoff Hz, then clipped at --clip (0.05) and with a dropout of --gap_ms (300 ms) in
every window.  Every window is a job in both modes, so pass A and pass B are one batch of recordings * windows / 2 windows each.  One
warm-up of each mode and one complete predict_bwe_long run, reported apart as ``bwe_long_first_complete_run`` (the first complete run after
the two-step ones is slower than every later one), then --rounds alternating pairs (predict_bwe_long, predict_bwe_declip_long) of COMPLETE
runs.  The yardstick is predict_bwe_long, existing code: the new mode is "at rate" when it lies within the spread of the identical
predict_bwe_long runs plus 0.5 %.  Per-pass times come from events recorded on the stream around every Sampler.predict call -- no host
synchronisation inside a run; what a run spends outside the sampler calls (the checks, the plan, two gather launches and one scatter launch
per pass) is its wall time minus the spans.  Prints one JSON line and writes it to --out."""
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
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--T", type=int, default=36)
    ap.add_argument("--taps", type=int, default=501)
    ap.add_argument("--cutoff", type=float, default=3000.0)
    ap.add_argument("--clip", type=float, default=0.05)
    ap.add_argument("--gap_ms", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_bwe_declip_long_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from audio_inpainting_diffusion_amd import bwe_long
    from audio_inpainting_diffusion_amd.config import make_args
    from audio_inpainting_diffusion_amd.degrade import FIRFilter
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.init import seeded_init_, seeded_normal
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    from audio_inpainting_diffusion_amd.sampler import Sampler, autoregressive_length, autoregressive_overlap
    dev = torch.device("cuda", 0)
    B, L, R, W, T, K = a.batch, 184184, a.recordings, a.windows, a.T, a.taps
    args = make_args("maestro22k", audio_len=L, T=T, xi=0.25)
    args.tester.data_consistency.use = False                    # guidance only
    net = seeded_init_(Unet_CQT_oct_with_attention(args, dev), 0)
    net.prepare()
    smp = Sampler(model=net, diff_params=EDM(args), args=args)
    end = int(autoregressive_overlap(args) * L)
    N = autoregressive_length(L, end, W)
    n = np.arange(K) - (K - 1) / 2
    h = np.sinc(2 * a.cutoff / args.exp.sample_rate * n) * np.hamming(K)
    taps = torch.from_numpy((h / h.sum()).astype(np.float32))
    clean = torch.stack([torch.from_numpy(seeded_normal(7, g, N)) for g in range(R)]).float().mul_(0.063).to(dev)
    filtered = FIRFilter(taps, N, device=dev).apply(clean)      # the whole recording through the filter, "same" padding
    jobs_A, jobs_B = bwe_long.bwe_plan(R, N, L, end, K)
    assert len(jobs_A) + len(jobs_B) == R * W
    # the dropouts: one of gap samples in the middle of every window's owned range
    gap = int(round(a.gap_ms * 1e-3 * args.exp.sample_rate))
    mask = torch.ones(1, N)
    for r, s, head, tail, lo, hi in jobs_A + jobs_B:
        if r == 0:
            mid = s + (lo + hi) // 2
            mask[0, mid - gap // 2:mid - gap // 2 + gap] = 0
    degraded = mask.to(dev) * filtered.clamp(-a.clip, a.clip)   # filter, then clip, then dropouts
    clipped = float((filtered.abs() >= a.clip).float().mean())
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

    def run(mode):
        spans.clear()
        torch.cuda.synchronize()
        n0, t0 = smp.n_evals, time.perf_counter()
        if mode == "bwe_long":
            out = smp.predict_bwe_long(filtered, taps, "firwin", max_batch=B, seeds=list(range(R)))
        else:
            out = smp.predict_bwe_declip_long(degraded, taps, "firwin", clip_value=a.clip, mask=mask, max_batch=B, seeds=list(range(R)))
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        assert torch.isfinite(out).all()
        return {"evals": smp.n_evals - n0, "wall_s": wall, "call_s": [s.elapsed_time(e) / 1e3 for s, e, _ in spans], "call_batch": [b for _, _, b in spans]}

    modes = ("bwe_long", "bwe_declip_long")
    smp.nb_steps = 2                                             # warm-up: plans and pinned buffers of every batch size the timed runs use
    for mode in modes:
        run(mode)
    smp.nb_steps = T
    first = run("bwe_long")                                      # one complete run, reported apart: the first complete run after the short ones is slow
    res = {mode: [] for mode in modes}
    for _ in range(a.rounds):
        for mode in modes:
            res[mode].append(run(mode))
    nA, nB = -(-len(jobs_A) // B), -(-len(jobs_B) // B)
    r2 = lambda v: [round(x, 2) for x in v]                      # noqa: E731

    def rates(runs):
        return ([len(jobs_A) * per_item / sum(r["call_s"][:nA]) for r in runs], [len(jobs_B) * per_item / sum(r["call_s"][nA:nA + nB]) for r in runs],
                [r["evals"] / r["wall_s"] for r in runs], [r["wall_s"] - sum(r["call_s"]) for r in runs])
    ref_a, ref_b, ref_whole, ref_out = rates(res["bwe_long"])
    new_a, new_b, new_whole, new_out = rates(res["bwe_declip_long"])
    spread = lambda v: (max(v) - min(v)) / max(v)                # noqa: E731
    rel = {"pass_A": max(new_a) / max(ref_a), "pass_B": max(new_b) / max(ref_b), "whole_call": max(new_whole) / max(ref_whole)}
    spreads = {"pass_A": spread(ref_a), "pass_B": spread(ref_b), "whole_call": spread(ref_whole)}
    line = json.dumps({"metric": "denoiser evaluations/s", "segment": L, "T": T, "xi": 0.25, "filter": "hamming-windowed sinc", "taps": K, "cutoff_hz": a.cutoff,
                       "clip_level": a.clip, "clipped_fraction_of_filtered_samples": round(clipped, 4), "dropout_ms": a.gap_ms, "dropout_samples": gap,
                       "dropouts_per_recording": W, "recordings": R, "windows_per_recording": W, "samples_per_recording": N, "overlap_samples": end,
                       "jobs_pass_A": len(jobs_A), "jobs_pass_B": len(jobs_B), "max_batch": B, "rounds": a.rounds, "evals_per_window": per_item,
                       "pass_batches": res["bwe_declip_long"][0]["call_batch"], "margin": f"spread of the identical predict_bwe_long runs + {MARGIN:.1%}",
                       "bwe_long_first_complete_run": round(first["evals"] / first["wall_s"], 2),
                       "bwe_long_pass_A": r2(ref_a), "bwe_long_pass_B": r2(ref_b), "bwe_long_whole_call": r2(ref_whole),
                       "bwe_long_outside_sampler_calls_ms": [round(c * 1e3, 2) for c in ref_out],
                       "bwe_long_spread": {k: round(v, 4) for k, v in spreads.items()},
                       "bwe_declip_long_pass_A": r2(new_a), "bwe_declip_long_pass_B": r2(new_b), "bwe_declip_long_whole_call": r2(new_whole),
                       "bwe_declip_long_outside_sampler_calls_ms": [round(c * 1e3, 2) for c in new_out],
                       "bwe_declip_long_vs_bwe_long": {k: round(v, 4) for k, v in rel.items()},
                       "bwe_declip_long_at_rate": {k: bool(rel[k] >= 1 - spreads[k] - MARGIN) for k in rel},
                       "wall_s": {"bwe_long": [round(r["wall_s"], 2) for r in res["bwe_long"]], "bwe_declip_long": [round(r["wall_s"], 2) for r in res["bwe_declip_long"]]}})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
