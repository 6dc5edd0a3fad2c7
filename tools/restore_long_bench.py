#!/usr/bin/env python
"""Denoiser evaluations/s of whole-recording restoration (Sampler.predict_inpainting_long) at the BASELINE.json configs[1] shape
(L = 184184, T = 36, xi = 0.25), next to predict_inpainting at batch 8 measured IN THE SAME RUN: --recordings recordings of
--windows windows each with a 300 ms gap in every window's owned range, so that pass A and pass B are one batch of
recordings * windows / 2 windows each (8 by default: the same batch as the inpainting runs).  One warm-up of each, then --rounds
alternating pairs (inpainting, restoration) of COMPLETE runs; last, the same recordings restored one window at a time (max_batch = 1).
Per-pass times come from events recorded on the stream around every Sampler.predict call -- no host synchronisation inside a
restoration; what a restoration spends outside the two sampler calls (the plan, the mask upload, one gather and one scatter launch
per pass) is its wall time minus the two spans.  Prints one JSON line and writes it to --out."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_restore_long_bench.json"))
    a = ap.parse_args()
    import torch
    from audio_inpainting_diffusion_amd.config import make_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.init import seeded_init_, seeded_normal
    from audio_inpainting_diffusion_amd.masks import long_gap_mask
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    from audio_inpainting_diffusion_amd.restore import restore_plan
    from audio_inpainting_diffusion_amd.sampler import Sampler, autoregressive_length, autoregressive_overlap
    dev = torch.device("cuda", 0)
    B, L, R, W, T = a.batch, 184184, a.recordings, a.windows, a.T
    args = make_args("maestro22k", audio_len=L, T=T, xi=0.25)
    net = seeded_init_(Unet_CQT_oct_with_attention(args, dev), 0)
    net.prepare()
    smp = Sampler(model=net, diff_params=EDM(args), args=args)
    end = int(autoregressive_overlap(args) * L)
    N = autoregressive_length(L, end, W)
    gap = int(300 * 22050 / 1000)
    mask = torch.ones(1, N)
    jobs_A, jobs_B, _ = restore_plan(torch.zeros(1, N), L, end)               # every window: a gap at the centre of its owned range
    for _, s, _, _, lo, hi in jobs_A + jobs_B:
        c = s + (lo + hi) // 2
        mask[:, c - gap // 2:c - gap // 2 + gap] = 0
    jobs_A, jobs_B, _ = restore_plan(mask, L, end, R=R)
    assert len(jobs_A) + len(jobs_B) == R * W, "every window must hold a gap"
    rec = torch.stack([torch.from_numpy(seeded_normal(7, g, N)) for g in range(R)]).float().mul_(0.063).to(dev)
    mask_inp = long_gap_mask(L, 22050, 300)
    y_inp = (torch.stack([torch.from_numpy(seeded_normal(7, g, L)) for g in range(B)]).float() * 0.063 * mask_inp).to(dev)
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
        if mode == "inpainting":
            smp.seeds = list(range(B))
            out = smp.predict_inpainting(y_inp, mask_inp)
        else:
            out = smp.predict_inpainting_long(rec, mask, max_batch=max_batch, seeds=list(range(R)))
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        assert torch.isfinite(out).all()
        return {"evals": smp.n_evals - n0, "wall_s": wall, "call_s": [s.elapsed_time(e) / 1e3 for s, e, _ in spans], "call_batch": [b for _, _, b in spans]}

    smp.nb_steps = 2                                             # warm-up: plans, graphs and pinned buffers of every batch size the timed runs use
    run("inpainting"), run("restore"), run("restore", 1)
    smp.nb_steps = T
    res = {"inpainting": [], "restore": []}
    for _ in range(a.rounds):
        for mode in ("inpainting", "restore"):
            res[mode].append(run(mode))
    seq = run("restore", 1)
    nA, nB = -(-len(jobs_A) // B), -(-len(jobs_B) // B)
    inp = [r["evals"] / r["call_s"][0] for r in res["inpainting"]]            # the same stream-event span as the passes below
    pass_a = [len(jobs_A) * per_item / sum(r["call_s"][:nA]) for r in res["restore"]]
    pass_b = [len(jobs_B) * per_item / sum(r["call_s"][nA:nA + nB]) for r in res["restore"]]
    whole = [r["evals"] / r["wall_s"] for r in res["restore"]]
    outside = [r["wall_s"] - sum(r["call_s"]) for r in res["restore"]]
    spread = (max(inp) - min(inp)) / max(inp)
    ratio_a, ratio_b = max(pass_a) / max(inp), max(pass_b) / max(inp)
    r2 = lambda v: [round(x, 2) for x in v]                      # noqa: E731
    line = json.dumps({"metric": "denoiser evaluations/s", "segment": L, "T": T, "xi": 0.25, "recordings": R, "windows_per_recording": W, "samples_per_recording": N,
                       "overlap_samples": end, "gap_samples": gap, "jobs_pass_A": len(jobs_A), "jobs_pass_B": len(jobs_B), "max_batch": B, "rounds": a.rounds,
                       "evals_per_window": per_item, "pass_batches": res["restore"][0]["call_batch"],
                       "inpainting_batch": B, "inpainting_complete_run": r2(inp), "inpainting_spread": round(spread, 4),
                       "pass_A": r2(pass_a), "pass_B": r2(pass_b), "restore_whole_call": r2(whole), "outside_sampler_calls_s": [round(c, 4) for c in outside],
                       "pass_A_vs_inpainting": round(ratio_a, 4), "pass_B_vs_inpainting": round(ratio_b, 4),
                       "ratios_within_inpainting_spread": bool(abs(1 - ratio_a) <= spread and abs(1 - ratio_b) <= spread),
                       "one_window_at_a_time": round(seq["evals"] / seq["wall_s"], 2), "one_window_at_a_time_wall_s": round(seq["wall_s"], 2),
                       "batched_wall_s": [round(r["wall_s"], 2) for r in res["restore"]],
                       "batching_gain": round(seq["wall_s"] / min(r["wall_s"] for r in res["restore"]), 3)})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
