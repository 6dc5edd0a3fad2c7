#!/usr/bin/env python
"""Denoiser evaluations/s of autoregressive generation at the BASELINE.json configs[1] shape (B = 8, L = 184184, T = 36, xi = 0.25),
N = 3 windows, next to predict_inpainting measured IN THE SAME RUN: one warm-up of each, then --rounds alternating pairs
(inpainting, autoregressive) of COMPLETE runs.  The guided windows 1..N-1 are reported against inpainting (same loop, plus one
aid_ar_carry launch per window); the unconditional window 0 is forward-only and reported separately.  Per-window times come from
events recorded on the stream around every Sampler.predict call -- no host synchronisation inside a piece.  Prints one JSON line."""
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
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--T", type=int, default=36)
    a = ap.parse_args()
    import torch
    from audio_inpainting_diffusion_amd.config import make_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.init import seeded_init_, seeded_normal
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    from audio_inpainting_diffusion_amd.sampler import Sampler, autoregressive_overlap
    dev = torch.device("cuda", 0)
    B, L, N, T = a.batch, 184184, a.windows, a.T
    args = make_args("maestro22k", audio_len=L, T=T, xi=0.25)
    net = seeded_init_(Unet_CQT_oct_with_attention(args, dev), 0)
    net.prepare()
    smp = Sampler(model=net, diff_params=EDM(args), args=args)
    end = int(autoregressive_overlap(args) * L)
    mask = torch.ones(1, L)
    mask[:, end:] = 0                                            # the autoregressive mask for the inpainting runs too: the same loop on the same operator
    y_inp = (torch.stack([torch.from_numpy(seeded_normal(7, g, L)) for g in range(B)]).float() * 0.063 * mask).to(dev)
    per_window = B * (2 * T - 1)                                 # T first evaluations + T - 1 Heun corrections (the last step is Euler), per item

    spans = []
    inner = smp.predict

    def timed_predict(shape, device):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        x = inner(shape, device)
        e1.record()
        spans.append((e0, e1))
        return x
    smp.predict = timed_predict

    def run(mode):
        spans.clear()
        smp.seeds = list(range(B))
        torch.cuda.synchronize()
        n0, t0 = smp.n_evals, time.perf_counter()
        out = smp.predict_inpainting(y_inp, mask) if mode == "inpainting" else smp.predict_autoregressive((B, L), N, dev)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        assert torch.isfinite(out).all()
        return {"evals": smp.n_evals - n0, "wall_s": wall, "window_s": [s.elapsed_time(e) / 1e3 for s, e in spans], "shape": list(out.shape)}

    smp.nb_steps = 2                                             # warm-up: plans, graphs and pinned buffers of both branches
    run("inpainting"), run("autoregressive")
    smp.nb_steps = T
    res = {"inpainting": [], "autoregressive": []}
    for _ in range(a.rounds):
        for mode in ("inpainting", "autoregressive"):
            res[mode].append(run(mode))
    inp = [r["evals"] / r["window_s"][0] for r in res["inpainting"]]            # the same stream-event span as the windows below
    guided = [(N - 1) * per_window / sum(r["window_s"][1:]) for r in res["autoregressive"]]
    uncond = [per_window / r["window_s"][0] for r in res["autoregressive"]]
    whole = [r["evals"] / r["wall_s"] for r in res["autoregressive"]]
    carry = [r["wall_s"] - sum(r["window_s"]) for r in res["autoregressive"]]
    r2 = lambda v: [round(x, 2) for x in v]
    print(json.dumps({"metric": "denoiser evaluations/s", "shape": [B, L], "T": T, "xi": 0.25, "windows": N, "overlap_samples": end,
                      "piece_shape": res["autoregressive"][0]["shape"], "rounds": a.rounds, "evals_per_window": per_window,
                      "inpainting_complete_run": r2(inp), "inpainting_spread": round((max(inp) - min(inp)) / max(inp), 4),
                      "autoregressive_guided_windows": r2(guided), "autoregressive_unconditional_window": r2(uncond),
                      "autoregressive_whole_piece": r2(whole), "outside_windows_s": [round(c, 4) for c in carry],
                      "guided_vs_inpainting": round(max(guided) / max(inp), 4),
                      "window_s": [[round(x, 3) for x in r["window_s"]] for r in res["autoregressive"]]}))


if __name__ == "__main__":
    main()
