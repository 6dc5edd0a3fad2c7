#!/usr/bin/env python
"""Denoiser evaluations/s of blind bandwidth extension (Sampler.predict_blind_bwe) at the BASELINE.json configs[1] shape (L = 184184, T = 36,
xi = 0.25, batch 8), next to predict_bwe "firwin" on the SAME low-passed segments measured IN THE SAME RUN: a Hamming-windowed sinc of --taps
taps at --cutoff Hz.  Blind mode fits the filter inside every guided evaluation -- three launches (statistics, fit, filter) where predict_bwe
makes one -- so it is NOT expected to lie inside the spread of the identical predict_bwe runs plus 0.5 %: the tool states what an evaluation
costs more, not a pass / fail.  One two-step warm-up of each mode and one complete predict_bwe run, reported apart (the first complete run
after the short ones is slower than every later one), then --rounds alternating pairs (predict_bwe, predict_blind_bwe) of COMPLETE runs, each
between two host synchronisations.  Prints one JSON line and writes it to --out."""
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
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--T", type=int, default=36)
    ap.add_argument("--taps", type=int, default=501)
    ap.add_argument("--cutoff", type=float, default=3000.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_blind_bwe_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from audio_inpainting_diffusion_amd import blind
    from audio_inpainting_diffusion_amd.config import make_args
    from audio_inpainting_diffusion_amd.degrade import FIRFilter
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.init import seeded_init_, seeded_normal
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    from audio_inpainting_diffusion_amd.sampler import Sampler
    dev = torch.device("cuda", 0)
    B, L, T, K = a.batch, 184184, a.T, a.taps
    args = make_args("maestro22k", audio_len=L, T=T, xi=0.25)
    args.tester.data_consistency.use = False                    # guidance only
    cfg = blind.settings_of(args)                               # the module defaults: 1024 / 256 / 501
    assert cfg.K == K, "predict_bwe is given as many taps as blind mode designs"
    net = seeded_init_(Unet_CQT_oct_with_attention(args, dev), 0)
    net.prepare()
    smp = Sampler(model=net, diff_params=EDM(args), args=args)
    n = np.arange(K) - (K - 1) / 2
    h = np.sinc(2 * a.cutoff / args.exp.sample_rate * n) * np.hamming(K)
    taps = torch.from_numpy((h / h.sum()).astype(np.float32))
    clean = torch.stack([torch.from_numpy(seeded_normal(7, g, L)) for g in range(B)]).float().mul_(0.063).to(dev)
    y = FIRFilter(taps, L, device=dev).apply(clean)
    per_item = 2 * T - 1                                         # T first evaluations + T - 1 Heun corrections (the last step is Euler)

    def run(mode):
        smp.seeds = list(range(B))
        torch.cuda.synchronize()
        n0, t0 = smp.n_evals, time.perf_counter()
        out = smp.predict_bwe(y, taps, "firwin") if mode == "bwe" else smp.predict_blind_bwe(y)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        assert torch.isfinite(out).all()
        return {"evals": smp.n_evals - n0, "wall_s": wall}

    modes = ("bwe", "blind_bwe")
    smp.nb_steps = 2                                             # warm-up: plans, tables and pinned buffers
    for mode in modes:
        run(mode)
    smp.nb_steps = T
    first = run("bwe")
    res = {mode: [] for mode in modes}
    for _ in range(a.rounds):
        for mode in modes:
            res[mode].append(run(mode))
    fit_hz = [round(float(v), 1) for v in smp.blind_fit[:, 0]]   # (after the last run; a read-back outside every timed span)
    fit_slope = [round(float(v), 1) for v in smp.blind_fit[:, 1]]
    rate = {m: [r["evals"] / r["wall_s"] for r in res[m]] for m in modes}
    assert all(r["evals"] == B * per_item for m in modes for r in res[m])
    spread = (max(rate["bwe"]) - min(rate["bwe"])) / max(rate["bwe"])
    ratio = max(rate["blind_bwe"]) / max(rate["bwe"])
    # per evaluation of the whole batch: 1 / (rate / B) seconds
    ms = {m: 1e3 * B / max(rate[m]) for m in modes}
    r2 = lambda v: [round(x, 2) for x in v]                      # noqa: E731
    line = json.dumps({"metric": "denoiser evaluations/s", "segment": L, "T": T, "xi": 0.25, "batch": B, "filter": "hamming-windowed sinc", "taps": K,
                       "cutoff_hz": a.cutoff, "blind_settings": {"n_fft": cfg.n_fft, "hop": cfg.hop, "K": cfg.K, "floor_dB": cfg.floor_dB, "k_lo": cfg.k_lo,
                                                                "eps": cfg.eps, "cutoff_candidates": int(cfg.cutoffs.size), "slope_candidates": int(cfg.slopes.size)},
                       "rounds": a.rounds, "evals_per_item": per_item, "bwe_first_complete_run": round(first["evals"] / first["wall_s"], 2),
                       "bwe": r2(rate["bwe"]), "blind_bwe": r2(rate["blind_bwe"]), "bwe_spread": round(spread, 4),
                       "blind_bwe_vs_bwe": round(ratio, 4), "inside_spread_plus_margin": bool(ratio >= 1 - spread - MARGIN),
                       "margin": f"spread of the identical predict_bwe runs + {MARGIN:.1%} (stated, not a bar: blind mode adds three launches per evaluation)",
                       "ms_per_batch_evaluation": {m: round(v, 3) for m, v in ms.items()},
                       "blind_cost_ms_per_batch_evaluation": round(ms["blind_bwe"] - ms["bwe"], 3),
                       "blind_fit_last_evaluation_hz": fit_hz, "blind_fit_last_evaluation_db_per_octave": fit_slope,
                       "note": "seeded random weights: the fitted filter of the last evaluation says nothing about restoration quality",
                       "wall_s": {m: [round(r["wall_s"], 2) for r in res[m]] for m in modes}})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
