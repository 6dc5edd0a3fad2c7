#!/usr/bin/env python
"""Denoiser evaluations/s of blind bandwidth extension of whole recordings (Sampler.predict_blind_bwe_long) at the BASELINE.json configs[1]
shape (L = 184184, T = 36, xi = 0.25, max_batch 8): --recordings recordings of --samples samples (2 x 1151150: 8 + 8 windows), recording r
through a Hamming-windowed sinc of --taps taps at 3 kHz (even r) or 5 kHz (odd r), --probes probe windows each.  Everything IN THE SAME RUN,
complete T-step runs between two host synchronisations, --rounds alternating rounds of

  bwe_long   predict_bwe_long on the same recordings with ONE of the filters (the yardstick of stage 2: the same kernel family),
  stage2     predict_blind_bwe_long with frozen_taps = the rows stage 1 fitted: stage 2 alone, one tap row per window,
  stage1     blind_long.estimate_filters: the energy launch, its read-back and the chunks of probes through PooledBlindLowpass (one stream),
  blind      predict_blind_bwe on --recordings x --probes segments: the per-item fit on sub-batch streams, at the batch of a stage-1 chunk.

Stage 2 is expected at bwe_long's rate within the spread of the identical bwe_long runs plus 0.5 %; stage 1 has no target: the tool states
its ratio to ``blind`` and its share of the whole call (stage1 / (stage1 + stage2) in wall time).  Prints one JSON line and writes it to --out."""
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
    ap.add_argument("--probes", type=int, default=4)
    ap.add_argument("--max-batch", type=int, default=8)
    ap.add_argument("--T", type=int, default=36)
    ap.add_argument("--taps", type=int, default=501)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_blind_bwe_long_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from audio_inpainting_diffusion_amd import blind, blind_long, bwe_long
    from audio_inpainting_diffusion_amd.config import make_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.init import seeded_init_, seeded_normal
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    from audio_inpainting_diffusion_amd.sampler import Sampler, autoregressive_overlap
    dev = torch.device("cuda", 0)
    R, N, L, T, K, MB = a.recordings, a.samples, 184184, a.T, a.taps, a.max_batch
    args = make_args("maestro22k", audio_len=L, T=T, xi=0.25)
    args.tester.data_consistency.use = False                    # guidance only
    cfg = blind.settings_of(args)                               # the module defaults: 1024 / 256 / 501
    assert cfg.K == K, "predict_bwe_long is given as many taps as blind mode designs"
    end = int(autoregressive_overlap(args) * L)
    net = seeded_init_(Unet_CQT_oct_with_attention(args, dev), 0)
    net.prepare()
    smp = Sampler(model=net, diff_params=EDM(args), args=args)
    n = np.arange(K) - (K - 1) / 2
    sincs = []
    for fc in (3000.0, 5000.0):
        h = np.sinc(2 * fc / args.exp.sample_rate * n) * np.hamming(K)
        sincs.append(torch.from_numpy((h / h.sum()).astype(np.float32)))
    clean = torch.stack([torch.from_numpy(seeded_normal(7, g, N)) for g in range(R)]).float().mul_(0.063)
    y = torch.cat([torch.nn.functional.conv1d(clean[r:r + 1, None], sincs[r % 2][None, None], padding="same").squeeze(1) for r in range(R)]).to(dev)
    jobs = sum(len(p) for p in bwe_long.bwe_plan(R, N, L, end, K))
    seeds = list(range(R))
    n_probe = R * min(a.probes, len(blind_long.candidate_starts(N, L, end, K)))
    seg = torch.cat([y[r:r + 1, p * (L - end):p * (L - end) + L] for r in range(R) for p in range(n_probe // R)]).contiguous()
    per_item = 2 * T - 1                                         # T first evaluations + T - 1 Heun corrections (the last step is Euler)
    fitted = {}

    def run(mode):
        smp.seeds = list(range(seg.shape[0]))
        torch.cuda.synchronize()
        n0, t0 = smp.n_evals, time.perf_counter()
        if mode == "bwe_long":
            out = smp.predict_bwe_long(y, sincs[0], "firwin", max_batch=MB, seeds=seeds)
        elif mode == "stage2":
            out = smp.predict_blind_bwe_long(y, probes=a.probes, max_batch=MB, seeds=seeds, frozen_taps=fitted["taps"])
        elif mode == "stage1":
            fitted["taps"], fitted["fit"], fitted["probes"] = blind_long.estimate_filters(smp, y, cfg, L, end, a.probes, MB, seeds)
            out = fitted["taps"]
        else:
            out = smp.predict_blind_bwe(seg)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        assert torch.isfinite(out).all()
        return {"evals": smp.n_evals - n0, "wall_s": wall}

    modes = ("bwe_long", "stage1", "stage2", "blind")
    smp.nb_steps = 2                                             # warm-up: plans, tables and pinned buffers
    for mode in modes:
        run(mode)
    smp.nb_steps = T
    first = run("bwe_long")
    res = {mode: [] for mode in modes}
    for _ in range(a.rounds):
        for mode in modes:
            res[mode].append(run(mode))
    want = {"bwe_long": jobs, "stage2": jobs, "stage1": n_probe, "blind": n_probe}
    assert all(r["evals"] == want[m] * per_item for m in modes for r in res[m]), {m: [r["evals"] for r in res[m]] for m in modes}
    rate = {m: [r["evals"] / r["wall_s"] for r in res[m]] for m in modes}
    spread = (max(rate["bwe_long"]) - min(rate["bwe_long"])) / max(rate["bwe_long"])
    ratio2 = max(rate["stage2"]) / max(rate["bwe_long"])
    ratio1 = max(rate["stage1"]) / max(rate["blind"])
    s1, s2 = min(r["wall_s"] for r in res["stage1"]), min(r["wall_s"] for r in res["stage2"])
    fit_hz = blind.fit_in_hz(fitted["fit"], cfg, args.exp.sample_rate).cpu()
    r2 = lambda v: [round(x, 2) for x in v]                      # noqa: E731
    line = json.dumps({"metric": "denoiser evaluations/s", "segment": L, "T": T, "xi": 0.25, "max_batch": MB, "recordings": R, "samples": N,
                       "windows": jobs, "probes_per_recording": n_probe // R, "filters": "hamming-windowed sincs at 3 kHz (even recordings) and 5 kHz (odd)", "taps": K,
                       "blind_settings": {"n_fft": cfg.n_fft, "hop": cfg.hop, "K": cfg.K, "cutoff_candidates": int(cfg.cutoffs.size), "slope_candidates": int(cfg.slopes.size)},
                       "rounds": a.rounds, "evals_per_item": per_item, "bwe_long_first_complete_run": round(first["evals"] / first["wall_s"], 2),
                       "bwe_long": r2(rate["bwe_long"]), "stage2": r2(rate["stage2"]), "stage1": r2(rate["stage1"]), "blind_bwe_same_batch": r2(rate["blind"]),
                       "bwe_long_spread": round(spread, 4), "stage2_vs_bwe_long": round(ratio2, 4), "stage2_inside_spread_plus_margin": bool(ratio2 >= 1 - spread - MARGIN),
                       "margin": f"spread of the identical predict_bwe_long runs + {MARGIN:.1%}",
                       "stage1_vs_blind_bwe": round(ratio1, 4), "stage1_share_of_the_call": round(s1 / (s1 + s2), 4),
                       "stage1_note": "one stream (a group may straddle the network's sub-batch split) and, in its wall time, the energy launch with its read-back and the gather of every chunk; no target",
                       "fit_hz": [round(float(v), 1) for v in fit_hz[:, 0]], "fit_db_per_octave": [round(float(v), 1) for v in fit_hz[:, 1]], "probe_starts": fitted["probes"],
                       "note": "seeded random weights: the fitted filters say nothing about restoration quality",
                       "wall_s": {m: [round(r["wall_s"], 2) for r in res[m]] for m in modes}})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
