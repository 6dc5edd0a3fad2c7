#!/usr/bin/env python
"""Guided denoiser evaluations/s of the restoration entry points at the BASELINE.json configs[1] shape (B = 8, L = 184184,
T = 36 schedule, xi = 0.25): one warm-up step, then --steps timed steps of each mode, alternated --rounds times.  Prints one
JSON line.  Modes: predict_inpainting, predict_bwe firwin (K = 501), predict_bwe cheby1, predict_declipping, predict_resample with the
equivalent torch conv1d lambda (the generic single-stream path), phase retrieval (predict_pr: |STFT| with N = 1024, hop = 256;
norm 2 is the spectral norm there, seeded by power iteration -- its per-item iteration counts are reported), and, on request
(--modes ...,bwe_resample,bwe_resample_lambda), predict_bwe "resample" at --resample-factor (degrade.SincResample) and the same
resampler as a torch lambda through predict_resample (autograd, one stream)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--cheby-order", type=int, default=8)
    ap.add_argument("--cheby-fc", type=float, default=3000.0)
    ap.add_argument("--modes", default="", help="comma-separated subset of the modes (default: all but bwe_resample and bwe_resample_lambda)")
    ap.add_argument("--resample-factor", type=float, default=2.0, help="bandwidth-extension factor of the bwe_resample modes (2 -> 2:1, 1.47 -> 147:100)")
    ap.add_argument("--pr-trajectory", action="store_true", help="after timing, run phase retrieval over the whole schedule once and "
                    "report the power-iteration counts of the spectral-norm seed per evaluation (from sigma_max down to the last step)")
    a = ap.parse_args()
    import numpy as np
    import scipy.signal
    import torch
    from audio_inpainting_diffusion_amd.config import make_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.init import seeded_init_, seeded_normal
    from audio_inpainting_diffusion_amd.masks import mask_from_args
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    from audio_inpainting_diffusion_amd.sampler import Sampler
    dev = torch.device("cuda", 0)
    B, L = 8, 184184
    args = make_args("maestro22k", audio_len=L, T=36, xi=0.25)
    args.tester.data_consistency.use = False
    net = seeded_init_(Unet_CQT_oct_with_attention(args, dev), 0)
    net.prepare()
    clean = torch.stack([torch.from_numpy(seeded_normal(7, g, L)) for g in range(B)]).float() * 0.063
    taps = torch.from_numpy(scipy.signal.firwin(501, 4000, fs=22050).astype(np.float32)).view(1, 1, -1)
    fir = lambda x: torch.nn.functional.conv1d(x.unsqueeze(1), taps.to(x.device), padding="same").squeeze(1)
    ba = scipy.signal.cheby1(a.cheby_order, 0.05, a.cheby_fc, fs=22050)
    mask = mask_from_args(args, generator=torch.Generator().manual_seed(99)).to(dev, torch.float32).reshape(1, L)   # as bench.py
    y_fir = fir(clean).to(dev)
    y_clip = clean.clamp(-0.05, 0.05).to(dev)
    y_inp = (clean.to(dev) * mask)
    from audio_inpainting_diffusion_amd.phase import STFTMagnitude
    pr_op = STFTMagnitude(1024, 256, L, device=dev)
    y_pr = pr_op.apply(clean.to(dev))
    pr_op.diagnostics = []
    smp = Sampler(model=net, diff_params=EDM(args), args=args)
    from audio_inpainting_diffusion_amd.degrade import SincResample, sinc_kernel
    rs_op = SincResample.from_factor(a.resample_factor, L, device=dev)
    rs_k, rs_width = sinc_kernel(rs_op.orig, rs_op.new)
    rs_k = torch.from_numpy(rs_k).float().to(dev)[:, None, :]

    def rs_lambda(x):                                       # torchaudio's resample as torch ops: pad, strided conv1d over the phases, interleave, cut
        xp = torch.nn.functional.pad(x, (rs_width, rs_width + rs_op.orig))
        y = torch.nn.functional.conv1d(xp[:, None], rs_k, stride=rs_op.orig).transpose(1, 2).reshape(x.shape[0], -1)
        return y[..., :rs_op.L_out]

    def setup(mode):
        from audio_inpainting_diffusion_amd.degrade import FIRFilter, HardClip, IIRFilter
        smp.mask = smp.smask = None
        if mode == "inpainting":
            smp.setup_inpainting(y_inp, mask)
            return
        if mode == "bwe_firwin":
            smp.y, smp.spectral = y_fir, FIRFilter(taps, L, device=dev)
        elif mode == "bwe_cheby1":
            op = IIRFilter(*ba, L, device=dev)
            smp.y, smp.spectral = op.apply(clean.to(dev)), op
        elif mode == "declipping":
            smp.y, smp.spectral = y_clip, HardClip(0.05)
        elif mode == "phase_retrieval":
            smp.y, smp.spectral = y_pr, pr_op
        elif mode == "bwe_resample":
            smp.y, smp.spectral = rs_op.apply(clean.to(dev)), rs_op
        elif mode == "bwe_resample_lambda":
            from audio_inpainting_diffusion_amd.sampler import LambdaDegradation
            smp.y, smp.spectral = rs_op.apply(clean.to(dev)), LambdaDegradation(rs_lambda)
        else:
            from audio_inpainting_diffusion_amd.sampler import LambdaDegradation
            smp.y, smp.spectral = y_fir, LambdaDegradation(fir)
        smp.degradation = smp.spectral

    modes = ["inpainting", "bwe_firwin", "bwe_cheby1", "declipping", "resample_lambda", "phase_retrieval"]
    if a.modes:
        modes = [m for m in modes + ["bwe_resample", "bwe_resample_lambda"] if m in a.modes.split(",")]
    rates = {m: [] for m in modes}
    for _ in range(a.rounds):
        for m in modes:
            setup(m)
            smp.seeds = list(range(B))
            st = smp.begin((B, L), dev)
            smp.step(st, 0)                                     # warm-up
            torch.cuda.synchronize()
            n0, t0 = smp.n_evals, time.perf_counter()
            for i in range(1, 1 + a.steps):
                smp.step(st, i)
            torch.cuda.synchronize()
            rates[m].append((smp.n_evals - n0) / (time.perf_counter() - t0))
    best = {m: max(v) for m, v in rates.items()}
    diag = torch.cat([d.cpu() for d in pr_op.diagnostics]) if pr_op.diagnostics else torch.zeros(0, 2)
    it = diag[:, 0]
    seed = {"norm": args.tester.posterior_sampling.norm, "tol": pr_op.seed_tol, "max_iter": pr_op.seed_max_iter, "item_evaluations": int(it.numel()),
            "iterations_min": int(it.min()) if it.numel() else None, "iterations_median": float(it.median()) if it.numel() else None,
            "iterations_max": int(it.max()) if it.numel() else None, "residual_max": float(diag[:, 1].max()) if it.numel() else None}
    if a.pr_trajectory:
        setup("phase_retrieval")
        pr_op.diagnostics = []
        smp.seeds = list(range(B))
        out = smp.predict(tuple((B, L)), dev)
        per_eval = [d.cpu() for d in pr_op.diagnostics]
        it_all = torch.cat([d[:, 0] for d in per_eval])
        seed["trajectory"] = {"steps": args.tester.T, "finite": bool(torch.isfinite(out).all()), "item_evaluations": int(it_all.numel()),
                              "iterations_min": int(it_all.min()), "iterations_median": float(it_all.median()), "iterations_max": int(it_all.max()),
                              "residual_max": float(torch.cat([d[:, 1] for d in per_eval]).max()),
                              "iterations_max_per_launch": [int(d[:, 0].max()) for d in per_eval]}
    print(json.dumps({"metric": "guided denoiser evaluations/s", "shape": [B, L], "steps": a.steps, "rounds": a.rounds,
                      "cheby1": {"order": a.cheby_order, "fc": a.cheby_fc, "fs": 22050}, "fir_taps": 501,
                      "resample": {"factor": a.resample_factor, "orig": rs_op.orig, "new": rs_op.new, "observed": rs_op.L_out},
                      "phase_retrieval": {"win_size": 1024, "hop_size": 256, "seed": seed},
                      "evals_per_s": {m: round(v, 2) for m, v in best.items()}, "all": {m: [round(x, 2) for x in v] for m, v in rates.items()},
                      "vs_inpainting": {m: round(best[m] / best["inpainting"], 4) for m in modes} if "inpainting" in best else None}))


if __name__ == "__main__":
    main()
