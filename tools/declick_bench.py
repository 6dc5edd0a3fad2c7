#!/usr/bin/env python
"""Time of one declick.detect call (audio_inpainting_diffusion_amd/declick.py: aid_ar_score, aid_click_mask and the read-back of the mask)
on --recordings recordings of --samples samples with --clicks clicks and --dropouts dropouts each (declick.add_clicks on four partials plus
coloured noise, seeded), at the default settings or --block / --order / --pad.  --reps calls between two host synchronisations after
--warmup calls; prints one JSON line and writes it to --out.  Under ``rocprofv3 --kernel-trace --stats`` (a run of its own) the per-launch
times of the two kernels are the kernel statistics' ``ar_score_kernel`` and ``click_mask_kernel`` rows."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def recordings(R, N, seed=1):
    import numpy as np
    rng = np.random.default_rng(seed)
    t = np.arange(N)
    rows = []
    for _ in range(R):
        x = sum(a * np.sin(2 * np.pi * f * t / 22050 + rng.uniform(0, 6.28)) for a, f in ((0.3, 220.0), (0.2, 440.0), (0.1, 1330.0), (0.05, 3100.0)))
        w = rng.standard_normal(N + 2)
        rows.append(x + 0.005 * (w[2:] + 0.9 * w[1:-1] + 0.4 * w[:-2]))
    return np.stack(rows).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=2)
    ap.add_argument("--samples", type=int, default=1151150)
    ap.add_argument("--clicks", type=int, default=2000)
    ap.add_argument("--dropouts", type=int, default=20)
    ap.add_argument("--block", type=int, default=2048)
    ap.add_argument("--order", type=int, default=16)
    ap.add_argument("--pad", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from audio_inpainting_diffusion_amd import declick
    y, truth = declick.add_clicks(recordings(a.recordings, a.samples), a.clicks, seed=2, dropouts=a.dropouts)
    yd = torch.from_numpy(y).cuda()
    kw = dict(block=a.block, order=a.order, pad=a.pad)
    for _ in range(a.warmup):
        det = declick.detect(yd, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        det = declick.detect(yd, **kw)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.reps
    cfg = declick.make_settings(**kw)
    t0 = time.perf_counter()
    for _ in range(a.reps):                                          # the two launches alone, without the read-back and the host's report
        declick.mask(yd, declick.score(yd, **cfg.score_args)[0], **cfg.mask_args)
    torch.cuda.synchronize()
    dt_launches = (time.perf_counter() - t0) / a.reps
    sc = declick.detection_scores(det.mask, truth, pad=a.pad)
    res = {"tool": "declick_bench", "recordings": a.recordings, "samples": a.samples, "clicks": a.clicks, "dropouts": a.dropouts, "block": a.block,
           "order": a.order, "pad": a.pad, "reps": a.reps, "ms_per_detect_call": round(dt * 1e3, 4), "ms_two_launches": round(dt_launches * 1e3, 4),
           "n_flagged": det.n_flagged.tolist(), "n_gaps": det.n_gaps.tolist(), "longest_gap": det.longest_gap.tolist(),
           "masked_fraction": [round(int(n) / a.samples, 5) for n in det.n_flagged], "recall": round(sc["recall"], 5), "precision": round(sc["precision"], 5)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
