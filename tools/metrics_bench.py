#!/usr/bin/env python
"""Time of one metrics.evaluate call (audio_inpainting_diffusion_amd/metrics.py: aid_stft_logspec_dist, aid_eval_sums and the read-back of
[R, 8] doubles) on --recordings recordings of --samples samples at --n-fft / --hop: seeded white noise and noise + 0.1 * noise, --region none
or one gap of a tenth of the recording.  --reps calls between two host synchronisations after --warmup calls; prints one JSON line and writes
it to --out.  Under ``rocprofv3 --kernel-trace --stats`` (a run of its own) the per-launch times of the two kernels are the kernel
statistics' ``logspec_dist_kernel`` and ``eval_sums_kernel`` rows."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=2)
    ap.add_argument("--samples", type=int, default=1151150)
    ap.add_argument("--n-fft", type=int, default=2048)
    ap.add_argument("--hop", type=int, default=512)
    ap.add_argument("--region", choices=("none", "gap"), default="none")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from audio_inpainting_diffusion_amd import metrics
    g = torch.Generator().manual_seed(1)
    ref = torch.randn(a.recordings, a.samples, generator=g)
    est = (ref + 0.1 * torch.randn(a.recordings, a.samples, generator=g)).cuda()
    ref = ref.cuda()
    w = None
    if a.region == "gap":
        w = torch.zeros(1, a.samples, device="cuda")
        w[:, a.samples // 2:a.samples // 2 + a.samples // 10] = 1.0
    kw = dict(sample_rate=22050, n_fft=a.n_fft, hop=a.hop)
    for _ in range(a.warmup):
        m = metrics.evaluate(ref, est, w, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        m = metrics.evaluate(ref, est, w, **kw)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.reps
    res = {"tool": "metrics_bench", "recordings": a.recordings, "samples": a.samples, "n_fft": a.n_fft, "hop": a.hop, "region": a.region,
           "frames_per_recording": 1 + a.samples // a.hop, "reps": a.reps, "ms_per_evaluate_call": round(dt * 1e3, 4),
           "lsd": m["lsd"].tolist(), "snr_db": m["snr_db"].tolist(), "si_sdr_db": m["si_sdr_db"].tolist(), "n_frames": m["n_frames"].tolist()}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
