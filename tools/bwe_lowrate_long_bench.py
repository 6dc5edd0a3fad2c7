#!/usr/bin/env python
"""Denoiser evaluations/s of bandwidth extension of whole low-sample-rate recordings (Sampler.predict_bwe_lowrate_long) at the BASELINE.json
configs[1] shape (L = 184184, T = 36, xi = 0.25), next to predict_bwe "resample" at batch 8 on segments of the same recordings measured IN THE
SAME PROCESS: --recordings recordings of --samples high-rate samples each (2 x 1151150), resampled as a whole at every factor of --factors
(2 -> 2:1, 1.47 -> 147:100).  Every window is a job; the grid is aligned to the input period, so at 147:100 the step shrinks by 105 samples and
the same recording takes nine windows instead of eight.  Per factor: one warm-up of each mode and one complete predict_bwe run, reported apart
as ``bwe_first_complete_run``, then --rounds alternating pairs (predict_bwe, whole recordings) of COMPLETE runs; last, the same recordings one
window at a time (max_batch = 1).  The yardstick is predict_bwe in the same process: a pass is "at rate" when it lies no further below than the
spread of the identical predict_bwe runs plus 0.5 %.  Per-pass times come from events recorded on the stream around every Sampler.predict call
-- no host synchronisation inside a run; what a run spends outside the sampler calls (the plan, one gather and one scatter launch per pass) is
its wall time minus the spans; ``chunk_evals_per_s`` is the rate of every chunk of a run, because a pass whose job count is no multiple of
max_batch ends on a smaller chunk.  Prints one JSON line and writes it to --out."""
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
    ap.add_argument("--factors", type=float, nargs="+", default=[2, 1.47])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_bwe_lowrate_long_bench.json"))
    a = ap.parse_args()
    import torch
    from audio_inpainting_diffusion_amd import lowrate_long, restore
    from audio_inpainting_diffusion_amd.config import make_args
    from audio_inpainting_diffusion_amd.degrade import resample_poly
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.init import seeded_init_, seeded_normal
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    from audio_inpainting_diffusion_amd.sampler import Sampler, autoregressive_overlap
    dev = torch.device("cuda", 0)
    B, L, R, N, T = a.batch, 184184, a.recordings, a.samples, a.T
    args = make_args("maestro22k", audio_len=L, T=T, xi=0.25)
    args.tester.data_consistency.use = False                    # guidance only
    net = seeded_init_(Unet_CQT_oct_with_attention(args, dev), 0)
    net.prepare()
    smp = Sampler(model=net, diff_params=EDM(args), args=args)
    end = int(autoregressive_overlap(args) * L)
    clean = torch.stack([torch.from_numpy(seeded_normal(7, g, N)) for g in range(R)]).float().mul_(0.063).to(dev)
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
    r2 = lambda v: [round(x, 2) for x in v]                      # noqa: E731

    def measure(factor):
        factor = int(factor) if factor == int(factor) else factor
        rate = lowrate_long.rate_of(factor)
        rec = resample_poly(clean, rate.orig, rate.new)         # the whole recording through the resampler
        M, Mw = rec.shape[1], lowrate_long.window_len(L, rate)
        assert M == lowrate_long.low_len(N, rate)
        jobs_A, jobs_B = lowrate_long.lowrate_plan(R, N, L, end, rate)
        starts = [(r, s) for r, s, *_ in (jobs_A + jobs_B) if s + L <= N][:B]
        y_seg = torch.stack([rec[r, (s // rate.orig) * rate.new:(s // rate.orig) * rate.new + Mw] for r, s in starts]).contiguous()
        assert tuple(y_seg.shape) == (B, Mw)

        def run(mode, max_batch=B):
            spans.clear()
            torch.cuda.synchronize()
            n0, t0 = smp.n_evals, time.perf_counter()
            if mode == "bwe":
                smp.seeds = list(range(B))
                out = smp.predict_bwe(y_seg, factor, "resample")
            else:
                out = smp.predict_bwe_lowrate_long(rec, factor, "resample", length=N, max_batch=max_batch, seeds=list(range(R)))
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            assert torch.isfinite(out).all()
            print(f"factor {factor} {mode} max_batch {max_batch} steps {smp.nb_steps}: {wall:.2f} s", file=sys.stderr, flush=True)
            return {"evals": smp.n_evals - n0, "wall_s": wall, "call_s": [s.elapsed_time(e) / 1e3 for s, e, _ in spans], "call_batch": [b for _, _, b in spans]}

        modes = ("bwe", "long")
        smp.nb_steps = 2                                         # warm-up: plans and pinned buffers of every batch size the timed runs use
        for mode in modes:
            run(mode)
        run("long", 1)
        smp.nb_steps = T
        first = run("bwe")                                       # one complete run, reported apart: the first complete run after the short ones is slow
        res = {mode: [] for mode in modes}
        for _ in range(a.rounds):
            for mode in modes:
                res[mode].append(run(mode))
        seq = run("long", 1)
        nA, nB = -(-len(jobs_A) // B), -(-len(jobs_B) // B)
        ref = [r["evals"] / r["call_s"][0] for r in res["bwe"]]  # the same stream-event span as the passes below
        spread = (max(ref) - min(ref)) / max(ref)
        runs = res["long"]
        pa = [len(jobs_A) * per_item / sum(r["call_s"][:nA]) for r in runs]
        pb = [len(jobs_B) * per_item / sum(r["call_s"][nA:nA + nB]) for r in runs]
        whole = [r["evals"] / r["wall_s"] for r in runs]
        outside = [r["wall_s"] - sum(r["call_s"]) for r in runs]
        rel_a, rel_b = max(pa) / max(ref), max(pb) / max(ref)
        return {"factor": factor, "ratio": f"{rate.orig}:{rate.new}", "kernel_taps": rate.K, "low_rate_samples_per_recording": M, "window_row": L + Mw,
                "overlap_samples": restore.aligned_end(L, end, rate.orig), "windows_per_recording": (len(jobs_A) + len(jobs_B)) // R,
                "jobs_pass_A": len(jobs_A), "jobs_pass_B": len(jobs_B), "pass_batches": runs[0]["call_batch"],
                "chunk_evals_per_s": [r2([b * per_item / c for b, c in zip(r["call_batch"], r["call_s"])]) for r in runs],
                "bwe_first_complete_run": round(first["evals"] / first["call_s"][0], 2), "bwe_complete_run": r2(ref), "bwe_spread": round(spread, 4),
                "pass_A": r2(pa), "pass_B": r2(pb), "long_whole_call": r2(whole), "outside_sampler_calls_ms": [round(c * 1e3, 2) for c in outside],
                "pass_A_vs_bwe": round(rel_a, 4), "pass_B_vs_bwe": round(rel_b, 4), "margin": round(spread + MARGIN, 4),
                "pass_A_at_rate": bool(rel_a >= 1 - spread - MARGIN), "pass_B_at_rate": bool(rel_b >= 1 - spread - MARGIN),
                "long_spread": round((max(whole) - min(whole)) / max(whole), 4),
                "one_window_at_a_time": round(seq["evals"] / seq["wall_s"], 2), "one_window_at_a_time_wall_s": round(seq["wall_s"], 2),
                "batched_wall_s": [round(r["wall_s"], 2) for r in runs], "batching_gain": round(seq["wall_s"] / min(r["wall_s"] for r in runs), 3)}

    line = json.dumps({"metric": "denoiser evaluations/s", "segment": L, "T": T, "xi": 0.25, "degradation": "resample", "recordings": R,
                       "samples_per_recording": N, "requested_overlap_samples": end, "max_batch": B, "bwe_batch": B, "rounds": a.rounds,
                       "evals_per_window": per_item, "factors": [measure(f) for f in a.factors]})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
