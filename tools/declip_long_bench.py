#!/usr/bin/env python
"""Denoiser evaluations/s of declipping whole recordings (Sampler.predict_declipping_long) at the BASELINE.json configs[1] shape
(L = 184184, T = 36, xi = 0.25), next to predict_declipping at batch 8 on segments of the same recordings measured IN THE SAME RUN:
--recordings recordings of --windows windows each (2 x 8: 1151150 samples), clipped at --clip so that every window is a job and pass A
and pass B are one batch of recordings * windows / 2 windows each (8 by default: the same batch as the predict_declipping runs).  One
warm-up of each and one complete predict_declipping run, reported apart as ``declipping_first_complete_run`` (the first complete run
after the two-step ones is slower than every later one), then --rounds alternating triples (predict_declipping, whole recordings, whole
recordings with ClipObserved.rows hidden) of COMPLETE runs; last, the same recordings one window at a time (max_batch = 1).  With ``rows`` hidden the per-item operator
forces network.denoise_guided onto one stream, as before ClipObserved offered it; the gain of the sub-batch stream path is the ratio
of the two, to be read against the spreads of the identical runs of each of the three (``rows_gain_exceeds_every_spread``).
Per-pass times come from events recorded on the stream around every Sampler.predict call -- no host synchronisation inside a run;
what a run spends outside the sampler calls (the plan, one gather and one scatter launch per pass) is its wall time minus the spans.
Prints one JSON line and writes it to --out."""
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
    ap.add_argument("--clip", type=float, default=0.05)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_declip_long_bench.json"))
    a = ap.parse_args()
    import torch
    from audio_inpainting_diffusion_amd import declip_long
    from audio_inpainting_diffusion_amd.config import make_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.init import seeded_init_, seeded_normal
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    from audio_inpainting_diffusion_amd.sampler import Sampler, autoregressive_length, autoregressive_overlap
    dev = torch.device("cuda", 0)
    B, L, R, W, T = a.batch, 184184, a.recordings, a.windows, a.T
    args = make_args("maestro22k", audio_len=L, T=T, xi=0.25)
    args.tester.data_consistency.use = False                    # guidance only, as the reference's declipping (predict_declipping has no projection)
    net = seeded_init_(Unet_CQT_oct_with_attention(args, dev), 0)
    net.prepare()
    smp = Sampler(model=net, diff_params=EDM(args), args=args)
    end = int(autoregressive_overlap(args) * L)
    N = autoregressive_length(L, end, W)
    rec = torch.stack([torch.from_numpy(seeded_normal(7, g, N)) for g in range(R)]).float().mul_(0.063).clamp_(-a.clip, a.clip).to(dev)
    jobs_A, jobs_B, _ = declip_long.declip_plan(rec, declip_long.clip_levels(a.clip, R), L, end)
    assert len(jobs_A) + len(jobs_B) == R * W, "every window must hold a clipped sample"
    starts = [(r, s) for r, s, *_ in (jobs_A + jobs_B) if s + L <= N][:B]
    y_seg = torch.stack([rec[r, s:s + L] for r, s in starts]).contiguous()
    assert y_seg.shape[0] == B
    per_item = 2 * T - 1                                         # T first evaluations + T - 1 Heun corrections (the last step is Euler)

    class NoRows:
        """ClipObserved with ``rows`` hidden: network.denoise_guided keeps a per-item operator without it on one stream"""
        shared_mask = False

        def __init__(self, state, clip):
            self._op = with_rows(state, clip)
            self.apply, self.adjoint, self.project = self._op.apply, self._op.adjoint, self._op.project
    with_rows = declip_long.ClipObserved

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
        if mode == "declipping":
            smp.seeds = list(range(B))
            out = smp.predict_declipping(y_seg, a.clip)
        else:
            declip_long.ClipObserved = NoRows if mode == "long_no_rows" else with_rows
            try:
                out = smp.predict_declipping_long(rec, a.clip, max_batch=max_batch, seeds=list(range(R)))
            finally:
                declip_long.ClipObserved = with_rows
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        assert torch.isfinite(out).all()
        return {"evals": smp.n_evals - n0, "wall_s": wall, "call_s": [s.elapsed_time(e) / 1e3 for s, e, _ in spans], "call_batch": [b for _, _, b in spans]}

    modes = ("declipping", "long", "long_no_rows")
    smp.nb_steps = 2                                             # warm-up: plans and pinned buffers of every batch size the timed runs use
    for mode in modes:
        run(mode)
    run("long", 1)
    smp.nb_steps = T
    first = run("declipping")                                    # one complete run, reported apart: the first complete run after the short ones is slow
    res = {mode: [] for mode in modes}
    for _ in range(a.rounds):
        for mode in modes:
            res[mode].append(run(mode))
    seq = run("long", 1)
    nA, nB = -(-len(jobs_A) // B), -(-len(jobs_B) // B)
    ref = [r["evals"] / r["call_s"][0] for r in res["declipping"]]            # the same stream-event span as the passes below
    spread = (max(ref) - min(ref)) / max(ref)
    r2 = lambda v: [round(x, 2) for x in v]                      # noqa: E731

    def passes(runs):
        pa = [len(jobs_A) * per_item / sum(r["call_s"][:nA]) for r in runs]
        pb = [len(jobs_B) * per_item / sum(r["call_s"][nA:nA + nB]) for r in runs]
        return pa, pb, [r["evals"] / r["wall_s"] for r in runs], [r["wall_s"] - sum(r["call_s"]) for r in runs]
    pa, pb, whole, outside = passes(res["long"])
    pa0, pb0, whole0, _ = passes(res["long_no_rows"])
    gain = max(whole) / max(whole0)
    spread_l, spread_0 = (max(whole) - min(whole)) / max(whole), (max(whole0) - min(whole0)) / max(whole0)
    line = json.dumps({"metric": "denoiser evaluations/s", "segment": L, "T": T, "xi": 0.25, "clip": a.clip, "recordings": R, "windows_per_recording": W,
                       "samples_per_recording": N, "overlap_samples": end, "clipped_fraction": round(float((rec.abs() >= a.clip).float().mean()), 4),
                       "jobs_pass_A": len(jobs_A), "jobs_pass_B": len(jobs_B), "max_batch": B, "rounds": a.rounds, "evals_per_window": per_item,
                       "pass_batches": res["long"][0]["call_batch"],
                       "declipping_batch": B, "declipping_first_complete_run": round(first["evals"] / first["call_s"][0], 2),
                       "declipping_complete_run": r2(ref), "declipping_spread": round(spread, 4),
                       "pass_A": r2(pa), "pass_B": r2(pb), "long_whole_call": r2(whole), "outside_sampler_calls_ms": [round(c * 1e3, 2) for c in outside],
                       "pass_A_vs_declipping": round(max(pa) / max(ref), 4), "pass_B_vs_declipping": round(max(pb) / max(ref), 4),
                       "rows_hidden_pass_A": r2(pa0), "rows_hidden_pass_B": r2(pb0), "rows_hidden_whole_call": r2(whole0),
                       "long_spread": round(spread_l, 4), "rows_hidden_spread": round(spread_0, 4),
                       "rows_gain": round(gain, 4), "rows_gain_exceeds_every_spread": bool(gain - 1 > max(spread, spread_l, spread_0)),
                       "one_window_at_a_time": round(seq["evals"] / seq["wall_s"], 2), "one_window_at_a_time_wall_s": round(seq["wall_s"], 2),
                       "batched_wall_s": [round(r["wall_s"], 2) for r in res["long"]],
                       "batching_gain": round(seq["wall_s"] / min(r["wall_s"] for r in res["long"]), 3)})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
