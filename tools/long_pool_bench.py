#!/usr/bin/env python
"""A folder of recordings of pairwise DIFFERENT lengths through harness.restore_long, file by file and -- with --pool -- in pooled passes
(Sampler.predict_long_pooled), at the BASELINE.json configs[1] shape (L = 184184, T = 36, xi = 0.25), complete runs: --recordings
recordings of three windows each, the lengths stepping down by --length-step samples from L + 2 * step, a 300 ms gap in every window's
owned range (8 files: 16 jobs in pass A, 8 in pass B).  File by file every file is a sampler call at batch 2 and one at batch 1; pooled,
pass A is two calls at batch 8 and pass B one.

One process runs, --rounds times: the folder file by file, then (with --pool) the folder pooled; and, twice, predict_inpainting at batch
--batch on segments of the same recordings, whose spread + 0.5 % is the margin.  WITHOUT --pool the tool uses only calls that exist
without pooling, so the same file measures a commit that has no ``pool``.  The sampler calls are timed by events on the stream, the
folder by the host clock between synchronisations.

`--gpus N` re-launches the tool as N ranks (dist.launch_ranks: one rank per GPU over RCCL; with fewer GPUs than ranks they share them and
the collectives run on gloo, staged through the host -- a FUNCTIONAL run, labelled `functional_shared_gpu`: function and overhead, not
scaling).  A pass then takes what its slowest rank takes.  Rank 0 prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
README_BATCH_RATE = {1: 39.6, 2: 50.6, 8: 63.7}               # README's batch table, evaluations/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--pool", action="store_true", help="also run the folder pooled, alternated with the file-by-file runs")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--recordings", type=int, default=8)
    ap.add_argument("--length-step", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=8, help="max_batch, per rank")
    ap.add_argument("--T", type=int, default=36)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        from audio_inpainting_diffusion_amd.dist import launch_ranks
        sys.exit(launch_ranks(a.gpus, [os.path.abspath(__file__)] + sys.argv[1:]))

    import torch
    from audio_inpainting_diffusion_amd import dist as D
    from audio_inpainting_diffusion_amd import harness, restore
    from audio_inpainting_diffusion_amd.config import make_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.init import seeded_init_, seeded_normal
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    from audio_inpainting_diffusion_amd.sampler import Sampler, autoregressive_overlap

    rank, local, world = D.init_distributed()
    if world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    if world > 1 and D.bind_rank_to_gpu_numa(local, int(os.environ.get("LOCAL_WORLD_SIZE", world)), log=sys.stderr) is None:
        torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), torch.get_num_threads()) // world))    # (its share of what this command may use)
    shared = int(os.environ.get("AID_SHARED_GPU", "0")) or int(world > torch.cuda.device_count())
    local = local % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    B, L, R, T = a.batch, 184184, a.recordings, a.T
    args = make_args("maestro22k", audio_len=L, T=T, xi=0.25)
    net = seeded_init_(Unet_CQT_oct_with_attention(args, dev), rank)          # ranks start from different weights: the one broadcast makes them equal
    D.broadcast_parameters(net, src=0)
    net.prepare()
    smp = Sampler(model=net, diff_params=EDM(args), args=args)
    end = int(autoregressive_overlap(args) * L)
    step = L - end
    Ns = [L + 2 * step - i * a.length_step for i in range(R)]                 # three windows each: W = ceil((N - L) / step) + 1
    gap = int(300 * 22050 / 1000)
    files, masks, jobs = [], [], []
    for i, N in enumerate(Ns):
        every_A, every_B, _ = restore.restore_plan(torch.zeros(1, N), L, end)
        mask = torch.ones(N)
        for _, s, _, _, lo, hi in every_A + every_B:                          # every window: a gap at the centre of its owned range
            c = s + (lo + hi) // 2
            mask[c - gap // 2:c - gap // 2 + gap] = 0
        A_, B_, _ = restore.restore_plan(mask, L, end)
        assert (len(A_), len(B_)) == (2, 1), f"file {i} of {N} samples: every one of its three windows must hold a gap"
        files.append(torch.from_numpy(seeded_normal(7, i, N)).float().mul_(0.063))
        masks.append(mask)
        jobs.append((len(A_), len(B_)))
    J = [sum(j[p] for j in jobs) for p in range(2)]
    seeds = list(range(R))
    per_item = 2 * T - 1                                         # T first evaluations + T - 1 Heun corrections (the last step is Euler)

    def my_calls(pool):
        """[(pass, batch)] of this rank's sampler calls, in the order they are made"""
        units = [J] if pool else jobs                            # pooled: one unit of both pooled passes; else a unit per file
        return [(p, min(B, hi - c0)) for u in units for p in range(2) for lo, hi in [D.shard_range(u[p], rank, world)] for c0 in range(lo, hi, B)]

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

    def folder(pool):
        spans.clear()
        D.barrier()
        torch.cuda.synchronize()
        n0, t = smp.n_evals, time.perf_counter()
        outs = harness.restore_long(smp, files, masks, seeds=seeds, max_batch=B, device=dev, **({"pool": True} if pool else {}))
        torch.cuda.synchronize()
        wall = time.perf_counter() - t
        assert all(bool(torch.isfinite(o).all()) for o in outs)
        want = my_calls(pool)
        assert [b for _, _, b in spans] == [b for _, b in want], ([b for _, _, b in spans], want)
        calls = [s.elapsed_time(e) / 1e3 for s, e, _ in spans]
        return {"pool": pool, "evals": smp.n_evals - n0, "wall_s": wall, "call_batch": [b for _, b in want],
                "sampler_s": [sum(c for c, (p, _) in zip(calls, want) if p == k) for k in range(2)]}, outs

    seg_y = torch.stack([f[:L] for f in files[:B]]).to(dev)
    seg_m = torch.stack([m[:L] for m in masks[:B]])

    def segments():
        spans.clear()
        smp.seeds = seeds[:B]
        torch.cuda.synchronize()
        n0 = smp.n_evals
        smp.predict_inpainting(seg_y * seg_m.to(dev), seg_m)
        torch.cuda.synchronize()
        smp.seeds = None
        return (smp.n_evals - n0) / sum(s.elapsed_time(e) / 1e3 for s, e, _ in spans)

    modes = [False, True] if a.pool else [False]
    smp.nb_steps = 2                                             # warm-up: plans, graphs and pinned buffers of the batch sizes the timed runs use
    for pool in modes:
        folder(pool)
    if world == 1:
        segments()
    smp.nb_steps = T
    mine, last, batch_rate = [], {}, []
    for k in range(a.rounds):
        if world == 1 and k < 2:
            batch_rate.append(segments())
        for pool in modes:
            res, outs = folder(pool)
            mine.append(res)
            last[pool] = outs
    diff = None
    if a.pool:
        diff = {"max_abs": max(float((p - u).abs().max()) for p, u in zip(last[True], last[False])),
                "max_rel_l2": max(float((p - u).norm() / u.norm()) for p, u in zip(last[True], last[False]))}
    every = D.gather_objects(mine)
    if rank == 0:
        runs = []
        for k in range(len(mine)):
            rs = [e[k] for e in every]
            assert sum(r["evals"] for r in rs) == sum(J) * per_item
            pass_s = [max(r["sampler_s"][p] for r in rs) for p in range(2)]
            wall = max(r["wall_s"] for r in rs)
            runs.append({"pool": rs[0]["pool"], "wall_s": round(wall, 3), "pass_A_evals_per_s": round(J[0] * per_item / pass_s[0], 2),
                         "pass_B_evals_per_s": round(J[1] * per_item / pass_s[1], 2), "folder_evals_per_s": round(sum(J) * per_item / wall, 2),
                         "outside_sampler_calls_s": round(rs[0]["wall_s"] - sum(rs[0]["sampler_s"]), 4), "call_batch_per_rank": [r["call_batch"] for r in rs]})
        wall_of = lambda pool: [r["wall_s"] for r in runs if r["pool"] == pool]                                   # noqa: E731
        spread = abs(batch_rate[0] - batch_rate[1]) / max(batch_rate) if len(batch_rate) == 2 else None
        margin = None if spread is None else spread + 0.005
        pooled = [r for r in runs if r["pool"]]
        derived = (sum(j[0] for j in jobs) / README_BATCH_RATE[2] + sum(j[1] for j in jobs) / README_BATCH_RATE[1]) / (sum(J) / README_BATCH_RATE[8]) if B == 8 and R == 8 else None
        backend = torch.distributed.get_backend() if world > 1 else "single process"
        line = json.dumps({"metric": "denoiser evaluations/s", "tool": "long_pool_bench", "world": world, "backend": backend, "functional_shared_gpu": bool(shared),
                           "note": ("ranks share a GPU and the collectives are staged through the host: function and overhead, NOT scaling" if shared else None),
                           "visible_gpus": torch.cuda.device_count(), "segment": L, "T": T, "xi": 0.25, "recordings": R, "samples_per_recording": Ns,
                           "gap_samples": gap, "jobs_pass_A": J[0], "jobs_pass_B": J[1], "max_batch_per_rank": B, "evals_per_window": per_item,
                           "runs": runs, "inpainting_batch": B, "inpainting_complete_run": [round(v, 2) for v in batch_rate],
                           "inpainting_spread": None if spread is None else round(spread, 5), "margin_spread_plus_0.5pct": None if margin is None else round(margin, 5),
                           "pooled_passes_at_rate": (None if margin is None or not pooled else
                                                     all(min(r["pass_A_evals_per_s"], r["pass_B_evals_per_s"]) >= min(batch_rate) * (1 - margin) for r in pooled)),
                           "pooled_over_unpooled_wall": ([round(u / p, 4) for u, p in zip(wall_of(False), wall_of(True))] if a.pool else None),
                           "pooled_over_unpooled_derived_from_README_batch_table": None if derived is None else round(derived, 3),
                           "pooled_vs_unpooled_largest_difference": diff})
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
    D.barrier()
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
