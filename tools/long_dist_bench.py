#!/usr/bin/env python
"""Whole-recording restoration (Sampler.predict_inpainting_long) shared out over the ranks of a process group, at the BASELINE.json
configs[1] shape (L = 184184, T = 36, xi = 0.25): --recordings recordings of --windows windows each with a 300 ms gap in every window's
owned range (2 x 8: 8 + 8 jobs), complete runs.  tools/restore_long_bench.py plus bench.py --gpus N: `python tools/long_dist_bench.py
--gpus N` re-launches itself as N ranks (dist.launch_ranks: one rank per GPU over RCCL; with fewer GPUs than ranks they share them and
the collectives run on gloo, staged through the host -- a FUNCTIONAL run, labelled `functional_shared_gpu`: it measures function and
overhead, not scaling).  The weights are broadcast once; every rank restores dist.shard_range of each pass (restore.run_passes).

Per rank and pass: the sampler calls are timed by events on the stream; the guard (one all_gather_object before anything is launched)
and the exchange (one dist.gather_outputs, then the scatter of the whole pass) by the host clock between synchronisations -- those
synchronisations exist in this tool only.  A pass takes what its slowest rank takes: aggregate evaluations/s = jobs * (2 T - 1) /
max over ranks (sampler calls + exchange).  Rank 0 prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--recordings", type=int, default=2)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--batch", type=int, default=8, help="max_batch, per rank")
    ap.add_argument("--T", type=int, default=36)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        from audio_inpainting_diffusion_amd.dist import launch_ranks
        sys.exit(launch_ranks(a.gpus, [os.path.abspath(__file__)] + sys.argv[1:]))

    import torch
    from audio_inpainting_diffusion_amd import dist as D
    from audio_inpainting_diffusion_amd import restore
    from audio_inpainting_diffusion_amd.config import make_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.init import seeded_init_, seeded_normal
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    from audio_inpainting_diffusion_amd.sampler import Sampler, autoregressive_length, autoregressive_overlap

    rank, local, world = D.init_distributed()
    if world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    if world > 1 and D.bind_rank_to_gpu_numa(local, int(os.environ.get("LOCAL_WORLD_SIZE", world)), log=sys.stderr) is None:
        torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), torch.get_num_threads()) // world))    # (its share of what this command may use)
    shared = int(os.environ.get("AID_SHARED_GPU", "0")) or int(world > torch.cuda.device_count())
    local = local % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    B, L, R, W, T = a.batch, 184184, a.recordings, a.windows, a.T
    args = make_args("maestro22k", audio_len=L, T=T, xi=0.25)
    net = seeded_init_(Unet_CQT_oct_with_attention(args, dev), rank)          # ranks start from different weights: the one broadcast makes them equal
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nbytes = D.broadcast_parameters(net, src=0)
    torch.cuda.synchronize()
    t_bcast = time.perf_counter() - t0
    net.prepare()
    smp = Sampler(model=net, diff_params=EDM(args), args=args)
    end = int(autoregressive_overlap(args) * L)
    N = autoregressive_length(L, end, W)
    gap = int(300 * 22050 / 1000)
    mask = torch.ones(1, N)
    jobs_A, jobs_B, _ = restore.restore_plan(torch.zeros(1, N), L, end)       # every window: a gap at the centre of its owned range
    for _, s, _, _, lo, hi in jobs_A + jobs_B:
        c = s + (lo + hi) // 2
        mask[:, c - gap // 2:c - gap // 2 + gap] = 0
    jobs_A, jobs_B, _ = restore.restore_plan(mask, L, end, R=R)
    assert len(jobs_A) + len(jobs_B) == R * W, "every window must hold a gap"
    rec = torch.stack([torch.from_numpy(seeded_normal(7, g, N)) for g in range(R)]).float().mul_(0.063).to(dev)
    per_item = 2 * T - 1                                         # T first evaluations + T - 1 Heun corrections (the last step is Euler)
    shares = [[hi - lo for lo, hi in (D.shard_range(len(j), r, world) for j in (jobs_A, jobs_B))] for r in range(world)]
    chunks = [-(-n // B) for n in shares[rank]]                  # sampler calls of this rank per pass

    spans, clock = [], {"guard": [], "allgather": [], "scatter": []}
    inner = smp.predict

    def timed_predict(shape, device):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        x = inner(shape, device)
        e1.record()
        spans.append((e0, e1, int(shape[0])))
        return x
    smp.predict = timed_predict

    def on_the_clock(fn, what):
        def timed(*args, **kw):
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = fn(*args, **kw)
            torch.cuda.synchronize()
            clock[what].append((time.perf_counter() - t, len(clock["allgather"])))
            return res
        return timed
    if D._active():                                              # (the group-less path is left as it is: one scatter launch per chunk, nothing to exchange)
        restore.guard_ranks = on_the_clock(restore.guard_ranks, "guard")
        restore.window_scatter = on_the_clock(restore.window_scatter, "scatter")
        D.gather_outputs = on_the_clock(D.gather_outputs, "allgather")

    def run():
        spans.clear()
        for v in clock.values():
            v.clear()
        D.barrier()
        torch.cuda.synchronize()
        n0, t = smp.n_evals, time.perf_counter()
        out = smp.predict_inpainting_long(rec, mask, max_batch=B, seeds=list(range(R)))
        torch.cuda.synchronize()
        wall = time.perf_counter() - t
        assert torch.isfinite(out).all()
        calls = [s.elapsed_time(e) / 1e3 for s, e, _ in spans]
        sampler_s = [sum(calls[:chunks[0]]), sum(calls[chunks[0]:])]
        exchange_s = [sum(t for t, p in clock["allgather"] if p == k) + sum(t for t, p in clock["scatter"] if p == k + 1) for k in range(2)]
        return {"evals": smp.n_evals - n0, "wall_s": wall, "sampler_s": sampler_s, "exchange_s": exchange_s, "allgather_s": [t for t, _ in clock["allgather"]],
                "guard_s": sum(t for t, _ in clock["guard"]), "call_batch": [b for _, _, b in spans], "checksum": float(out.double().sum())}

    smp.nb_steps = 2                                             # warm-up: plans, graphs and pinned buffers of the batch sizes the timed runs use
    run()
    smp.nb_steps = T
    mine = [run() for _ in range(a.rounds)]
    every = D.gather_objects(mine)
    if rank == 0:
        r4 = lambda v: [round(x, 4) for x in v]                  # noqa: E731
        rounds = []
        for k in range(a.rounds):
            rs = [e[k] for e in every]
            assert len({r["checksum"] for r in rs}) == 1, "the ranks hold different results"
            assert sum(r["evals"] for r in rs) == R * W * per_item
            pass_s = [max(r["sampler_s"][p] + r["exchange_s"][p] for r in rs) for p in range(2)]
            rounds.append({"wall_s": round(max(r["wall_s"] for r in rs), 3),
                           "pass_A_evals_per_s": round(len(jobs_A) * per_item / pass_s[0], 2), "pass_B_evals_per_s": round(len(jobs_B) * per_item / pass_s[1], 2),
                           "whole_call_evals_per_s": round(R * W * per_item / max(r["wall_s"] for r in rs), 2),
                           "sampler_s_per_rank": [r4(r["sampler_s"]) for r in rs], "exchange_s_per_rank": [r4(r["exchange_s"]) for r in rs],
                           "allgather_s_per_rank": [r4(r["allgather_s"]) for r in rs], "guard_s_per_rank": r4([r["guard_s"] for r in rs]),
                           "outside_sampler_calls_s": round(rs[0]["wall_s"] - sum(rs[0]["sampler_s"]), 4), "call_batch_per_rank": [r["call_batch"] for r in rs]})
        backend = torch.distributed.get_backend() if world > 1 else "single process"
        line = json.dumps({"metric": "denoiser evaluations/s", "tool": "long_dist_bench", "world": world, "backend": backend, "functional_shared_gpu": bool(shared),
                           "note": ("ranks share a GPU and the collectives are staged through the host: function and overhead, NOT scaling" if shared else None),
                           "visible_gpus": torch.cuda.device_count(), "rccl_version": D.rccl_version(), "segment": L, "T": T, "xi": 0.25, "recordings": R,
                           "windows_per_recording": W, "samples_per_recording": N, "jobs_pass_A": len(jobs_A), "jobs_pass_B": len(jobs_B),
                           "jobs_per_rank": shares, "max_batch_per_rank": B, "evals_per_window": per_item, "exchange_bytes_per_pass": [len(jobs_A) * L * 4, len(jobs_B) * L * 4],
                           "broadcast_bytes": nbytes, "broadcast_s": round(t_bcast, 3), "rounds": rounds})
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
