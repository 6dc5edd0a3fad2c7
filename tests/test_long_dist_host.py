"""CPU tests (gloo, no GPU) of whole-recording restoration under a process group: restore.run_passes shares every pass out over the ranks
(dist.shard_range), exchanges once per pass (dist.gather_outputs) and scatters the whole pass on every rank; the guard that compares the
ranks' work before anything is launched; the refusal of ``seeds`` = None under a group.  The pattern is tests/test_dist_gloo.py: spawned
workers, one set per world size, every check inside it.

The job table is a Python list here and the scatter a Python loop, so no kernel is needed; ``predict`` is a stub whose rows name the job
they were computed for, its seed, and -- for a window of pass B -- a sample that pass A must have left in ``out``."""
import os
import queue
import socket
import sys
import traceback

import pytest
import torch
import torch.multiprocessing as mp

L, END, MAX_BATCH, SEEDS = 16, 4, 2, [7, 9]
STEP = L - END
N = L + 4 * STEP                                          # five windows per recording: 0, 2, 4 even, 1, 3 odd


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _case():
    """(jobs_A, jobs_B): two recordings, five even windows and two odd ones are jobs, as restore_plan orders them"""
    from audio_inpainting_diffusion_amd.restore import restore_windows
    wins = restore_windows(N, L, END)
    assert len(wins) == 5
    A = [(0,) + wins[0], (0,) + wins[2], (0,) + wins[4], (1,) + wins[0], (1,) + wins[4]]
    B = [(0,) + wins[1], (1,) + wins[3]]
    return A, B


def _recordings():
    return torch.arange(2 * N, dtype=torch.float32).reshape(2, N) / 1024 - 3


class _Stub:
    def __init__(self):
        self.seeds = "untouched"


def _patch(restore, setattr_):
    def scatter(x, out, table):
        assert x.shape[0] == len(table)
        for row, (r, s, head, tail, lo, hi) in zip(x, table):
            out[r, s + lo:s + hi] = row[lo:hi]
    setattr_(restore, "job_table", lambda jobs, device: list(jobs))
    setattr_(restore, "window_scatter", scatter)


def _run(restore, passes, out, seeds=SEEDS, calls=None, gathers=None):
    """restore.run_passes over the stub -> (calls, gathers): calls = [(jobs of the chunk, seeds of the chunk)], gathers = the sub-tables.
    A caller that expects run_passes to raise hands in its own lists: they hold what was called before the exception."""
    stub, calls, gathers = _Stub(), [] if calls is None else calls, [] if gathers is None else gathers

    def gather(table):
        gathers.append(list(table))
        return list(table)                                # (``win`` is the sub-table itself: predict sees what it is indexed against)

    def predict(win, c0, c1):
        assert win is not None and 0 <= c0 < c1 <= len(win)                # indexed relative to the table gather was given
        jobs = win[c0:c1]
        assert len(stub.seeds) == len(jobs)
        calls.append((tuple(jobs), list(stub.seeds)))
        rows = []
        for (r, s, head, tail, lo, hi), seed in zip(jobs, stub.seeds):
            left = float(out[r, s]) if head else 0.0                        # pass B: a sample its even neighbour wrote in pass A
            rows.append((seed % 65536) * L + torch.arange(L, dtype=torch.float32) + (seed // 65536) / 4 + left / 2)
        return torch.stack(rows)
    restore.run_passes(stub, out, passes, STEP, MAX_BATCH, seeds, gather, predict, L=L)
    assert stub.seeds == "untouched"
    return calls, gathers


def _worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from audio_inpainting_diffusion_amd import _lib, dist as D, restore
        r, _, w = D.init_distributed("gloo")
        assert (r, w) == (rank, world) and D._active()
        _patch(restore, setattr)
        A, B = _case()
        res = {"rank": rank}
        # 1. the shared passes
        out = _recordings()
        res["calls"], res["gathers"] = _run(restore, (A, B), out)
        res["out"] = out.clone()
        # 2. an empty pass in front changes nothing but the digest, which is the same on every rank
        out2 = _recordings()
        _run(restore, ([], A, B), out2)
        res["out_after_empty_pass"] = out2
        # 3. the guard: rank 1 was given another plan
        A_bad = list(A)
        if rank == 1:
            r_, s_, head, tail, lo, hi = A_bad[2]
            A_bad[2] = (r_, s_, head, tail, lo, hi - 1)
        out3 = _recordings()
        res["guard_calls"], res["guard_gathers"] = [], []                  # (owned here: they outlive the exception)
        try:
            _run(restore, (A_bad, B), out3, calls=res["guard_calls"], gathers=res["guard_gathers"])
            res["guard"] = None
        except _lib.AidError as e:
            res["guard"] = str(e)
        res["guard_out_untouched"] = torch.equal(out3, _recordings())
        # ... and other recordings on the last rank
        out4 = _recordings()
        if rank == world - 1:
            out4[1, 5] += 1
        res["guard_recordings_calls"], res["guard_recordings_gathers"] = [], []
        try:
            _run(restore, (A, B), out4, calls=res["guard_recordings_calls"], gathers=res["guard_recordings_gathers"])
            res["guard_recordings"] = None
        except _lib.AidError as e:
            res["guard_recordings"] = str(e)
        mine = _recordings()
        if rank == world - 1:
            mine[1, 5] += 1
        res["guard_recordings_out_untouched"] = torch.equal(out4, mine)
        # 4. L is needed under a group
        try:
            restore.run_passes(_Stub(), _recordings(), (A, B), STEP, MAX_BATCH, SEEDS, lambda t: t, lambda *a: None)
            res["no_L"] = None
        except _lib.AidError as e:
            res["no_L"] = str(e)
        # 5. the refusal of seeds = None, before the device of y is judged
        y = _recordings()
        for name, seeds in (("refusal", None), ("refusal_with_seeds", SEEDS)):
            try:
                restore.check_batch(y, 8, seeds, "restoration of whole recordings")
                res[name] = None
            except _lib.AidError as e:
                res[name] = str(e)
        D.barrier()
        q.put(res)
        torch.distributed.destroy_process_group()
    except BaseException:
        q.put({"rank": rank, "error": traceback.format_exc()})
        raise


def _spawn(world, timeout=120):
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(world):
            res.append(q.get(timeout=timeout))
            assert "error" not in res[-1], res[-1]["error"]
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    except queue.Empty:
        pytest.fail(f"a worker of world {world} did not answer within {timeout} s")
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join(timeout=10)
    return sorted(res, key=lambda d: d["rank"])


@pytest.mark.parametrize("world", [2, 3])
def test_every_rank_runs_its_share_and_every_rank_holds_the_single_process_result(world, monkeypatch):
    from audio_inpainting_diffusion_amd import _lib, restore
    from audio_inpainting_diffusion_amd.dist import shard_range
    A, B = _case()
    assert len(A) == 5 and len(B) == 2
    # the same call without a group, in this process
    _patch(restore, monkeypatch.setattr)
    ref = _recordings()
    ref_calls, ref_gathers = _run(restore, (A, B), ref)
    assert [len(c[0]) for c in ref_calls] == [2, 2, 1, 2] and ref_gathers == [A, B] and not torch.equal(ref, _recordings())
    rule = lambda jobs: [SEEDS[r] * restore.SEED_STRIDE + s // STEP for r, s, *_ in jobs]      # noqa: E731
    assert [s for c in ref_calls for s in c[1]] == rule(A + B)
    with pytest.raises(_lib.AidError, match="GPU only") as refused:                          # (y is on the host: the device, judged last, is the one refusal left)
        restore.check_batch(_recordings(), 8, None, "restoration of whole recordings")
    assert "seeds" not in str(refused.value)                                                 # without a group: no word about seeds

    res = _spawn(world)
    seen = {"A": [], "B": []}
    for rank, d in enumerate(res):
        for name, jobs in (("A", A), ("B", B)):
            lo, hi = shard_range(len(jobs), rank, world)
            mine = [c for c in d["calls"] if set(c[0]) <= set(jobs)]
            done = [j for c in mine for j in c[0]]
            assert done == jobs[lo:hi], (rank, name)                                         # exactly its share, in order
            assert [len(c[0]) for c in mine] == [min(MAX_BATCH, hi - c0) for c0 in range(lo, hi, MAX_BATCH)]
            assert all(c[1] == rule(c[0]) for c in mine)                                     # the seed rule, per chunk
            assert [g for g in d["gathers"] if set(g) <= set(jobs)] == ([jobs[lo:hi]] if hi > lo else [])
            seen[name] += done
        assert sum(len(c[0]) for c in d["calls"]) == sum(shard_range(len(j), rank, world)[1] - shard_range(len(j), rank, world)[0] for j in (A, B))
    assert seen["A"] == A and seen["B"] == B                                                 # the union: every job once
    if world == 3:
        assert shard_range(len(B), 2, 3) == (2, 2) and all(set(c[0]) <= set(A) for c in res[2]["calls"])     # no job in pass B, and it returned
    for d in res:
        assert torch.equal(d["out"], ref) and torch.equal(d["out_after_empty_pass"], ref)
        # the guard: every rank raises, names rank 1 and what differs, and nothing was predicted or written
        assert d["guard"] is not None and "rank 1 differs from rank 0 in plan" in d["guard"] and "rank 2" not in d["guard"]
        assert d["guard_calls"] == [] and d["guard_gathers"] == [] and d["guard_out_untouched"]
        assert d["guard_recordings"] is not None and f"rank {world - 1} differs from rank 0 in recordings" in d["guard_recordings"]
        assert d["guard_recordings_calls"] == [] and d["guard_recordings_gathers"] == [] and d["guard_recordings_out_untouched"]
        assert d["no_L"] is not None and "L" in d["no_L"]
        assert d["refusal"] is not None and "seeds" in d["refusal"] and "GPU only" not in d["refusal"]
        assert d["refusal_with_seeds"] is not None and "GPU only" in d["refusal_with_seeds"]
