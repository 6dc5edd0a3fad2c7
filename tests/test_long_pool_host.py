"""CPU tests (no GPU) of restore.run_pooled_passes: the jobs of recordings of DIFFERENT lengths, one restore.Group per length, share the
chunks of one pooled pass A and one pooled pass B -- alone and, over gloo, shared out over the ranks of a process group.  The pattern is
tests/test_long_dist_host.py: the job table is a Python list and the scatter a Python loop, so no kernel is needed; the rows a group's
``gather`` returns name the group and the job, and -- for a window of pass B -- hold a sample that pass A must have left in that group's
``out``; ``predict`` adds the seed it was given.

The fixture: three groups with (2, 1), (1, 1) and (2, 0) jobs in passes A and B, max_batch = 2.  Pooled pass A is five jobs in chunks
[0:2], [2:4], [4:5]; the second chunk holds the one job of group 1 and the first of group 2."""
import os
import queue
import socket
import sys
import traceback

import pytest
import torch
import torch.multiprocessing as mp

L, END, MAX_BATCH = 16, 4, 2
STEP = L - END
LENGTHS = (L + 2 * STEP, L + STEP - 3, L - 2)             # three, two and one window
FILES = ([0], [1], [2, 3])                                # group 2 holds two recordings
SEEDS = [7, 9, 11, 13]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _plans(lengths=LENGTHS):
    """[(jobs_A, jobs_B)] per group: every window of every recording is a job, as restore_plan orders them"""
    from audio_inpainting_diffusion_amd.restore import every_window_plan, restore_windows
    return [every_window_plan(len(files), restore_windows(N, L, END)) for N, files in zip(lengths, FILES)]


def _outs(lengths=LENGTHS):
    return [torch.arange(len(files) * N, dtype=torch.float32).reshape(len(files), N) / 1024 - g for g, (N, files) in enumerate(zip(lengths, FILES))]


class _Stub:
    def __init__(self):
        self.seeds = "untouched"


def _patch(restore, setattr_, events, outs):
    def scatter(x, out, table):
        g = [i for i, o in enumerate(outs) if o is out]
        assert len(g) == 1 and x.shape[0] == len(table) and x.is_contiguous()
        events.append(("scatter", g[0], tuple(table), [int(v) for v in x[:, 0]]))
        for row, (r, s, head, tail, lo, hi) in zip(x, table):
            out[r, s + lo:s + hi] = row[lo:hi]
    setattr_(restore, "job_table", lambda jobs, device: list(jobs))
    setattr_(restore, "window_scatter", scatter)


def _tag(g, job):
    """what names a job in row[0]: group, recording, window"""
    return 10000 * (g + 1) + 100 * job[0] + job[1] // STEP


def _run(restore, lengths=LENGTHS, events=None, setattr_=setattr):
    """restore.run_pooled_passes over stub closures -> (events, outs).  events: ("gather", g, jobs), ("predict", tags of the chunk, seeds of
    the chunk), ("scatter", g, jobs, tags of the rows).  A caller that expects a raise hands in its own list."""
    events = [] if events is None else events
    stub, outs, plans = _Stub(), _outs(lengths), _plans(lengths)
    _patch(restore, setattr_, events, outs)

    def gather_of(g):
        def gather(table):
            events.append(("gather", g, tuple(table)))
            rows = torch.zeros(len(table), L)
            for j, job in enumerate(table):
                rows[j, 0] = _tag(g, job)
                rows[j, 1] = float(outs[g][job[0], job[1]]) if job[2] else 0.0        # pass B: a sample its even neighbour wrote in pass A
            return rows
        return gather

    def predict(win, c0, c1):
        assert torch.is_tensor(win) and 0 <= c0 < c1 <= win.shape[0] and c1 - c0 <= MAX_BATCH and len(stub.seeds) == c1 - c0
        events.append(("predict", [int(v) for v in win[c0:c1, 0]], list(stub.seeds)))
        x = win[c0:c1].clone()
        x[:, 2:] = torch.tensor(stub.seeds, dtype=torch.float32)[:, None] / 65536 + x[:, 1:2] / 2 + torch.arange(L - 2) / 64
        return x
    groups = [restore.Group(outs[g], plans[g], gather_of(g), FILES[g]) for g in range(3)]
    restore.run_pooled_passes(stub, groups, STEP, MAX_BATCH, SEEDS, predict, L=L)
    assert stub.seeds == "untouched"
    return events, outs


def _pooled(p):
    """[(g, job)] of pooled pass p, in group, file and window order"""
    return [(g, job) for g, plan in enumerate(_plans()) for job in plan[p]]


def _seed(g, job):
    return SEEDS[FILES[g][job[0]]] * 65536 + job[1] // STEP


def test_the_jobs_of_three_groups_share_the_chunks_of_two_pooled_passes(monkeypatch):
    from audio_inpainting_diffusion_amd import restore
    assert [(len(a), len(b)) for a, b in _plans()] == [(2, 1), (1, 1), (2, 0)]
    events, outs = _run(restore, setattr_=monkeypatch.setattr)
    A, B = _pooled(0), _pooled(1)
    assert len(A) == 5 and len(B) == 2
    predicts = [e for e in events if e[0] == "predict"]
    # the chunks: [0:2], [2:4], [4:5] of pass A, then [0:2] of pass B; the second spans groups 1 and 2
    chunks = [A[0:2], A[2:4], A[4:5], B[0:2]]
    assert [e[1] for e in predicts] == [[_tag(g, j) for g, j in c] for c in chunks]
    assert [g for g, _ in chunks[1]] == [1, 2] and [g for g, _ in chunks[3]] == [0, 1]
    # the seed of every job: seeds[file] * 65536 + window, the file looked up through the group
    assert [e[2] for e in predicts] == [[_seed(g, j) for g, j in c] for c in chunks]
    assert sorted({s // 65536 for e in predicts for s in e[2]}) == SEEDS
    # every row went to the out of the group that owns its job, once, with that group's sub-table
    scatters = [e for e in events if e[0] == "scatter"]
    assert [(e[1], list(e[2])) for e in scatters] == [(0, [A[0][1], A[1][1]]), (1, [A[2][1]]), (2, [A[3][1]]), (2, [A[4][1]]), (0, [B[0][1]]), (1, [B[1][1]])]
    assert all(e[3] == [_tag(e[1], j) for j in e[2]] for e in scatters)
    # pass B's gathers come after all of pass A's scatters; the group with an empty pass B is neither gathered nor scattered there
    kinds = [(e[0], e[1]) for e in events if e[0] != "predict"]
    assert kinds[:3] == [("gather", 0), ("gather", 1), ("gather", 2)]
    last_A = max(i for i, e in enumerate(events) if e[0] == "scatter" and e[2][0][2] == 0)           # (head == 0: an even window)
    first_B = min(i for i, e in enumerate(events) if e[0] == "gather" and e[2][0][2] > 0)            # (head > 0: an odd window)
    assert last_A < first_B and kinds[-4:] == [("gather", 0), ("gather", 1), ("scatter", 0), ("scatter", 1)]
    assert sum(1 for e in events if e[0] == "gather") == 5
    # pass B read what pass A wrote, and the result is what the groups give one by one through run_passes
    for g in range(3):
        events_g, plans, one = [], _plans(), _outs()
        _patch(restore, monkeypatch.setattr, events_g, one)
        stub = _Stub()

        def gather(table, g=g):
            rows = torch.zeros(len(table), L)
            for j, job in enumerate(table):
                rows[j, 0], rows[j, 1] = _tag(g, job), float(one[g][job[0], job[1]]) if job[2] else 0.0
            return rows

        def predict(win, c0, c1):
            x = win[c0:c1].clone()
            x[:, 2:] = torch.tensor(stub.seeds, dtype=torch.float32)[:, None] / 65536 + x[:, 1:2] / 2 + torch.arange(L - 2) / 64
            return x
        restore.run_passes(stub, one[g], plans[g], STEP, MAX_BATCH, [SEEDS[i] for i in FILES[g]], gather, predict, L=L)
        assert torch.equal(outs[g], one[g]) and not torch.equal(outs[g], _outs()[g])


def _worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from audio_inpainting_diffusion_amd import _lib, dist as D, restore
        r, _, w = D.init_distributed("gloo")
        assert (r, w) == (rank, world) and D._active()
        res = {"rank": rank}
        collectives = []
        inner = D.gather_outputs

        def counted(local, n):
            collectives.append((int(local.shape[0]), int(n)))
            return inner(local, n)
        D.gather_outputs = counted
        # 1. the shared pooled passes
        res["events"], outs = _run(restore)
        res["outs"], res["collectives"] = outs, list(collectives)
        # 2. the guard: rank 1 was given one file of another length
        lengths = (LENGTHS[0], LENGTHS[1] - (1 if rank == 1 else 0), LENGTHS[2])
        res["guard_events"] = []
        try:
            _run(restore, lengths, events=res["guard_events"])
            res["guard"] = None
        except _lib.AidError as e:
            res["guard"] = str(e)
        res["collectives_after_guard"] = len(collectives)
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
def test_every_rank_runs_its_share_of_the_pooled_jobs_and_holds_the_single_process_result(world, monkeypatch):
    from audio_inpainting_diffusion_amd import restore
    from audio_inpainting_diffusion_amd.dist import shard_range
    _, ref = _run(restore, setattr_=monkeypatch.setattr)
    passes = [_pooled(0), _pooled(1)]
    res = _spawn(world)
    done = [[], []]
    for rank, d in enumerate(res):
        predicts = [e for e in d["events"] if e[0] == "predict"]
        gathers = [e for e in d["events"] if e[0] == "gather"]
        mine = []
        for p, jobs in enumerate(passes):
            lo, hi = shard_range(len(jobs), rank, world)
            mine.append(jobs[lo:hi])
            done[p] += jobs[lo:hi]
        # the shares: exactly its slice of each pooled pass, in chunks of at most max_batch, under the unchanged seed rule
        want = [c for share in mine for c in (share[i:i + MAX_BATCH] for i in range(0, len(share), MAX_BATCH))]
        assert [e[1] for e in predicts] == [[_tag(g, j) for g, j in c] for c in want], rank
        assert [e[2] for e in predicts] == [[_seed(g, j) for g, j in c] for c in want], rank
        # it gathered only the rows of its share, group by group
        assert [(e[1], list(e[2])) for e in gathers] == [(g, [j for gg, j in share if gg == g]) for share in mine for g in sorted({g for g, _ in share})], rank
        # one collective per pass, entered by every rank -- with [0, L] rows where its share is empty
        assert d["collectives"] == [(len(mine[0]), 5), (len(mine[1]), 2)], rank
        # every rank scattered the whole of both passes, group by group
        scattered = [(e[1], j) for e in d["events"] if e[0] == "scatter" for j in e[2]]
        assert scattered == passes[0] + passes[1], rank
        assert all(torch.equal(a, b) for a, b in zip(d["outs"], ref)), rank
        # the guard: every rank raises, names rank 1, and nothing was gathered, predicted, exchanged or written
        assert d["guard"] is not None and "rank 1 differs from rank 0 in" in d["guard"] and "shape" in d["guard"], d["guard"]
        assert d["guard_events"] == [] and d["collectives_after_guard"] == 2
    assert done == passes                                                                     # the union: every job once
    if world == 3:
        assert shard_range(2, 2, 3) == (2, 2) and res[2]["collectives"][1] == (0, 2)          # no job in pass B, and it took part
