"""Restoration of whole recordings, longer than one model segment, with gaps anywhere -- in two batched sampler passes.

Windows of L = args.exp.audio_len samples lie on the autoregressive grid: window w starts at w * step, step = L - end,
end = int(overlap * L) (sampler.autoregressive_overlap), so neighbours share ``end`` samples.  Every sample of the recording is OWNED
by exactly one window:

    even w                      [s_w, s_w + L)                  the whole window
    odd  w                      [s_w + end, s_w + L - end)      the middle its two even neighbours leave free
    odd last w (no neighbour)   [s_w + end, s_w + L)

Even windows do not overlap one another, so pass A inpaints all of them that hold a gap as ONE batch, each from its own observations.
Pass B does the same for the odd windows; their first and last ``end`` samples are taken as observed from the result restored so far
(what pass A wrote there, or the recording), the way a window of autoregressive generation is conditioned on the tail of the one before
it.  A window whose owned range has no gap is no job and costs nothing.  Hard concatenation, no cross-fade (as the reference's
autoregressive mode, testing/edm_sampler.py:416).

``restore_plan`` is host code (the only part that looks at the mask on the host); ``window_gather`` / ``window_scatter`` launch the
two HIP kernels of csrc/aid_restore.hip; ``restore_passes`` is the pass code, driven with anything that has ``predict_inpainting``.

This module is also the one home of what the other whole-recording modes share (declip_long.py, bwe_long.py, bwe_iir_long.py, bwe_declip_long.py,
lowrate_long.py, phase_long.py, spec_long.py, blind_long.py; DESIGN.md, "The window scheme of whole recordings"): ``aligned_end`` / ``trimmed_windows`` /
``every_window_plan`` (the grid aligned to a period, the ownership trimmed by an operator's reach, every window a job), ``check_rows`` /
``check_batch`` (the refusals every mode raises), ``WindowOperator`` (the base of the window operators) and ``run_passes`` (the pass loop).
``run_pooled_passes`` is that loop over several ``Group`` records, one per recording length: the jobs of all lengths share the chunks of one
pooled pass A and one pooled pass B; ``run_passes`` is its one-group case.  The seven modes that pool are one ``LongTask``
record each in ``LONG_TASKS``, declared by the mode's module, and ``run_task`` is their one driver, for one length and for many.

Under an active process group (dist.py) ``run_passes`` shares every pass out over the ranks -- contiguous shares, the unchanged seed rule,
one all-gather of the windows per pass, the whole pass scattered on every rank -- after ``guard_ranks`` has compared what the ranks were
given (``pass_digest``); host code only, the kernels and the sampler rounds are the same.
"""
from __future__ import annotations

from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from . import degrade
from . import dist as _dist

Job = Tuple[int, int, int, int, int, int]            # (recording r, start s, head, tail, lo, hi)
SEED_STRIDE = 65536                                  # the job of window w of recording r runs with seed seeds[r] * SEED_STRIDE + w
SCATTER_JOBS = 65535                                 # the most jobs one aid_window_scatter launch takes (csrc/aid_restore.hip)


def restore_windows(N: int, L: int, end: int) -> List[Tuple[int, int, int, int, int]]:
    """(start s, head, tail, lo, hi) of every window of a recording of N samples; [lo, hi) is the owned range relative to s, cut at N."""
    N, L, end = int(N), int(L), int(end)
    if N < 1 or L < 1:
        raise _lib.AidError(f"restore_plan: N = {N} and L = {L} must be >= 1")
    if not (1 <= end and 2 * end < L):
        raise _lib.AidError(f"restore_plan: the overlap end = {end} must lie in [1, L/2) for L = {L}, so that an odd window owns a non-empty middle")
    step = L - end
    W = max(1, -(-(N - L) // step) + 1)
    wins = []
    for w in range(W):
        s = w * step
        if w % 2 == 0:
            head, tail, lo, hi = 0, 0, 0, L
        elif w == W - 1:
            head, tail, lo, hi = end, 0, end, L
        else:
            head, tail, lo, hi = end, end, end, L - end
        wins.append((s, head, tail, lo, min(hi, N - s)))
    return wins


def aligned_end(L: int, end: int, period: int) -> int:
    """end' >= end with (L - end') a multiple of ``period``: every window of the grid then starts at a multiple of it"""
    return int(end) + (int(L) - int(end)) % int(period)


def trimmed_windows(N: int, L: int, end: int, K: int) -> List[Tuple[int, int, int, int, int]]:
    """(start s, head, tail, lo, hi) of every window of a recording of N samples seen through an operator that reaches K - 1 samples (a
    filter of K taps); [lo, hi) is the owned range relative to s, cut at N.  The grid is restore_windows'; heads, tails and owned ranges are
    trimmed by m = K - 1, so that every window owns only samples whose observation it used:

        even w                      [s_w + (m if w else 0), s_w + L - (0 if last else m))
        odd  w                      [s_w + end - m, s_w + L - end + m)       head = tail = end - m known from the result so far
        odd last w (no neighbour)   [s_w + end - m, s_w + L)                 head = end - m, tail = 0

    which tiles [0, N) whenever end >= 2 m (required with more than one window)."""
    K = int(K)
    if K < 1:
        raise _lib.AidError(f"trimmed_windows: K = {K} taps must be >= 1")
    grid = restore_windows(N, L, end)                                      # (N, L >= 1; end in [1, L/2))
    N, L, end, m, W = int(N), int(L), int(end), K - 1, len(grid)
    if W > 1 and end < 2 * m:
        raise _lib.AidError(f"trimmed_windows: the overlap end = {end} must be >= 2 (K - 1) = {2 * m} for a filter of K = {K} taps, so that every "
                            "sample is observed with its whole filter support in the window that owns it")
    wins = []
    for w, (s, *_) in enumerate(grid):
        last = w == W - 1
        if w % 2 == 0:
            head, tail, lo, hi = 0, 0, (m if w else 0), (L if last else L - m)
        elif last:
            head, tail, lo, hi = end - m, 0, end - m, L
        else:
            head, tail, lo, hi = end - m, end - m, end - m, L - end + m
        wins.append((s, head, tail, lo, min(hi, N - s)))
    return wins


def every_window_plan(R: int, wins) -> Tuple[List[Job], List[Job]]:
    """(jobs_A, jobs_B): every even / odd window of ``wins`` for every recording as (r, s, head, tail, lo, hi), ordered by recording and
    window -- the plan of a degradation that touches all samples, so that every window is a job."""
    jobs = ([], [])
    for r in range(int(R)):
        for w, win in enumerate(wins):
            jobs[w % 2].append((r,) + win)
    return jobs


def restore_plan(mask: torch.Tensor, L: int, end: int, R: Optional[int] = None) -> Tuple[List[Job], List[Job], int]:
    """mask [R, N] or [1, N] (1 = observed, 0 = gap; any dtype / device) -> (jobs_A, jobs_B, N_pad): the even / odd windows whose owned
    range holds a zero of the mask, as (r, s, head, tail, lo, hi), ordered by recording and window; N_pad = L + (W - 1) * step is the
    length the grid covers (samples from N on do not exist: nobody owns them and they make no window a job).
    ``R``: number of recordings a one-row mask is shared by (its jobs are repeated for every recording); default mask.shape[0]."""
    if mask.dim() == 1:
        mask = mask.reshape(1, -1)
    if mask.dim() != 2:
        raise _lib.AidError(f"restore_plan: mask must be [R, N] or [1, N], got {tuple(mask.shape)}")
    rows, N = mask.shape
    R = rows if R is None else int(R)
    if rows not in (1, R):
        raise _lib.AidError(f"restore_plan: a mask of {rows} rows for {R} recordings")
    wins = restore_windows(N, L, end)
    gap = (mask.detach().to("cpu") == 0)
    # zeros before sample q, per row: a window is active when the count differs between the ends of its owned range
    cum = torch.zeros((rows, N + 1), dtype=torch.int64)
    cum[:, 1:] = torch.cumsum(gap, dim=1)
    jobs_A: List[Job] = []
    jobs_B: List[Job] = []
    for r in range(R):
        c = cum[r if rows > 1 else 0]
        for w, (s, head, tail, lo, hi) in enumerate(wins):
            if int(c[s + hi]) > int(c[s + lo]):
                (jobs_B if w % 2 else jobs_A).append((r, s, head, tail, lo, hi))
    return jobs_A, jobs_B, L + (len(wins) - 1) * (L - end)


def job_table(jobs: Sequence[Job], device) -> torch.Tensor:
    """[J, 6] int64 on ``device``: the table aid_window_gather / aid_window_scatter read (include/aid_restore.h)"""
    return torch.tensor(list(jobs), dtype=torch.int64).reshape(-1, _lib.AID_RESTORE_JOB_FIELDS).to(device)


def _rows(t: torch.Tensor, what: str):
    _lib._req(t)
    if t.dim() != 2 or (t.stride(1) != 1 and t.shape[1] > 1):
        raise _lib.AidError(f"{what} must be [rows, N] with contiguous rows")


def _table(jobs: torch.Tensor):
    if not (jobs.is_cuda and jobs.dtype == torch.int64 and jobs.dim() == 2 and jobs.shape[1] == _lib.AID_RESTORE_JOB_FIELDS and jobs.is_contiguous()):
        raise _lib.AidError("the job table must be a contiguous [J, 6] int64 tensor on the GPU (restore.job_table)")


def window_gather(rec: torch.Tensor, out: torch.Tensor, mask: torch.Tensor, jobs: torch.Tensor, L: int):
    """One aid_window_gather launch on the current stream -> (y [J, L], m [J, L]): the observations and the mask of every job's window;
    the first ``head`` / last ``tail`` samples observed from ``out``, the rest from ``rec`` under ``mask`` ([R, N] or [1, N], float32)."""
    for t, what in ((rec, "rec"), (out, "out"), (mask, "mask")):
        _rows(t, what)
    _table(jobs)
    R, N = rec.shape
    if out.shape != rec.shape or mask.shape[1] != N or mask.shape[0] not in (1, R):
        raise _lib.AidError(f"window_gather: rec {tuple(rec.shape)}, out {tuple(out.shape)} and mask {tuple(mask.shape)} do not match")
    J = jobs.shape[0]
    y = torch.empty((J, L), dtype=torch.float32, device=rec.device)
    m = torch.empty((J, L), dtype=torch.float32, device=rec.device)
    if J:
        _lib.call("aid_window_gather", _lib.WindowGatherParams(rec.data_ptr(), out.data_ptr(), mask.data_ptr(), y.data_ptr(), m.data_ptr(), jobs.data_ptr(),
                                                                J, R, int(L), N, rec.stride(0), out.stride(0), mask.stride(0) if mask.shape[0] > 1 else 0))
    return y, m


def window_scatter(x: torch.Tensor, out: torch.Tensor, jobs: torch.Tensor):
    """One aid_window_scatter launch on the current stream: out[r_j, s_j + i] = x[j, i] over every job's owned range, below N."""
    _rows(out, "out")
    _lib._req(x)
    _table(jobs)
    J = jobs.shape[0]
    if x.dim() != 2 or x.shape[0] != J or not x.is_contiguous():
        raise _lib.AidError(f"window_scatter: x must be contiguous [J = {J}, L], got {tuple(x.shape)}")
    if J:
        _lib.call("aid_window_scatter", _lib.WindowScatterParams(x.data_ptr(), out.data_ptr(), jobs.data_ptr(), J, out.shape[0], x.shape[1], out.shape[1], out.stride(0)))


def check_rows(y, what: str, nonempty: bool = False) -> None:
    """The first refusal of a whole-recording mode: y is float32 [R, N] with contiguous rows, on any device (``what`` names it in the text)."""
    if not (torch.is_tensor(y) and y.dtype == torch.float32 and y.dim() == 2 and (y.shape[1] <= 1 or y.stride(1) == 1)
            and not (nonempty and 0 in y.shape)):
        raise _lib.AidError(f"y must be float32 {what} with contiguous rows, got {tuple(y.shape) if torch.is_tensor(y) else type(y).__name__}")


def check_batch(y: torch.Tensor, max_batch, seeds, task: str) -> None:
    """The last refusals of a whole-recording mode, after the mode's own: max_batch, one seed per recording -- under an active process group
    (dist._active()) ``seeds`` = None is refused too: run_passes shares the windows out over the ranks, and only seeded jobs give a result
    that does not depend on the world size -- and, judged last so that a host tensor with any other fault is refused for that fault, the
    device of y.  All before anything is launched."""
    if isinstance(max_batch, bool) or not isinstance(max_batch, int) or max_batch < 1:
        raise _lib.AidError(f"max_batch must be an integer >= 1, got {max_batch!r}")
    if seeds is not None and len(seeds) != y.shape[0]:
        raise _lib.AidError(f"{len(seeds)} seeds for {y.shape[0]} recordings")
    if seeds is None and _dist._active():
        raise _lib.AidError(f"{task} under a process group needs seeds, one per recording: without them every rank would draw from its own global "
                            "generator and the result would depend on the world size")
    if not y.is_cuda:
        raise _lib.AidError(f"{task} runs on the GPU only (no CPU fallback): y must be a float32 tensor on the GPU")


class WindowOperator(degrade._Operator):
    """What the observation operators of a window share (ClipObserved, FIRObserved, FIRClipObserved, RateObserved, STFTMagObserved, SpectralMaskObserved): the
    operator protocol of degrade.py over a per-sample ``state`` [1|B, row] (float32 on the GPU; aid_rows.h describes the codes).  They hold
    per-item rows, so ``shared_mask`` is False; ``rows(lo, hi)`` is the operator of items lo:hi, kept per range so that the apply / adjoint
    pair of a sub-batch meets the same object, which is what lets network.denoise_guided run sub-batches on concurrent streams.  A subclass
    calls ``__init__`` with its state, says in ``_slice`` how the operator of a slice is built and, where it holds more per item than the
    state, in ``items_held`` how many items it serves.  What an operator keeps between calls is kept per stream: the x_hat of the last apply
    (``_keep`` / ``_kept``) and scratch per (B, stream) (``_scratch``)."""
    shared_mask = False

    def __init__(self, state: torch.Tensor, row: str):
        if not (torch.is_tensor(state) and state.is_cuda and state.dtype == torch.float32 and state.dim() == 2 and (state.stride(1) == 1 or state.shape[1] == 1)):
            raise _lib.AidError(f"{type(self).__name__}: state must be a float32 GPU tensor {row} with contiguous rows (no CPU fallback)")
        self.state = state
        self._sub, self._x, self._frames = {}, {}, {}

    @property
    def items_held(self) -> Optional[int]:
        """the number of items the operator serves; None: any number, through one shared state row"""
        return None if self.state.shape[0] == 1 else self.state.shape[0]

    @property
    def _state_ld(self) -> int:
        return self.state.stride(0) if self.state.shape[0] > 1 else 0

    def _state_rows(self, lo: int, hi: int) -> torch.Tensor:
        return self.state if self.state.shape[0] == 1 else self.state[lo:hi]

    def rows(self, lo: int, hi: int):
        """The operator restricted to items lo:hi (views, no copy; tables and a shared state row stay shared), kept per range."""
        lo, hi, held = int(lo), int(hi), self.items_held
        if not (0 <= lo < hi and (held is None or hi <= held)):
            raise _lib.AidError(f"{type(self).__name__}.rows: [{lo}, {hi}) is no range of {'its' if held is None else held} items")
        op = self._sub.get((lo, hi))
        if op is None:
            op = self._sub[(lo, hi)] = self._slice(lo, hi)
        return op

    def _signal(self, x, n: int, what: str = ""):
        """x as contiguous [B, n], refused unless it is float32 on the GPU with as many items as the operator holds"""
        x = x.reshape(x.shape[0], -1)
        held = self.items_held
        if not (x.is_cuda and x.dtype == torch.float32 and x.shape[1] == n and x.shape[0] >= 1 and held in (None, x.shape[0])):
            raise _lib.AidError(f"{type(self).__name__}{what}: expected a float32 GPU tensor [{'B' if held is None else held}, {n}], got {tuple(x.shape)}")
        return x.contiguous()

    def _observation(self, x, y, n: int):
        """the y of project(x, y) as contiguous [B, n]"""
        y = y.reshape(y.shape[0], -1)
        if not (y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == (x.shape[0], n)):
            raise _lib.AidError(f"{type(self).__name__}.project: the observation must be a float32 GPU tensor [{x.shape[0]}, {n}], got {tuple(y.shape)}")
        return y.contiguous()

    def _keep(self, x):
        self._x[torch.cuda.current_stream().cuda_stream] = x

    def _kept(self, g):
        """the x_hat of the last apply on this stream, for the adjoint of ``g``"""
        x = self._x.get(torch.cuda.current_stream().cuda_stream)
        if x is None or x.shape[0] != g.shape[0]:
            raise _lib.AidError(f"{type(self).__name__}.adjoint needs the matching apply on this stream first")
        return x

    def _scratch(self, B: int, *shape, device):
        key = (B, torch.cuda.current_stream().cuda_stream)          # (sub-batches on concurrent streams must not share scratch)
        fr = self._frames.get(key)
        if fr is None:
            fr = self._frames[key] = torch.empty(B, *shape, device=device, dtype=torch.float32)
        return fr


def no_jobs(*passes) -> bool:
    """True when no pass has a job and no process group is active: the recordings are returned as they are.  Under a group run_passes is
    entered even without a job, for its guard: a rank that alone found no job must not leave the others waiting."""
    return not any(passes) and not _dist._active()


class Group(NamedTuple):
    """One set of equal-length recordings of a pooled run (run_pooled_passes): what a ``*_passes`` function hands to run_passes, and where
    its recordings stand in the caller's list of seeds."""
    out: torch.Tensor                                # [R_g, N_g], restored in place
    passes: Sequence[Sequence[Job]]                  # (jobs_A, jobs_B); the r of a job is a row of ``out``
    gather: Callable                                 # gather(table [J, 6]) -> the rows of the table's jobs, a tensor [J, ...] or a tuple of such
    files: Optional[Sequence[int]] = None            # files[r]: the index of row r in ``seeds``; None: r itself


def _job_seeds(seeds, jobs: Sequence[Job], step: int, files: Optional[Sequence[int]] = None):
    """the seed rule: the job of window w = s // step of recording r runs with seeds[r] * SEED_STRIDE + w (None without seeds); with
    ``files`` recording r is seeds[files[r]]"""
    if seeds is None:
        return None
    return [int(seeds[r if files is None else files[r]]) * SEED_STRIDE + s // step for r, s, *_ in jobs]


def pass_digest(out: torch.Tensor, passes: Sequence[Sequence[Job]], step: int, seeds, L) -> dict:
    """What every rank of a process group must agree on before a sharded run_passes: the number of passes, the job count and a hash of the
    job tuples per pass (tuples of ints hash identically in every process), the shape of ``out``, step, L, the seeds, and one float64
    checksum of ``out`` -- a single reduction, read once (as hex text, so that a NaN compares equal to itself)."""
    return {"passes": len(passes), "jobs": tuple(len(jobs) for jobs in passes),
            "plan": tuple(hash(tuple(tuple(int(v) for v in job) for job in jobs)) for jobs in passes),
            "shape": tuple(out.shape), "step": int(step), "L": int(L), "seeds": None if seeds is None else tuple(int(s) for s in seeds),
            "recordings": float(out.sum(dtype=torch.float64)).hex()}


def guard_ranks(digest: dict) -> None:
    """One all_gather_object of ``digest``; unless all are equal, EVERY rank raises AidError naming the ranks that differ from rank 0 and the
    fields they differ in -- a rank that was handed other files fails here, not in an all-gather of mismatched size."""
    every = [None] * torch.distributed.get_world_size()
    torch.distributed.all_gather_object(every, digest)
    bad = [(r, sorted(k for k in every[0] if d.get(k) != every[0][k])) for r, d in enumerate(every) if d != every[0]]
    if bad:
        raise _lib.AidError("run_passes: the ranks of the process group were not given the same work: "
                            + ", ".join(f"rank {r} differs from rank 0 in {', '.join(ks)}" for r, ks in bad)
                            + " (every rank passes the same recordings, arguments and seeds)")


def pooled_digest(groups: Sequence[Group], step: int, seeds, L) -> dict:
    """pass_digest over all groups of a pooled run: its per-group fields as tuples over the groups (so a rank that was handed one other file
    length differs in "shape"), the files of every group, and step, L and the seeds once."""
    per = [pass_digest(g.out, g.passes, step, None, L) for g in groups]
    d = {k: tuple(p[k] for p in per) for k in ("passes", "jobs", "plan", "shape", "recordings")}
    d.update(files=tuple(None if g.files is None else tuple(int(i) for i in g.files) for g in groups),
             step=int(step), L=int(L), seeds=None if seeds is None else tuple(int(s) for s in seeds))
    return d


def _cat_rows(wins: list):
    """the gathered rows of several groups laid row-wise into one ``win`` (copies, bit-exact); one group's rows are used as they are"""
    if len(wins) == 1:
        return wins[0]
    if isinstance(wins[0], (tuple, list)):
        return tuple(torch.cat(ts) for ts in zip(*wins))
    return torch.cat(wins)


def _owned(bounds: Sequence[int], a: int, b: int):
    """(group g, a_g, b_g) for every group with pooled jobs in [a, b): its jobs a_g:b_g, relative to the group's own job list"""
    for g in range(len(bounds) - 1):
        lo, hi = max(a, bounds[g]), min(b, bounds[g + 1])
        if hi > lo:
            yield g, lo - bounds[g], hi - bounds[g]


def run_pooled_passes(sampler, groups: Sequence[Group], step: int, max_batch: int, seeds, predict, L: Optional[int] = None) -> None:
    """The pass loop of every whole-recording restoration, over recordings of any lengths: ``groups`` holds one Group per length, and the jobs
    of all groups share the sampler calls.  Per pass p the jobs of all groups, in group order and within a group ordered by recording and
    window, are ONE list of J jobs.  Every group with jobs runs its own gather on its own table (one launch per group and pass), the gathered
    rows are laid row-wise into one ``win`` (a window's row has the same length for every recording: it depends on L and the operator, not
    on N), and per chunk [c0, c1) of at most ``max_batch`` pooled jobs -- a chunk may span recordings and groups -- ``x = predict(win, c0, c1)``
    -> [c1 - c0, L] is scattered with one aid_window_scatter launch per group the chunk touches, into that group's ``out``.  A pass starts only
    after every group's earlier pass has been scattered: same stream, in order.  Groups and passes without a job cost nothing.
    ``sampler.seeds`` is set per chunk by the seed rule, seeds[group.files[r]] * SEED_STRIDE + w (None without seeds), and put back at the
    end: a job's result depends on its seed alone, so the pooled result equals what the groups give one by one.

    Under an active process group (dist._active()) of ``world`` ranks every rank calls with the same groups and seeds, and with the same
    weights (call dist.broadcast_parameters first).  Before anything is launched one all_gather_object compares pooled_digest of every rank
    and all ranks raise if one differs (guard_ranks).  Then per pass of J pooled jobs: rank k takes [lo, hi) = dist.shard_range(J, k, world),
    gathers only the rows of its share, group by group, and calls ``predict`` per chunk of at most ``max_batch`` jobs of its share (max_batch
    is per rank); ONE dist.gather_outputs per pass returns [J, L] in job order on every rank (a rank without a job contributes [0, L]: ``L``
    is required here), and every rank scatters the whole pass group by group, in launches of at most 65535 jobs.  No collective inside
    ``predict``, the sampler or the network."""
    groups = list(groups)
    if not groups:
        return
    n_pass = len(groups[0].passes)
    if any(len(g.passes) != n_pass for g in groups):
        raise _lib.AidError(f"run_pooled_passes: every group must hold the same number of passes, got {[len(g.passes) for g in groups]}")
    sharded = _dist._active()
    if sharded:
        if L is None:
            raise _lib.AidError("run_passes under a process group needs L, the length of a window: a rank without a job in a pass contributes [0, L]")
        rank, world = torch.distributed.get_rank(), torch.distributed.get_world_size()
        guard_ranks(pooled_digest(groups, step, seeds, L))
    tables = [[job_table(g.passes[p], g.out.device) if g.passes[p] else None for g in groups] for p in range(n_pass)]
    keep = getattr(sampler, "seeds", None)
    try:
        for p in range(n_pass):
            bounds = [0]
            for g in groups:
                bounds.append(bounds[-1] + len(g.passes[p]))
            J = bounds[-1]
            if not J:
                continue
            lo, hi = _dist.shard_range(J, rank, world) if sharded else (0, J)
            parts = []
            if hi > lo:
                # (the closures index win relative to the tables they were given: the pooled job j is row j - lo)
                win = _cat_rows([groups[g].gather(tables[p][g][a:b]) for g, a, b in _owned(bounds, lo, hi)])
                for c0 in range(lo, hi, max_batch):
                    c1 = min(hi, c0 + max_batch)
                    owned = list(_owned(bounds, c0, c1))
                    sampler.seeds = None if seeds is None else [s for g, a, b in owned for s in _job_seeds(seeds, groups[g].passes[p][a:b], step, groups[g].files)]
                    x = predict(win, c0 - lo, c1 - lo)
                    if sharded:
                        parts.append(x)
                        continue
                    x = x.contiguous()
                    for g, a, b in owned:
                        window_scatter(x[bounds[g] + a - c0:bounds[g] + b - c0], groups[g].out, tables[p][g][a:b])
            if sharded:
                out = groups[0].out
                local = parts[0] if len(parts) == 1 else torch.cat(parts) if parts else torch.zeros((0, int(L)), dtype=out.dtype, device=out.device)
                allx = _dist.gather_outputs(local, J).contiguous()          # [J, L] in job order, the same on every rank
                for g, a, b in _owned(bounds, 0, J):
                    for j0 in range(a, b, SCATTER_JOBS):
                        j1 = min(b, j0 + SCATTER_JOBS)
                        window_scatter(allx[bounds[g] + j0:bounds[g] + j1], groups[g].out, tables[p][g][j0:j1])
    finally:
        sampler.seeds = keep


def run_passes(sampler, out: torch.Tensor, passes: Sequence[Sequence[Job]], step: int, max_batch: int, seeds, gather, predict, L: Optional[int] = None) -> None:
    """The pass loop of one set of equal-length recordings: run_pooled_passes over the one group (out, passes, gather).  Per non-empty job
    list of ``passes``: ``win = gather(table)`` (one launch for the whole pass), then per chunk [c0, c1) of at most ``max_batch`` jobs
    ``x = predict(win, c0, c1)`` -> [c1 - c0, L] and one aid_window_scatter launch of x into ``out``.  A later pass gathers what an earlier
    one scattered: same stream, in order.  ``sampler.seeds`` is set per chunk by the seed rule (None without seeds) and put back at the end.

    Under an active process group (dist._active()) of ``world`` ranks a pass is shared out; every rank calls with the same recordings, plan
    and seeds, and with the same weights (call dist.broadcast_parameters first).  Before anything is launched one all_gather_object
    compares the digest of every rank and all ranks raise if one differs (guard_ranks).  Then per pass of J jobs: rank k takes
    [lo, hi) = dist.shard_range(J, k, world), gathers ``win = gather(table[lo:hi])`` (nothing when its share is empty) and calls
    ``predict(win, c0 - lo, c1 - lo)`` per chunk of at most ``max_batch`` jobs of its share (max_batch is per rank), under the unchanged seed
    rule, so a job's result does not depend on the rank or chunk it ran in; ONE dist.gather_outputs per pass returns [J, L] in job order on
    every rank (a rank without a job contributes [0, L]: ``L`` is required here), and the whole pass is scattered, in launches of at most
    65535 jobs.  After a pass ``out`` is identical on every rank, and the next pass gathers from it as before.  No collective inside
    ``predict``, the sampler or the network."""
    run_pooled_passes(sampler, [Group(out, passes, gather)], step, max_batch, seeds, predict, L)


class LongTask(NamedTuple):
    """One whole-recording mode, as everything that drives it sees it: Sampler.predict_*_long and Sampler.predict_long_pooled (through
    Sampler._long), the module's ``*_passes`` function (through ``run_task``) and harness.py.  Each mode module declares its record with
    ``long_task`` next to the functions the record names; nothing else knows a mode."""
    name: str                                        # the task of predict_long_pooled, e.g. "bwe_iir"
    method: str                                      # the Sampler method, named in the refusals, e.g. "predict_bwe_iir_long"
    what: str                                        # "restored" / "declipped": what the rid refusal says the method returns
    consistency: Optional[str]                       # why tester.data_consistency in use is refused; None: it is served
    guided: Optional[str]                            # the tail of the refusal of xi <= 0; None: xi = 0 is served
    entries: Tuple[str, ...]                         # the names of a group's entries after y, in the order of the method's parameters
    call_args: Dict[str, object]                     # the arguments all groups of a call share: name -> default, REQUIRED where there is none
    prepare: Callable                                # prepare(sampler_args, **call_args) -> state: what the groups share, judged before any group
    check: Callable                                  # check(y, *entries, state, L, end, max_batch, seeds) -> checked: the refusals, all before any launch
    build: Callable                                  # build(y, checked, state, L, end) -> Group, from what ``check`` returned; it validates nothing
    predict: Callable                                # predict(sampler, state, L, device) -> predict(win, c0, c1), one for all groups
    step: Callable                                   # step(state, L, end) -> the distance between window starts


REQUIRED = object()                                  # the default of a call argument that has none
LONG_TASKS: Dict[str, LongTask] = {}


def long_task(**fields) -> None:
    """Declare a mode: its record, entered in LONG_TASKS under its name."""
    LONG_TASKS[fields["name"]] = LongTask(**fields)


def plain_step(state, L: int, end: int) -> int:
    """``step`` of a mode whose grid needs no alignment"""
    return L - end


def run_task(task: LongTask, sampler, state, groups, L: int, end: int, max_batch: int = 8, seeds=None, ready: Optional[Callable] = None) -> List[torch.Tensor]:
    """The one driver of the whole-recording modes, for one length and for many: ``groups`` holds per set of equal-length recordings
    (y, *task.entries) -- a bare tensor is (y,), a missing entry None -- and ``state`` is task.prepare's.  In this order: ``task.check`` of
    every group, the seed count over all groups, the one-device refusal, ``ready()`` (Sampler._check_model), and only then ``task.build`` of
    every group from what its check returned, and run_pooled_passes -> one [R_g, N_g] per group.  ``seeds``: one per recording over all
    groups in order; a single group is handed the list as it is, so that a list of the wrong length is refused where the plain methods
    refuse it.  Without a job and without a process group nothing is launched and the copies come back (``no_jobs``)."""
    width = 1 + len(task.entries)
    groups = [((tuple(g) if isinstance(g, (tuple, list)) else (g,)) + (None,) * width)[:width] for g in groups]
    device = next((g[0].device for g in groups if torch.is_tensor(g[0])), None)
    bounds = [0]
    for g in groups:
        bounds.append(bounds[-1] + (g[0].shape[0] if torch.is_tensor(g[0]) and g[0].dim() >= 1 else 0))
    share = len(groups) > 1 and seeds is not None
    checked = [task.check(*g, state, L, end, max_batch, seeds[bounds[i]:bounds[i + 1]] if share else seeds) for i, g in enumerate(groups)]
    if seeds is not None and len(seeds) != bounds[-1]:
        raise _lib.AidError(f"{len(seeds)} seeds for {bounds[-1]} recordings")
    if any(torch.is_tensor(g[0]) and g[0].device != device for g in groups):
        raise _lib.AidError("predict_long_pooled: the recordings of all groups must be on one device")
    if ready is not None:
        ready()
    built = [task.build(g[0], c, state, L, end)._replace(files=range(bounds[i], bounds[i + 1])) for i, (g, c) in enumerate(zip(groups, checked))]
    if not no_jobs(*(jobs for b in built for jobs in b.passes)):
        run_pooled_passes(sampler, built, task.step(state, L, end), max_batch, seeds, task.predict(sampler, state, L, device), L=L)
    return [b.out for b in built]


def check_restore_args(y: torch.Tensor, mask: torch.Tensor, state, L: int, end: int, max_batch: int, seeds) -> torch.Tensor:
    """The refusals of a restoration, all raised before anything is launched -> the mask as [1|R, N].  What can be judged without a GPU is
    judged first; the device of y last."""
    check_rows(y, "recordings [R, N]")
    if mask.dim() == 1:
        mask = mask.reshape(1, -1)
    if mask.dim() != 2 or mask.shape[1] != y.shape[1] or mask.shape[0] not in (1, y.shape[0]):
        raise _lib.AidError(f"mask {tuple(mask.shape)} does not match recordings {tuple(y.shape)} (y [R, N], mask [1, N] or [R, N])")
    restore_windows(y.shape[1], L, end)                               # (end in [1, L/2))
    check_batch(y, max_batch, seeds, "restoration of whole recordings")
    return mask


def restore_group(y: torch.Tensor, mask: torch.Tensor, state, L: int, end: int) -> Group:
    """The part of a restoration that plans and builds: y [R, N] recordings on the GPU (rows contiguous, any row stride), the mask
    [1|R, N] of check_restore_args -> Group(out = a copy of y, (jobs_A, jobs_B) of restore_plan, the aid_window_gather closure).  The plan
    is made on the host from the mask; the mask goes to the GPU only when there is a job."""
    jobs_A, jobs_B, _ = restore_plan(mask, L, end, y.shape[0])
    out = y.clone(memory_format=torch.contiguous_format)
    dmask = mask.to(y.device, torch.float32).contiguous() if jobs_A or jobs_B else None
    return Group(out, (jobs_A, jobs_B), lambda table: window_gather(y, out, dmask, table, L))    # (pass B reads what pass A scattered)


def restore_predict(sampler, state, L: int, device):
    """predict(win, c0, c1) of a restoration: ``sampler.predict_inpainting`` over rows c0:c1 of the gathered (y, m)"""
    return lambda win, c0, c1: sampler.predict_inpainting(win[0][c0:c1], win[1][c0:c1])


long_task(name="inpainting", method="predict_inpainting_long", what="restored", consistency=None, guided=None, entries=("mask",), call_args={},
          prepare=lambda args: None, check=check_restore_args, build=restore_group, predict=restore_predict, step=plain_step)


def restore_passes(sampler, y: torch.Tensor, mask: torch.Tensor, L: int, end: int, max_batch: int = 8, seeds: Optional[Sequence[int]] = None) -> torch.Tensor:
    """The two passes over ``sampler.predict_inpainting(yw [B, L], mw [B, L]) -> [B, L]`` with B <= max_batch: y [R, N] recordings on the GPU
    (rows contiguous, any row stride), mask [1|R, N] -> restored [R, N].  Per pass: one gather launch, the sampler calls, one scatter launch per
    call.  Recordings, mask and result stay on the GPU; the plan is made on the host from the mask before pass A.  ``seeds`` [R]: the job of
    window w of recording r runs with ``sampler.seeds = [seeds[r] * 65536 + w, ...]`` (None: sampler.seeds = None, the global generator)."""
    return run_task(LONG_TASKS["inpainting"], sampler, None, [(y, mask)], L, end, max_batch, seeds)[0]
