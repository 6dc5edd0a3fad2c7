"""Blind bandwidth extension of whole recordings: ONE fitted low-pass per recording (aid_window_energy in include/aid_bwe_long.h, aid_lowpass_fit_groups in include/aid_phase.h; blind.py holds the model, the
statistics, the cost and the tap design; bwe_long.py the window scheme of a recording seen through a FIR filter).

y [R, N] went, recording by recording, through an unknown zero-phase low-pass as a whole.  Two stages, both through
``sampler.predict_resample``:

STAGE 1 estimates one filter per recording.  The candidates are the windows of ``bwe_long.bwe_windows`` that lie wholly inside the recording
(window 0 when N < L); ``window_energy`` (one aid_window_energy launch, read back once) gives E[r, w], the sum of the squares of the
window's samples, and ``choose_probes`` takes the P_r = min(probes, candidates) windows of largest E of every recording, ties to the lower
window, ordered by start.  The probes run in chunks of whole recordings (``probe_chunks``: filled greedily in recording order while the
probe count stays within max_batch), each chunk one predict_resample through ``PooledBlindLowpass``: in every guided evaluation the band
statistics of all probes of a recording are added (aid_lowpass_fit_groups, in fp64, in item order) and ONE low-pass is fitted to the sum,
so a quiet or narrow-band window does not decide the filter -- it adds little to the sums.  Nothing is carried from one evaluation to the
next, and the restorations of the probes are discarded: what stage 1 returns is, per recording, the taps [K] and the fit [4] of the last
evaluation.  A probe is a window cut out of the recording, so within reach of a border its samples are no observations of the window
(bwe_long.py): the states of aid_bwe_gather with head = tail = 0 mark them, and the operator filters through aid_fir_observed_items with
those state rows.  |Y| of the statistics is taken from the recording's own samples over the whole window, border samples included: they
are true filtered values.

STAGE 2 is bwe_long's plan, gather, passes, scatter, seeds and rank sharing (restore.run_passes), with one tap row per job beside the
gathered (y, k) and ``FIRObservedRows`` -- FIRObserved with taps [B, K] -- as the window operator.

Seeds: window w of recording r runs with seeds[r] * SEED_STRIDE + w (restore.py), probe p with seeds[r] * SEED_STRIDE + SEED_STRIDE - 1 - p.
Under an active process group the ranks first compare what they were given (restore.guard_ranks), then rank k estimates the recordings
dist.shard_range(R, k, world) and one dist.gather_outputs of [R_k, K + 4] (taps and fit side by side) gives every rank all rows.

``window_energy_host`` / ``choose_probes`` / ``probe_chunks`` / ``pooled_stats_host`` restate the host-checkable parts in float64 numpy /
plain Python: they are the definition the kernels and the stage are tested against.  GPU only for the operators; no fallback.

Not covered: pooling recordings of different lengths into shared passes (there is no ``pool`` argument), reusing the stage-1 restorations,
sub-batch streams in stage 1 (a group may straddle the network's split, so PooledBlindLowpass has no ``rows`` and runs on one stream), more
than one knee, IIR or decimating models.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import blind
from . import bwe_long
from . import degrade
from . import dist as _dist
from . import restore

NO_PROJECTION = "a projection onto the consistent set of an estimated filter is not a projection onto the data"


# ---- the host restatements ---------------------------------------------------------------------------------------------------------------
def candidate_starts(N: int, L: int, end: int, K: int) -> List[int]:
    """the starts of the windows of bwe_long.bwe_windows(N, L, end, K) that lie wholly inside the recording (s + L <= N): a prefix of the
    grid, w * (L - end); [0] when there is none (N < L).  Raises what bwe_windows raises (end in [1, L/2); end >= 2 (K - 1) with more than
    one window)."""
    starts = [s for s, *_ in bwe_long.bwe_windows(N, L, end, K) if s + int(L) <= int(N)]
    return starts or [0]


def window_energy_host(y, starts: Sequence[int], L: int) -> np.ndarray:
    """E [R, W] float64: E[r, w] = sum_i y[r, starts[w] + i]^2 over the samples i < L of the window that exist"""
    y = np.asarray(y, dtype=np.float64)
    y = y.reshape(1, -1) if y.ndim == 1 else y
    return np.stack([(y[:, s:s + int(L)] ** 2).sum(axis=1) for s in starts], axis=1)


def check_probes(probes, max_batch) -> None:
    if isinstance(max_batch, bool) or not isinstance(max_batch, int) or max_batch < 1:
        raise _lib.AidError(f"max_batch must be an integer >= 1, got {max_batch!r}")
    if isinstance(probes, bool) or not isinstance(probes, int) or probes < 1:
        raise _lib.AidError(f"blind bandwidth extension of whole recordings: probes must be an integer >= 1, got {probes!r}")
    if probes > max_batch:
        raise _lib.AidError(f"blind bandwidth extension of whole recordings: probes = {probes} windows of one recording do not fit a chunk of "
                            f"max_batch = {max_batch} (a chunk holds whole recordings)")


def choose_probes(E, probes: int, max_batch: int) -> List[List[int]]:
    """E [R, C] (the energy of every candidate window) -> per recording the indices of its P_r = min(probes, C) windows of largest E, ties to
    the lower window, in ascending order.  Refuses probes < 1, probes > max_batch, and a recording whose largest E is not above 0 (there is
    nothing to fit a filter to), naming it.  Pure: no GPU."""
    check_probes(probes, max_batch)
    E = np.asarray(E, dtype=np.float64)
    if E.ndim != 2 or E.shape[1] < 1:
        raise _lib.AidError(f"choose_probes: E must be [R, candidates >= 1], got {E.shape}")
    chosen = []
    for r, row in enumerate(E):
        if not row.max() > 0:
            raise _lib.AidError(f"blind bandwidth extension of whole recordings: recording {r} is all zero in every candidate window (largest window "
                                f"energy {row.max()!r}): there is nothing to fit a filter to")
        order = sorted(range(row.size), key=lambda w: (-row[w], w))
        chosen.append(sorted(order[:min(int(probes), row.size)]))
    return chosen


def probe_chunks(counts: Sequence[int], max_batch: int, lo: int = 0, hi: Optional[int] = None) -> List[Tuple[int, int]]:
    """[(r0, r1), ...]: the recordings lo:hi in chunks of whole recordings, each filled greedily in recording order while the probes of its
    recordings number at most max_batch (counts[r] <= max_batch each)"""
    hi = len(counts) if hi is None else hi
    chunks, r0, n = [], lo, 0
    for r in range(lo, hi):
        if counts[r] > max_batch:
            raise _lib.AidError(f"probe_chunks: recording {r} has {counts[r]} probes, max_batch is {max_batch}")
        if n + counts[r] > max_batch:
            chunks.append((r0, r))
            r0, n = r, 0
        n += counts[r]
    if hi > r0:
        chunks.append((r0, hi))
    return chunks


def probe_seed(seed: int, p: int) -> int:
    """the seed of probe p of a recording whose seed is ``seed``: from the top of the recording's block of SEED_STRIDE seeds downwards"""
    return int(seed) * restore.SEED_STRIDE + restore.SEED_STRIDE - 1 - int(p)


def check_probe_seeds(n_windows: int, probes: int) -> None:
    """refuse when the probe seeds seeds[r] * SEED_STRIDE + SEED_STRIDE - 1 - p, p < probes, would meet the window seeds
    seeds[r] * SEED_STRIDE + w, w < n_windows"""
    if int(n_windows) + int(probes) > restore.SEED_STRIDE:
        raise _lib.AidError(f"blind bandwidth extension of whole recordings: {n_windows} windows and {probes} probes per recording do not fit the "
                            f"{restore.SEED_STRIDE} seeds of a recording (the probe seeds would meet the window seeds)")


def pooled_stats_host(stats, groups: Sequence[int]) -> np.ndarray:
    """stats [B, 2, F], groups [B] -> [B, 2, F] float64: for every item the sum of the statistics of the items of its group, added in
    ascending item order in float64 -- what aid_lowpass_fit_groups fits to; ``blind.fit_host`` of it is the pooled fit"""
    stats = np.asarray(stats, dtype=np.float64)
    groups = [int(g) for g in groups]
    if stats.ndim != 3 or stats.shape[0] != len(groups):
        raise _lib.AidError(f"pooled_stats_host: stats {stats.shape} for {len(groups)} group ids")
    out = np.zeros_like(stats)
    for b, g in enumerate(groups):
        for o, go in enumerate(groups):
            if go == g:
                out[b] += stats[o]
    return out


# ---- the launches ------------------------------------------------------------------------------------------------------------------------
def window_energy(y: torch.Tensor, L: int, step: int, W: int) -> torch.Tensor:
    """One aid_window_energy launch on the current stream: y [R, N] (float32, GPU, contiguous rows) -> E [R, W] float64, the energy of the
    windows that start at w * step, over their samples below N (a window that starts at or beyond N has energy 0).  The windows go to the
    kernel as a job table of restore.py, one job per (recording, window)."""
    restore._rows(y, "y")
    R, N = y.shape
    if int(W) < 1 or int(step) < 1 or int(L) < 1:
        raise _lib.AidError(f"window_energy: W = {W}, step = {step} and L = {L} must be >= 1")
    table = restore.job_table([(r, w * int(step), 0, 0, 0, int(L)) for r in range(R) for w in range(int(W))], y.device)
    E = torch.empty((R, int(W)), dtype=torch.float64, device=y.device)
    _lib.call("aid_window_energy", _lib.BweGatherParams(y.data_ptr(), None, E.data_ptr(), None, table.data_ptr(), R * int(W), R, 1, int(L), N,
                                                        y.stride(0) if R > 1 else N, N))
    return E


def group_array(groups: Sequence[int]):
    """the group ids of a launch as the host int array the launcher reads"""
    groups = [int(g) for g in groups]
    if not 1 <= len(groups) <= _lib.AID_LOWPASS_FIT_MAX_ITEMS:
        raise _lib.AidError(f"lowpass_fit_groups: 1 to {_lib.AID_LOWPASS_FIT_MAX_ITEMS} items per launch, got {len(groups)}")
    return (C.c_int * len(groups))(*groups)


def lowpass_fit_groups(stats, groups, cfg: blind.Settings, fit=None, taps=None):
    """One aid_lowpass_fit_groups launch on the current stream: stats [B, 2, F], groups [B] ids in [0, B) (a sequence, or ``group_array`` of
    one) -> (fit [B, 4], taps [B, K]) of the statistics pooled per group; the rows of a group are bit-identical"""
    _lib._req(stats)
    B = stats.shape[0]
    if tuple(stats.shape) != (B, 2, cfg.F) or not stats.is_contiguous() or B < 1:
        raise _lib.AidError(f"lowpass_fit_groups: stats must be contiguous [B, 2, {cfg.F}], got {tuple(stats.shape)}")
    if not isinstance(groups, C.Array):
        groups = group_array(groups)
    if len(groups) != B:
        raise _lib.AidError(f"lowpass_fit_groups: {len(groups)} group ids for {B} items")
    _, _, cand, wtap = blind.tables(cfg, stats.device)
    fit = torch.empty((B, 4), dtype=torch.float32, device=stats.device) if fit is None else fit
    taps = torch.empty((B, cfg.K), dtype=torch.float32, device=stats.device) if taps is None else taps
    # (the ids are host memory, read by the launcher before it returns)
    _lib.call("aid_lowpass_fit_groups", _lib.MatrixNormParams(stats.data_ptr(), cand.data_ptr(), taps.data_ptr(), fit.data_ptr(), wtap.data_ptr(), C.addressof(groups),
                                                               B, cfg.F, cfg.cutoffs.size, cfg.slopes.size, cfg.K, cfg.eps))
    return fit, taps


# ---- the operators -----------------------------------------------------------------------------------------------------------------------
class FIRObservedRows(restore.WindowOperator):
    """bwe_long.FIRObserved with one tap row per item: taps [B, K], state [B, L] (0 filtered, 1 known, -1 unobserved, -2 absent), on
    aid_fir_observed_items, modes 0 (apply) and 1 (adjoint).  With equal rows it is FIRObserved bit for bit.  ``rows(lo, hi)`` slices taps
    and states (views), so the sub-batches of the network keep their concurrent streams.  There is no projection: the taps are an
    estimate."""

    def __init__(self, taps: torch.Tensor, state: torch.Tensor):
        super().__init__(state, "[B, L]")
        if not (torch.is_tensor(taps) and taps.is_cuda and taps.dtype == torch.float32 and taps.dim() == 2 and taps.shape[0] == state.shape[0]
                and taps.shape[1] >= 1 and taps.stride(1) == 1 and (taps.shape[0] == 1 or taps.stride(0) == taps.shape[1])):
            raise _lib.AidError(f"FIRObservedRows: taps must be a contiguous float32 GPU tensor [{state.shape[0]}, K], one row per row of the state")
        self.taps, self.K, self.L = taps, taps.shape[1], state.shape[1]

    @property
    def items_held(self) -> int:
        return self.taps.shape[0]

    def _slice(self, lo: int, hi: int) -> "FIRObservedRows":
        return FIRObservedRows(self.taps[lo:hi], self.state[lo:hi])

    def _run(self, mode, x):
        x = self._signal(x, self.L)
        out = torch.empty_like(x)
        L = self.L
        _lib.call("aid_fir_observed_items", _lib.FirObservedParams(x.data_ptr(), None, self.state.data_ptr(), self.taps.data_ptr(), out.data_ptr(),
                                                                    x.shape[0], self.K, mode, L, L, L, self.state.stride(0), L))
        return out

    def apply(self, x):
        return self._run(0, x)

    def adjoint(self, g):
        return self._run(1, g)

    def project(self, x, y):
        raise AttributeError(f"FIRObservedRows: no data-consistency step ({NO_PROJECTION}): set tester.data_consistency.use = False")


class PooledBlindLowpass(degrade._Operator):
    """The operator of a chunk of probe windows: A(x_hat)_b = taps_b * x_hat_b over the states of item b, the taps fitted in ``apply`` to the
    statistics POOLED over the items of b's group -- three launches: aid_stft_band_stats, aid_lowpass_fit_groups, aid_fir_observed_items --
    and no host round trip.  ``adjoint`` is one launch, the adjoint filter with the taps the last apply left (constants in the VJP).

    ``y_raw`` [B, L]: the recording's own samples over every window, 0 where the window reaches beyond the recording; |Y| of the statistics
    is taken from it once.  ``state`` [B, L]: aid_bwe_gather's rows with head = tail = 0 (-1 within reach of a border that is not the
    recording's, -2 beyond its end).  ``groups`` [B]: ids in [0, B); items with equal id share one fit.  An item with absent samples (N < L
    only) has its x_hat multiplied by the 0/1 row of the samples that exist before the statistics, and nowhere else (``absent``: None looks
    at the state once).  After an apply ``taps`` [B, K] and ``fit`` [B, 4] hold what it found, bit-identical within a group.

    A group may straddle the network's sub-batch split, so there is deliberately no ``rows``: network.denoise_guided runs an operator with
    per-item data and no ``rows`` on one stream.  No projection."""
    shared_mask = False

    def __init__(self, y_raw: torch.Tensor, state: torch.Tensor, groups: Sequence[int], cfg: Optional[blind.Settings] = None, absent: Optional[bool] = None):
        cfg = blind.make_settings() if cfg is None else cfg
        for t, what in ((y_raw, "y_raw"), (state, "state")):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[0] >= 1 and t.shape[1] >= 1):
                raise _lib.AidError(f"PooledBlindLowpass: {what} must be a float32 GPU tensor [B, L] (no CPU fallback)")
        if y_raw.shape != state.shape or len(groups) != y_raw.shape[0]:
            raise _lib.AidError(f"PooledBlindLowpass: y_raw {tuple(y_raw.shape)}, state {tuple(state.shape)} and {len(groups)} group ids do not match")
        B, L = y_raw.shape
        if any(not 0 <= int(g) < B for g in groups):
            raise _lib.AidError(f"PooledBlindLowpass: every group id must lie in [0, {B}), got {list(groups)}")
        dev = y_raw.device
        self.cfg, self.L, self.K = cfg, L, cfg.K
        self.state = state.contiguous()
        self.groups, self._garr = [int(g) for g in groups], group_array(groups)
        self.y_mag = blind.stft_mag(y_raw, cfg)
        absent = bool((self.state <= -2).any()) if absent is None else bool(absent)
        self.present = (self.state > -2).to(torch.float32) if absent else None
        self.taps = torch.zeros((B, cfg.K), dtype=torch.float32, device=dev)
        self.fit = torch.zeros((B, 4), dtype=torch.float32, device=dev)
        self.stats = torch.zeros((B, 2, cfg.F), dtype=torch.float32, device=dev)
        self._frames = torch.empty((B, 1 + L // cfg.hop, 2, cfg.F), dtype=torch.float32, device=dev)
        self.log = None

    def _signal(self, x, what=""):
        x = x.reshape(x.shape[0], -1)
        if not (x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (self.taps.shape[0], self.L)):
            raise _lib.AidError(f"PooledBlindLowpass{what}: expected a float32 GPU tensor [{self.taps.shape[0]}, {self.L}], got {tuple(x.shape)}")
        return x.contiguous()

    def project(self, x, y):
        raise AttributeError(f"PooledBlindLowpass: no data-consistency step ({NO_PROJECTION}): set tester.data_consistency.use = False")

    def _fir(self, mode, x):
        out = torch.empty_like(x)
        L = self.L
        _lib.call("aid_fir_observed_items", _lib.FirObservedParams(x.data_ptr(), None, self.state.data_ptr(), self.taps.data_ptr(), out.data_ptr(),
                                                                    x.shape[0], self.K, mode, L, L, L, L, L))
        return out

    def apply(self, x_hat):
        x_hat = self._signal(x_hat)
        seen = x_hat if self.present is None else x_hat * self.present
        blind.band_stats(seen, self.y_mag, self.cfg, out=self.stats, scratch=self._frames)
        lowpass_fit_groups(self.stats, self._garr, self.cfg, fit=self.fit, taps=self.taps)
        if self.log is not None:
            self.log.append((self.taps.clone(), self.fit.clone()))
        return self._fir(0, x_hat)

    def adjoint(self, g):
        return self._fir(1, self._signal(g, ".adjoint"))


# ---- stage 1 -----------------------------------------------------------------------------------------------------------------------------
def raw_windows(y: torch.Tensor, jobs: Sequence[Tuple[int, int]], L: int) -> torch.Tensor:
    """[J, L]: the recording's own samples y[r, s:s + L] of every job (r, s), 0 where the window reaches beyond the recording (copies)"""
    N = y.shape[1]
    out = torch.zeros((len(jobs), int(L)), dtype=torch.float32, device=y.device)
    for j, (r, s) in enumerate(jobs):
        n = min(int(L), N - s)
        out[j, :n] = y[r, s:s + n]
    return out


def estimate_filters(sampler, y: torch.Tensor, cfg: blind.Settings, L: int, end: int, probes: int, max_batch: int, seeds):
    """Stage 1 -> (taps [R, K], fit [R, 4], probe starts per recording), on y.device and the same on every rank of an active process group."""
    R, N = y.shape
    step, K = L - end, cfg.K
    starts = candidate_starts(N, L, end, K)
    sharded = _dist._active()
    if sharded:                                                              # (a rank that was handed other recordings fails here, not in the exchange)
        restore.guard_ranks(dict(restore.pass_digest(y, bwe_long.bwe_plan(R, N, L, end, K), step, seeds, L), probes=int(probes)))
    E = window_energy(y, L, step, len(starts)).cpu().numpy()                 # (read back once, before anything else is launched)
    chosen = choose_probes(E, probes, max_batch)
    lo, hi = _dist.shard_range(R, torch.distributed.get_rank(), torch.distributed.get_world_size()) if sharded else (0, R)
    rows = []
    keep = getattr(sampler, "seeds", None)
    try:
        for r0, r1 in probe_chunks([len(c) for c in chosen], max_batch, lo, hi):
            jobs, groups, first = [], [], []
            for r in range(r0, r1):
                first.append(len(jobs))
                for w in chosen[r]:
                    groups.append(first[-1])
                    jobs.append((r, starts[w]))
            table = restore.job_table([(r, s, 0, 0, 0, L) for r, s in jobs], y.device)
            yw, kw = bwe_long.bwe_gather(y, y, table, L, K)
            op = PooledBlindLowpass(raw_windows(y, jobs, L), kw, groups, cfg, absent=N < L)
            sampler.seeds = None if seeds is None else [probe_seed(seeds[r], p) for r in range(r0, r1) for p in range(len(chosen[r]))]
            sampler.predict_resample(yw, (len(jobs), L), op)                  # (the restorations of the probes are discarded)
            idx = torch.tensor(first, dtype=torch.int64, device=y.device)
            rows.append(torch.cat([op.taps.index_select(0, idx), op.fit.index_select(0, idx)], dim=1))
    finally:
        sampler.seeds = keep
    local = rows[0] if len(rows) == 1 else torch.cat(rows) if rows else torch.zeros((0, K + 4), dtype=torch.float32, device=y.device)
    both = _dist.gather_outputs(local, R)
    return both[:, :K].contiguous(), both[:, K:].contiguous(), [[starts[w] for w in c] for c in chosen]


# ---- the two stages ----------------------------------------------------------------------------------------------------------------------
def check_blind_long_args(y, cfg: blind.Settings, L: int, end: int, probes, max_batch, seeds, frozen_taps):
    """The refusals of a blind bandwidth extension of whole recordings, all raised before anything is launched -> the frozen taps as float32
    [R, K] (None without).  What can be judged without a GPU is judged first; the device of y last."""
    restore.check_rows(y, "recordings [R, N]", nonempty=True)
    check_probes(probes, max_batch)
    if frozen_taps is not None:
        frozen_taps = blind.frozen_rows(frozen_taps, y.shape[0], cfg.K)
    wins = bwe_long.bwe_windows(y.shape[1], L, end, cfg.K)                   # (end in [1, L/2); end >= 2 (K - 1) with more than one window)
    check_probe_seeds(len(wins), probes)
    restore.check_batch(y, max_batch, seeds, "blind bandwidth extension of whole recordings")
    return frozen_taps


def blind_bwe_long_passes(sampler, y: torch.Tensor, cfg: blind.Settings, L: int, end: int, probes: int = 4, max_batch: int = 8,
                          seeds: Optional[Sequence[int]] = None, frozen_taps=None):
    """y [R, N] on the GPU -> (restored [R, N], taps [R, K], fit [R, 4], probe starts per recording).  Stage 1 (``estimate_filters``) is
    skipped entirely with ``frozen_taps`` ([K] or [R, K]): no energy launch, no sampler call, fit all zero and no probes.  Stage 2: the two
    passes of bwe_long over ``sampler.predict_resample(yw [B, L], (B, L), FIRObservedRows(taps of the jobs' recordings, kw))``."""
    frozen_taps = check_blind_long_args(y, cfg, L, end, probes, max_batch, seeds, frozen_taps)
    R, N = y.shape
    K = cfg.K
    if frozen_taps is None:
        taps, fit, starts = estimate_filters(sampler, y, cfg, L, end, probes, max_batch, seeds)
    else:
        taps, fit, starts = frozen_taps.to(y.device).contiguous(), torch.zeros((R, 4), dtype=torch.float32, device=y.device), [[] for _ in range(R)]
    out = y.clone(memory_format=torch.contiguous_format)

    def gather(table):
        return bwe_long.bwe_gather(y, out, table, L, K) + (taps.index_select(0, table[:, 0]),)     # (one tap row per job, once per pass)

    def predict(win, c0, c1):
        yw, kw, tw = (t[c0:c1] for t in win)
        return sampler.predict_resample(yw, (c1 - c0, L), FIRObservedRows(tw, kw))
    restore.run_passes(sampler, out, bwe_long.bwe_plan(R, N, L, end, K), L - end, max_batch, seeds, gather, predict, L=L)
    return out, taps, fit, starts
