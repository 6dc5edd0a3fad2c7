"""Bandwidth extension of whole recordings that exist only at a low sample rate, longer than one model segment -- in two batched sampler
passes (include/aid_lowrate_long.h).

The high-rate signal x [N] was resampled as a whole with torchaudio's default resampler at the ratio orig:new ("resample", degrade.SincResample)
or decimated by an integer f ("decimate": x[0:-1:f], the same kernels with orig = f, new = 1, width = 0 and the one-row table [1, 0, ..., 0]):
rec [M].  Low-rate sample i*new + j reads the K = 2*width + orig samples from i*orig - width on, so its phase is that of i*orig alone: when a
window starts at a multiple of orig, the window resampled yields the recording's own low-rate samples -- exactly, wherever the window holds the
sample's whole kernel support.  The grid of restore.py carries over with the requested overlap end = int(overlap * L) widened to

    end' = end + ((L - end) % orig)            so that step = L - end' and with it every window start is a multiple of orig,

and windows, heads, tails and owned ranges are restore.trimmed_windows(N, L, end', K), trimmed by m = K - 1 as for a FIR filter of K taps (more
than one window needs end' >= 2 m).  Every window is a job.  A window's observation row has L + Mw entries, Mw = ceil(new * L / orig): the
first L on the high-rate side (1 known from the result so far, -1 no direct observation, -2 absent), the rest on the low-rate side (0 observed:
y = the recording's low-rate sample, -1 unobserved: the kernel support leaves the window although the recording goes on there, -2 absent:
beyond the recording's last low-rate sample); ``window_state`` is the host reference.  ``RateObserved`` is the operator, on one HIP kernel
(aid_rate_observed: the loops of aid_resample_poly and aid_resample_poly_adj with selects); ``lowrate_gather`` builds the observations and
states of all windows of a pass in one launch; ``lowrate_passes`` is the pass code, driven with anything that has ``predict_resample``.  GPU
only; no fallback.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import degrade
from . import restore
from .restore import aligned_end

LOWRATE_TYPES = ("resample", "decimate")


class Rate(NamedTuple):
    """The geometry of one ratio: low-rate sample i*new + j reads high-rate samples [i*orig - width, i*orig - width + K)."""
    orig: int
    new: int
    width: int
    K: int
    decimate: bool = False


def rate_of(factor, filt_type: str = "resample") -> Rate:
    """(orig, new, width, K) of predict_bwe's degradation ``filt_type`` at ``factor``; an identity ratio is refused."""
    if filt_type == "resample":
        orig, new = degrade.bwe_resample_ratio(factor)
        width = degrade.sinc_kernel(orig, new)[1] if orig != new else 0
        rate = Rate(orig, new, width, 2 * width + orig)
    elif filt_type == "decimate":
        try:
            f = int(factor)
            whole = f == factor
        except (TypeError, ValueError):
            f, whole = 0, False
        if not (whole and 1 <= f <= 16):
            raise _lib.AidError(f"decimate: the factor must be an integer in [1, 16], got {factor!r}")
        rate = Rate(f, 1, 0, f, True)
    else:
        raise NotImplementedError(f"predict_bwe_lowrate_long: unknown filt_type {filt_type!r} (one of {', '.join(LOWRATE_TYPES)})")
    if rate.orig == rate.new:
        raise _lib.AidError(f"{filt_type} at factor {factor!r} is the identity ({rate.orig}:{rate.new}), so there is nothing to restore")
    return rate


def low_len(N: int, rate: Rate) -> int:
    """M: the number of low-rate samples of a recording of N high-rate samples (resample: ceil(new*N/orig); decimate: the reference's 0:-1:f)"""
    return (N - 2) // rate.orig + 1 if rate.decimate else -(-rate.new * N // rate.orig)


def default_length(M: int, rate: Rate) -> int:
    """the largest N with low_len(N) == M"""
    return M * rate.orig + 1 if rate.decimate else M * rate.orig // rate.new


def check_length(M: int, length, rate: Rate) -> int:
    """N for M low-rate samples: ``length``, which must be consistent with M, or the largest consistent one"""
    if length is None:
        return default_length(M, rate)
    N = int(length)
    if N != length or N < 1 or low_len(N, rate) != M:
        raise _lib.AidError(f"length = {length!r} is not consistent with the {M} low-rate samples of y at {rate.orig}:{rate.new}: a recording of "
                            f"{length!r} samples has {low_len(N, rate) if N == length and N >= 1 else 'no'} low-rate samples (the default is {default_length(M, rate)})")
    return N


def lowrate_windows(N: int, L: int, end: int, rate: Rate):
    """(start s, head, tail, lo, hi) of every window, as restore.trimmed_windows(N, L, end', K) with the aligned overlap end': every s is a
    multiple of rate.orig."""
    return restore.trimmed_windows(N, L, aligned_end(L, end, rate.orig), rate.K)


def lowrate_plan(R: int, N: int, L: int, end: int, rate: Rate):
    """(jobs_A, jobs_B): every even / odd window of every recording as (r, s, head, tail, lo, hi), ordered by recording and window"""
    return restore.every_window_plan(R, lowrate_windows(N, L, end, rate))


def window_len(L: int, rate: Rate) -> int:
    """Mw: the low-rate entries of a window of L samples"""
    return -(-rate.new * int(L) // rate.orig)


def window_state(N: int, M: int, L: int, rate: Rate, s: int, head: int, tail: int) -> np.ndarray:
    """The state of every entry of the window that starts at s (float32 [L + Mw]; host reference of aid_lowrate_gather).  High-rate entry i:
    -2 absent, 1 known, -1 otherwise.  Low-rate entry n: -2 absent, -1 unobserved, 0 observed.  The first match decides."""
    if s % rate.orig:
        raise _lib.AidError(f"window_state: the window start {s} is no multiple of the input period {rate.orig}")
    i = np.arange(L)
    known = (i < head) | (i >= L - tail)
    high = np.where(s + i >= N, -2.0, np.where(known, 1.0, -1.0))
    n = np.arange(window_len(L, rate))
    mrec = (s // rate.orig) * rate.new + n
    a0 = (n // rate.new) * rate.orig - rate.width
    unobserved = ((s > 0) & (a0 < 0)) | ((s + L < N) & (a0 + rate.K > L))
    low = np.where(mrec >= M, -2.0, np.where(unobserved, -1.0, 0.0))
    return np.concatenate([high, low]).astype(np.float32)


def rate_tables(rate: Rate, device):
    """(k [new, K], width, kT [K, new], j_lo [K], j_hi [K]) on ``device``: degrade.resample_tables for "resample"; for "decimate" the one-row
    table [1, 0, ..., 0] of K = f entries, built once per (f, device)."""
    if not rate.decimate:
        return degrade.resample_tables(rate.orig, rate.new, device)

    def build(device):
        k = torch.zeros(1, rate.K, dtype=torch.float32)
        k[0, 0] = 1.0
        j_hi = torch.zeros(rate.K, dtype=torch.int32)
        j_hi[0] = 1
        return (k.to(device), 0, k.t().contiguous().to(device), torch.zeros(rate.K, dtype=torch.int32).to(device), j_hi.to(device))
    return degrade.device_tables(("decimate", rate.orig), device, build)


class RateObserved(restore.WindowOperator):
    """Observation of x[B, L] through the resampler of ``tables`` = (k [new, K], width, kT [K, new], j_lo [K], j_hi [K]) on the GPU
    (degrade.resample_tables / rate_tables) with state[1|B, L + Mw] (float32 on the GPU; Mw = ceil(new * L / orig), L is taken from the row
    length).  With kh the first L states, kl the rest, xin = 0 where kh is absent, x elsewhere, and c = resample(xin):

        apply(x)       [B, L + Mw]: x where kh is known, 0 elsewhere  |  c where kl == 0, 0 elsewhere
        adjoint(g)     [B, L]: with a = the resampler's adjoint of (g_low where kl == 0, else 0): 0 where kh is absent, a + g_high where known,
                       a elsewhere

    The operator protocol of degrade.py over restore.WindowOperator (``rows(lo, hi)``; the tables and a shared state row stay shared).
    Linear: it keeps nothing between calls.  It changes the length, so there is no data-consistency projection.  With no known or absent
    sample and every low-rate state 0, the low side of apply and the adjoint of [0 | g] give SincResample's bits."""

    def __init__(self, tables, state: torch.Tensor):
        super().__init__(state, "[1|B, L + Mw]")
        k, width, kT, j_lo, j_hi = tables
        ok = all(torch.is_tensor(t) and t.is_cuda and t.is_contiguous() for t in (k, kT, j_lo, j_hi))
        if not (ok and k.dim() == 2 and k.dtype == kT.dtype == torch.float32 and tuple(kT.shape) == (k.shape[1], k.shape[0])
                and j_lo.dtype == j_hi.dtype == torch.int32 and j_lo.numel() == j_hi.numel() == k.shape[1] and k.shape[1] > 2 * int(width) >= 0):
            raise _lib.AidError("RateObserved: tables must be (k [new, K], width, kT [K, new], j_lo [K], j_hi [K]) on the GPU (degrade.resample_tables)")
        self.tables = tables
        self.new, self.K = k.shape
        self.width = int(width)
        self.orig = self.K - 2 * self.width
        row = state.shape[1]
        self.L = row * self.orig // (self.orig + self.new)
        self.Mw = -(-self.new * self.L // self.orig)
        if self.L < 1 or self.L + self.Mw != row:
            raise _lib.AidError(f"RateObserved: a state row of {row} entries is no L + ceil({self.new} L / {self.orig}) for any L >= 1")

    def _slice(self, lo: int, hi: int) -> "RateObserved":
        return RateObserved(self.tables, self._state_rows(lo, hi))

    def _run(self, mode, x):
        n_in, n_out = (self.L, self.L + self.Mw) if mode == 0 else (self.L + self.Mw, self.L)
        x = self._signal(x, n_in)
        B = x.shape[0]
        out = torch.empty((B, n_out), dtype=torch.float32, device=x.device)
        k, _, kT, j_lo, j_hi = self.tables
        _lib.call("aid_rate_observed", _lib.RateObservedParams(x.data_ptr(), self.state.data_ptr(), k.data_ptr(), kT.data_ptr(), j_lo.data_ptr(), j_hi.data_ptr(),
                                                               out.data_ptr(), self.L, self.Mw, n_in, self._state_ld, n_out,
                                                               B, mode, self.orig, self.new, self.width, self.K))
        return out

    def apply(self, x):
        """A(x): [B, L] -> [B, L + Mw]"""
        return self._run(0, x)

    def adjoint(self, g):
        """A^T(g): [B, L + Mw] -> [B, L]"""
        return self._run(1, g)


def lowrate_gather(rec: torch.Tensor, out: torch.Tensor, jobs: torch.Tensor, L: int, rate: Rate):
    """One aid_lowrate_gather launch on the current stream -> (y [J, L + Mw], state [J, L + Mw]): the observations and the states of every
    job's window (``window_state``); known samples from ``out`` [R, N], observed low-rate samples from ``rec`` [R, M], 0 elsewhere."""
    for t, what in ((rec, "rec"), (out, "out")):
        restore._rows(t, what)
    restore._table(jobs)
    (R, M), N = rec.shape, out.shape[1]
    if out.shape[0] != R or int(L) < 1 or M < 1 or N < 1:
        raise _lib.AidError(f"lowrate_gather: rec {tuple(rec.shape)} and out {tuple(out.shape)} do not match, or L = {L} is below 1")
    J, row = jobs.shape[0], int(L) + window_len(L, rate)
    y = torch.empty((J, row), dtype=torch.float32, device=rec.device)
    k = torch.empty((J, row), dtype=torch.float32, device=rec.device)
    if J:
        _lib.call("aid_lowrate_gather", _lib.LowrateGatherParams(rec.data_ptr(), out.data_ptr(), y.data_ptr(), k.data_ptr(), jobs.data_ptr(),
                                                                 int(L), row - int(L), N, M, rec.stride(0), out.stride(0),
                                                                 J, R, rate.orig, rate.new, rate.width, rate.K))
    return y, k


def check_lowrate_args(y: torch.Tensor, length, rate: Rate, L: int, end: int, max_batch: int, seeds):
    """The refusals of a bandwidth extension of whole low-rate recordings after rate_of's, all raised before anything is launched ->
    (rate, N).  What can be judged without a GPU is judged first; the device of y last."""
    restore.check_rows(y, "low-rate recordings [R, M]", nonempty=True)
    N = check_length(y.shape[1], length, rate)
    lowrate_windows(N, L, end, rate)                                       # (end' in [1, L/2); end' >= 2 (K - 1) with more than one window)
    restore.check_batch(y, max_batch, seeds, "bandwidth extension of whole low-rate recordings")
    return rate, N


def lowrate_group(y: torch.Tensor, checked, rate: Rate, L: int, end: int) -> restore.Group:
    """The part of a bandwidth extension of low-rate recordings that plans and builds: y [R, M] low-rate recordings on the GPU, (rate, N) of
    check_lowrate_args -> restore.Group(out = zeros [R, N], (jobs_A, jobs_B) of lowrate_plan, the aid_lowrate_gather closure).  The ratio is
    shared by every group of a call (``lowrate_step``, ``lowrate_predict``); the states of a job travel in the gathered rows."""
    R, N = y.shape[0], checked[1]
    out = torch.zeros((R, N), dtype=torch.float32, device=y.device)          # (every sample is owned; pass B's heads and tails lie in ranges pass A owns)
    return restore.Group(out, lowrate_plan(R, N, L, end, rate), lambda table: lowrate_gather(y, out, table, L, rate))


def lowrate_step(rate: Rate, L: int, end: int) -> int:
    """the aligned step L - end' of the grid at this ratio"""
    return L - aligned_end(L, end, rate.orig)


def lowrate_predict(sampler, rate: Rate, L: int, device):
    """predict(win, c0, c1) of a bandwidth extension of low-rate recordings: ``sampler.predict_resample`` through RateObserved(the ratio's
    tables on ``device``) over rows c0:c1 of the gathered (y, k)"""
    tables = rate_tables(rate, device)

    def predict(win, c0, c1):
        yw, kw = (t[c0:c1] for t in win)
        return sampler.predict_resample(yw, (c1 - c0, L), RateObserved(tables, kw))
    return predict


restore.long_task(name="bwe_lowrate", method="predict_bwe_lowrate_long", what="restored",
                  consistency="y + x - A(x) is undefined for an operator that changes the length", guided=None, entries=("length",),
                  call_args={"factor": restore.REQUIRED, "filt_type": "resample"}, prepare=lambda args, factor, filt_type: rate_of(factor, filt_type),
                  check=check_lowrate_args, build=lowrate_group, predict=lowrate_predict, step=lowrate_step)


def lowrate_passes(sampler, y: torch.Tensor, factor, filt_type: str, L: int, end: int, length=None, max_batch: int = 8,
                   seeds: Optional[Sequence[int]] = None) -> torch.Tensor:
    """The two passes over ``sampler.predict_resample(yw [B, L + Mw], (B, L), RateObserved(tables, kw [B, L + Mw])) -> [B, L]`` with
    B <= max_batch: y [R, M] low-rate recordings on the GPU (rows contiguous, any row stride) -> restored [R, N] at the high rate.  Per pass:
    one aid_lowrate_gather launch, the sampler calls, one aid_window_scatter launch per call (restore.run_task, with the aligned step
    L - end').  Recordings and result stay on the GPU.  Seeds as restore.restore_passes."""
    return restore.run_task(restore.LONG_TASKS["bwe_lowrate"], sampler, rate_of(factor, filt_type), [(y, length)], L, end, max_batch, seeds)[0]
