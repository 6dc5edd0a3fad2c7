"""Bandwidth extension of whole recordings, longer than one model segment, through a stride-1 FIR filter -- in two batched sampler passes
(include/aid_bwe_long.h).

The recording was low-passed as a whole: rec = taps * x with "same" padding (zeros before the first and after the last sample).  A window cut
out of rec is NOT the filtered window: within reach of a window border the filter saw samples the window does not hold.  With K taps,
P = (K-1)//2 (left reach), Q = K-1-P (right reach) and m = K-1, a sample of a window is used as an observation only when the window holds
its whole filter support; no halo is subtracted from anything.  The window scheme of restore.py carries over -- the autoregressive grid, the
even windows as pass A, the odd ones as pass B, seeds, aid_window_scatter -- with the ownership trimmed by m, so that every window owns only
samples whose observation it used:

    even w                      [s_w + (m if w else 0), s_w + L - (0 if last else m))
    odd  w                      [s_w + end - m, s_w + L - end + m)       head = tail = end - m known from the result so far
    odd last w (no neighbour)   [s_w + end - m, s_w + L)                 head = end - m, tail = 0

which tiles [0, N) whenever end >= 2 m (required with more than one window).  Every window is a job.  A sample of a window is in one of four
STATES (``window_state``, first match): -2 absent (beyond the end of the recording; it enters the filter as 0, the recording's own padding),
1 known (head / tail, taken from the result so far), -1 unobserved (it exists and feeds its neighbours' observations, but its own filtered
value depends on samples outside the window: the first P samples of a window that does not start the recording, the last Q of one that does
not reach its end), 0 filtered (y = rec).  For the true signal the window operator reproduces rec at every state-0 sample exactly: it is the
same dot product.  ``FIRObserved`` is that operator, on one HIP kernel (aid_fir_observed: the tile loop of aid_fir with a select where the
tile is staged and one in the epilogue); ``bwe_gather`` builds the observations and states of all windows of a pass in one launch;
``bwe_passes`` is the pass code, driven with anything that has ``predict_resample``.  GPU only; no fallback.
"""
from __future__ import annotations

import functools
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import restore

FIR_TYPES = ("firwin", "firwin_hpf")
# why the other degradations of predict_bwe do not window
_IIR = ("an IIR filter carries state from the start of the recording, so a window cut out of the filtered recording is not the filtered window "
        "(predict_bwe_iir_long seeds the recursion of every window from the recording instead).")
NOT_WINDOWED = {
    "cheby1": _IIR,
    "biquad": _IIR,
    "decimate": "a decimator's phase depends on the window start, so the windows of the grid do not see the recording's samples.",
    "resample": "a resampler is a decimator whose phase depends on the window start, so the windows of the grid do not see the recording's samples.",
}


def bwe_windows(N: int, L: int, end: int, K: int) -> List[Tuple[int, int, int, int, int]]:
    """(start s, head, tail, lo, hi) of every window of a recording of N samples seen through K taps: restore.trimmed_windows(N, L, end, K),
    the grid of restore.restore_windows with heads, tails and owned ranges trimmed by m = K - 1.  More than one window needs end >= 2 m."""
    return restore.trimmed_windows(N, L, end, K)


def window_state(N: int, L: int, K: int, s: int, head: int, tail: int) -> np.ndarray:
    """The state of every sample of the window that starts at s (float32 [L]; host reference of aid_bwe_gather): -2 absent, 1 known,
    -1 unobserved, 0 filtered; the first match decides."""
    P = (K - 1) // 2
    Q = K - 1 - P
    i = np.arange(L)
    unobserved = ((s > 0) & (i < P)) | ((s + L < N) & (i >= L - Q))
    known = (i < head) | (i >= L - tail)
    return np.where(s + i >= N, -2.0, np.where(known, 1.0, np.where(unobserved, -1.0, 0.0))).astype(np.float32)


def bwe_plan(R: int, N: int, L: int, end: int, K: int):
    """(jobs_A, jobs_B): every even / odd window of every recording as (r, s, head, tail, lo, hi), ordered by recording and window -- all
    samples are degraded, so every window is a job."""
    return restore.every_window_plan(R, bwe_windows(N, L, end, K))


def fir_taps(filt) -> torch.Tensor:
    """taps [K], [1, K] or [1, 1, K] (as predict_bwe takes them) -> float32 [K] on the host"""
    t = torch.as_tensor(filt).detach()
    if t.dim() == 0 or t.numel() != t.shape[-1] or t.numel() == 0:
        raise _lib.AidError(f"taps must be [K], [1, K] or [1, 1, K], got {tuple(t.shape)}")
    return t.reshape(-1).to("cpu", torch.float32).contiguous()


class FIRObserved(restore.WindowOperator):
    """Observation of x[B, L] through taps[K] ("same" correlation, as degrade.FIRFilter) with state[1|B, L] (float32 on the GPU; 0 filtered,
    1 known, -1 unobserved, -2 absent).  With xin = 0 where absent, x elsewhere, and c = taps * xin:

        apply(x)       x where known, c where filtered, 0 where unobserved or absent
        adjoint(g)     with a = the FIRFilter adjoint of (g where filtered, else 0): 0 where absent, a + g where known, a elsewhere
        project(x, y)  y where known, (-c + y) + x where filtered (the reference's data_consistency_step, in FIRFilter.project's order),
                       x where unobserved or absent

    The operator protocol of degrade.py over restore.WindowOperator (``rows(lo, hi)``; the taps and a shared state row stay shared).
    Linear: it keeps nothing between calls.  With every state 0, apply and adjoint give FIRFilter's bits."""

    def __init__(self, taps, state: torch.Tensor):
        super().__init__(state, "[1|B, L]")
        if torch.is_tensor(taps) and taps.is_cuda and taps.dtype == torch.float32 and taps.dim() == 1 and taps.is_contiguous() and taps.numel():
            self.taps = taps
        else:
            self.taps = fir_taps(taps).to(state.device)
        self.K, self.L = self.taps.numel(), state.shape[1]

    def _slice(self, lo: int, hi: int) -> "FIRObserved":
        return FIRObserved(self.taps, self._state_rows(lo, hi))

    def _run(self, mode, x, y=None):
        x = self._signal(x, self.L)
        out = torch.empty_like(x)
        L = self.L
        _lib.call("aid_fir_observed", _lib.FirObservedParams(x.data_ptr(), _lib.ptr(y), self.state.data_ptr(), self.taps.data_ptr(), out.data_ptr(),
                                                             x.shape[0], self.K, mode, L, L, L, self._state_ld, L))
        return out

    def apply(self, x):
        return self._run(0, x)

    def adjoint(self, g):
        return self._run(1, g)

    def project(self, x, y):
        return self._run(2, x, y=self._observation(x, y, self.L))


def bwe_gather(rec: torch.Tensor, out: torch.Tensor, jobs: torch.Tensor, L: int, K: int):
    """One aid_bwe_gather launch on the current stream -> (y [J, L], state [J, L]): the observations and the states of every job's window
    (``window_state``); known samples from ``out``, filtered ones from ``rec``, 0 where there is no observation."""
    for t, what in ((rec, "rec"), (out, "out")):
        restore._rows(t, what)
    restore._table(jobs)
    R, N = rec.shape
    if out.shape != rec.shape or int(K) < 1 or int(L) < 1:
        raise _lib.AidError(f"bwe_gather: rec {tuple(rec.shape)} and out {tuple(out.shape)} do not match, or K = {K} / L = {L} is below 1")
    J = jobs.shape[0]
    y = torch.empty((J, L), dtype=torch.float32, device=rec.device)
    k = torch.empty((J, L), dtype=torch.float32, device=rec.device)
    if J:
        _lib.call("aid_bwe_gather", _lib.BweGatherParams(rec.data_ptr(), out.data_ptr(), y.data_ptr(), k.data_ptr(), jobs.data_ptr(),
                                                         J, R, int(K), int(L), N, rec.stride(0), out.stride(0)))
    return y, k


def fir_state(filt):
    """What the groups of a call through FIR taps share: taps() -> float32 [K] on the host.  The taps are judged at the first call, which
    is after the first group's recordings, and made once."""
    return functools.lru_cache(None)(lambda: fir_taps(filt))


def bwe_prepare(args, filt, filt_type: str):
    """The filter type, judged before any recording -> fir_state(filt)"""
    if filt_type in NOT_WINDOWED:
        raise _lib.AidError(f"bandwidth extension of whole recordings covers stride-1 FIR filters only ({', '.join(FIR_TYPES)}), not {filt_type!r}: "
                            + NOT_WINDOWED[filt_type])
    if filt_type not in FIR_TYPES:
        raise NotImplementedError(f"predict_bwe_long: unknown filt_type {filt_type!r}")
    return fir_state(filt)


def check_bwe_args(y: torch.Tensor, state, L: int, end: int, max_batch: int, seeds) -> torch.Tensor:
    """The refusals of a bandwidth extension of whole recordings after bwe_prepare's, all raised before anything is launched -> the taps
    (float32 [K], host).  What can be judged without a GPU is judged first; the device of y last."""
    restore.check_rows(y, "recordings [R, N]")
    taps = state()
    bwe_windows(y.shape[1], L, end, taps.numel())                        # (end in [1, L/2); end >= 2 (K - 1) with more than one window)
    restore.check_batch(y, max_batch, seeds, "bandwidth extension of whole recordings")
    return taps


def bwe_group(y: torch.Tensor, taps: torch.Tensor, state, L: int, end: int) -> restore.Group:
    """The part of a bandwidth extension that plans and builds: y [R, N] recordings filtered with ``taps`` on the GPU ->
    restore.Group(out = a copy of y, (jobs_A, jobs_B) of bwe_plan, the aid_bwe_gather closure).  The taps are shared by every group of a
    call (``bwe_predict``); the states of a job travel in the gathered rows."""
    K = taps.numel()
    R, N = y.shape
    out = y.clone(memory_format=torch.contiguous_format)
    return restore.Group(out, bwe_plan(R, N, L, end, K), lambda table: bwe_gather(y, out, table, L, K))


def bwe_predict(sampler, state, L: int, device):
    """predict(win, c0, c1) of a bandwidth extension: ``sampler.predict_resample`` through FIRObserved(taps on ``device``) over rows c0:c1 of the
    gathered (y, k)"""
    dtaps = state().to(device)

    def predict(win, c0, c1):
        yw, kw = (t[c0:c1] for t in win)
        return sampler.predict_resample(yw, (c1 - c0, L), FIRObserved(dtaps, kw))
    return predict


FIR_CALL_ARGS = {"filt": restore.REQUIRED, "filt_type": restore.REQUIRED}
restore.long_task(name="bwe", method="predict_bwe_long", what="restored", consistency=None, guided=None, entries=(), call_args=FIR_CALL_ARGS,
                  prepare=bwe_prepare, check=check_bwe_args, build=bwe_group, predict=bwe_predict, step=restore.plain_step)


def bwe_passes(sampler, y: torch.Tensor, filt, filt_type: str, L: int, end: int, max_batch: int = 8, seeds: Optional[Sequence[int]] = None) -> torch.Tensor:
    """The two passes over ``sampler.predict_resample(yw [B, L], (B, L), FIRObserved(taps, kw [B, L])) -> [B, L]`` with B <= max_batch:
    y [R, N] recordings filtered with ``filt`` on the GPU (rows contiguous, any row stride) -> restored [R, N].  Per pass: one aid_bwe_gather
    launch, the sampler calls, one aid_window_scatter launch per call (restore.run_task).  Recordings and result stay on the GPU.  Seeds
    as restore.restore_passes."""
    return restore.run_task(restore.LONG_TASKS["bwe"], sampler, bwe_prepare(None, filt, filt_type), [(y,)], L, end, max_batch, seeds)[0]
