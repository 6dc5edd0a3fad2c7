"""Bandwidth extension of whole recordings, longer than one model segment, through an IIR filter ("cheby1", "biquad") -- in two batched sampler
passes (include/aid_bwe_long.h: aid_iir_observed, aid_iir_gather).

The recording was filtered as a whole: rec = lfilter(b, a, x) from a zero state.  A window cut out of rec is NOT the filtered window: the
recursion carries state from the start of the recording (bwe_long.NOT_WINDOWED).  But the state is in the recording: for every n >= order

    rec[n] = sum_{k=0..order} b_k x[n-k] - sum_{k=1..order} a_k rec[n-k],

and the feedback terms are samples of rec, which we hold.  A window that starts at s > 0 therefore takes its first ``order`` filtered samples
rec[s .. s + order) as the initial output state of the recursion -- SEED samples -- instead of as observations; from sample ``order`` on the
recursion uses only samples the window holds.  For the true signal this reproduces rec exactly in exact arithmetic, with no halo and no
approximation; with rec in float32 the rounding of the seeds (each off by <= 2^-24 max|rec|, each amplified by <= iir_amplification(a)) bounds
the deviation by ``seed_error_bound`` = order * amplification * 2^-24 relative to max|rec|, and it decays with the poles.

The window scheme is restore.trimmed_windows(N, L, end, order + 1), unchanged (m = order; more than one window needs end >= 2 order), every
window a job.  A sample of a window is in one of these STATES (``window_state``, first match): -2 absent (beyond the end of the recording),
-3 seed (s > 0 and i < order), 1 known (head / tail, from the result so far), 0 filtered.  Seeds come before "known", so the head of a pass-B
window starts at ``order``; a seed is never owned (lo >= order when s > 0).  -1 (unobserved) does not arise on the grid but stays a legal
state of the operator.  ``IIRObserved`` is the operator on one HIP kernel (aid_iir_observed, one workgroup per row, fp64 recursion);
``iir_gather`` builds the raw rows and states of all windows of a pass in one launch and turns the raw rows into observations with one
more (mode 3: the free response of the seeds is subtracted from the filtered samples, which makes the operator linear);
``bwe_iir_passes`` is the pass code, driven with anything that has ``predict_resample``.  GPU only; no fallback.

"biquad": torchaudio clamps the filtered signal to [-1, 1].  A recording with a sample |y| >= 1 is refused (one reduction on the GPU, read
once): there the clamp acted, so the recording no longer satisfies the recursion.  The window operator is the LINEAR filter.  This departs
from predict_bwe "biquad" on purpose, which also drops the gradient where the model's own filtered estimate leaves [-1, 1].
"""
from __future__ import annotations

import functools
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import bwe_long
from . import degrade
from . import restore

IIR_TYPES = ("cheby1", "biquad")
SEED = -3.0
# where the other degradations of predict_bwe go
ELSEWHERE = {"firwin": "predict_bwe_long", "firwin_hpf": "predict_bwe_long", "decimate": "predict_bwe_lowrate_long", "resample": "predict_bwe_lowrate_long"}


class IIRTable:
    """The coefficients of an IIR degradation as the kernels run them (degrade.iir_coefficients: rounded to float32, normalised, order <= 16,
    stability judged after rounding) with IIRFilter's conditioning refusal: ``b``, ``a`` float64 [order + 1], ``order``, ``amplification``
    (degrade.iir_amplification), ``seed_error_bound`` = order * amplification * 2^-24 (the most the float32 rounding of a window's seed
    samples moves its filtered samples, relative to max|rec|), and ``h`` float32 [2 (order + 1)], b then a, on the host until ``to``."""

    def __init__(self, filt, filt_type: str):
        if filt_type == "biquad":
            try:
                c = [float(torch.as_tensor(v, dtype=torch.float32).reshape(-1)[0]) for v in filt]
            except (TypeError, ValueError, IndexError, RuntimeError):
                c = []
            if len(c) != 6:
                raise _lib.AidError("IIRFilter: 'biquad' takes the six coefficients (b0, b1, b2, a0, a1, a2)")
            b, a = c[:3], c[3:]
        else:
            try:
                b, a = filt
            except (TypeError, ValueError):
                raise _lib.AidError("IIRFilter: 'cheby1' takes the coefficients (b, a)") from None
        to_np = lambda v: v.detach().cpu().double().numpy() if torch.is_tensor(v) else v                            # noqa: E731
        self.b, self.a = degrade.iir_coefficients(to_np(b), to_np(a))
        self.amplification = degrade.iir_amplification(self.a)
        if 2.0 ** -53 * self.amplification ** 2 > degrade.IIR_MAX_REL_ERROR:
            raise _lib.AidError(f"IIRFilter: the direct-form state of this filter is too ill-conditioned for the chunked recursion "
                                f"(amplification {self.amplification:.3g}: error ~{2.0 ** -53 * self.amplification ** 2:.1e} > "
                                f"{degrade.IIR_MAX_REL_ERROR:.0e}); use a lower order or a higher cut-off")
        self.order = self.b.size - 1
        self.K = self.order + 1
        self.seed_error_bound = self.order * self.amplification * 2.0 ** -24
        self.h = torch.from_numpy(np.concatenate([self.b, self.a]).astype(np.float32))

    def to(self, device) -> "IIRTable":
        self.h = self.h.to(device)
        return self


def iir_windows(N: int, L: int, end: int, order: int) -> List[Tuple[int, int, int, int, int]]:
    """(start s, head, tail, lo, hi) of every window of a recording of N samples seen through a recursion of this order:
    restore.trimmed_windows(N, L, end, order + 1).  More than one window needs end >= 2 order."""
    return restore.trimmed_windows(N, L, end, int(order) + 1)


def window_state(N: int, L: int, order: int, s: int, head: int, tail: int) -> np.ndarray:
    """The state of every sample of the window that starts at s (float32 [L]; host reference of aid_iir_gather): -2 absent, -3 seed, 1 known,
    0 filtered; the first match decides."""
    i = np.arange(L)
    seed = (s > 0) & (i < order)
    known = (i < head) | (i >= L - tail)
    return np.where(s + i >= N, -2.0, np.where(seed, SEED, np.where(known, 1.0, 0.0))).astype(np.float32)


def iir_plan(R: int, N: int, L: int, end: int, order: int):
    """(jobs_A, jobs_B): every even / odd window of every recording as (r, s, head, tail, lo, hi), ordered by recording and window"""
    return restore.every_window_plan(R, iir_windows(N, L, end, order))


class IIRObserved(restore.WindowOperator):
    """Observation of x[B, L] through the recursion of ``table`` with state[1|B, L] (float32 on the GPU; 0 filtered, 1 known, -1 unobserved,
    -2 absent, -3 seed).  Per row, with N = order and S = the length of the row's leading run of -3 states (a -3 after it counts as -1),
    xin = 0 where absent, x elsewhere, u[i] = sum_{k<=N, i-k>=0} b_k xin[i-k], yh[i] = 0 (i < S), yh[i] = u[i] - sum_{1<=k<=N, i-k>=S} a_k yh[i-k]:

        apply(x)       x where known, yh where filtered, 0 elsewhere
        adjoint(g)     g0 = g where filtered, else 0;  w[i] = 0 (i < S), w[i] = g0[i] - sum_{1<=k<=N, i+k<L} a_k w[i+k] (backwards);
                       c[j] = sum_{k<=N, j+k<L} b_k w[j+k];  0 where absent, c + g where known, c elsewhere
        project(x, y)  y where known, (y - yh) + x where filtered, x elsewhere
        prepare(raw)   a gathered raw row (rec at seed and filtered samples, the result so far at known ones) -> the observation row:
                       raw - r where filtered, r the input-free recursion started from the seeds (fp64, rounded once); raw where known; 0 elsewhere

    ``prepare`` is what makes the operator linear: |y' - apply(x)| over the filtered samples is |rec - (yh + r)|, the recursion seeded with the
    recording's own samples.  With S = 0 this is degrade.IIRFilter(clamp=False)'s operator (to rounding: the recursion is chunked differently).
    The protocol of degrade.py over restore.WindowOperator; the table and a shared state row stay shared.  It keeps nothing between calls."""

    def __init__(self, table: IIRTable, state: torch.Tensor):
        super().__init__(state, "[1|B, L]")
        if not isinstance(table, IIRTable):
            raise _lib.AidError("IIRObserved: the coefficients must be an IIRTable")
        if table.h.device != state.device:
            table.to(state.device)
        self.table, self.L = table, state.shape[1]
        self.order, self.K, self.seed_error_bound = table.order, table.K, table.seed_error_bound

    def _slice(self, lo: int, hi: int) -> "IIRObserved":
        return IIRObserved(self.table, self._state_rows(lo, hi))

    def _run(self, mode, x, y=None):
        x = self._signal(x, self.L)
        out = torch.empty_like(x)
        L = self.L
        _lib.call("aid_iir_observed", _lib.FirObservedParams(x.data_ptr(), _lib.ptr(y), self.state.data_ptr(), self.table.h.data_ptr(), out.data_ptr(),
                                                             x.shape[0], self.K, mode, L, L, L, self._state_ld, L))
        return out

    def apply(self, x):
        return self._run(0, x)

    def adjoint(self, g):
        return self._run(1, g)

    def project(self, x, y):
        return self._run(2, x, y=self._observation(x, y, self.L))

    def prepare(self, raw):
        return self._run(3, raw)


def iir_gather(rec: torch.Tensor, out: torch.Tensor, jobs: torch.Tensor, L: int, table: IIRTable):
    """One aid_iir_gather launch and one mode-3 aid_iir_observed launch on the current stream -> (y' [J, L], state [J, L]): the observations and
    the states of every job's window (``window_state``; IIRObserved.prepare of the raw rows)."""
    for t, what in ((rec, "rec"), (out, "out")):
        restore._rows(t, what)
    restore._table(jobs)
    R, N = rec.shape
    if out.shape != rec.shape or int(L) < 1:
        raise _lib.AidError(f"iir_gather: rec {tuple(rec.shape)} and out {tuple(out.shape)} do not match, or L = {L} is below 1")
    J = jobs.shape[0]
    raw = torch.empty((J, L), dtype=torch.float32, device=rec.device)
    k = torch.empty((J, L), dtype=torch.float32, device=rec.device)
    if not J:
        return raw, k
    table.to(rec.device)
    _lib.call("aid_iir_gather", _lib.BweGatherParams(rec.data_ptr(), out.data_ptr(), raw.data_ptr(), k.data_ptr(), jobs.data_ptr(),
                                                     J, R, table.K, int(L), N, rec.stride(0), out.stride(0)))
    return IIRObserved(table, k).prepare(raw), k


class IIRCall(NamedTuple):
    """What the groups of a call share: the filter type and table() -> the one coefficient table of the call (host until a group or the
    predict closure moves it).  The coefficients are judged at the first call, which is after the first group's recordings, and the table
    is made once."""
    filt_type: str
    table: Callable[[], IIRTable]


def bwe_iir_prepare(args, filt, filt_type: str) -> IIRCall:
    """The filter type, judged before any recording -> IIRCall"""
    if filt_type in ELSEWHERE:
        raise _lib.AidError(f"predict_bwe_iir_long covers IIR filters only ({', '.join(IIR_TYPES)}), not {filt_type!r}: use {ELSEWHERE[filt_type]}")
    if filt_type not in IIR_TYPES:
        raise NotImplementedError(f"predict_bwe_iir_long: unknown filt_type {filt_type!r}")
    return IIRCall(filt_type, functools.lru_cache(None)(lambda: IIRTable(filt, filt_type)))


def check_bwe_iir_args(y: torch.Tensor, state: IIRCall, L: int, end: int, max_batch: int, seeds) -> IIRTable:
    """The refusals of a bandwidth extension of whole recordings through an IIR filter after bwe_iir_prepare's, all raised before anything
    is launched -> the coefficient table (host).  What can be judged without a GPU is judged first; the device of y last."""
    restore.check_rows(y, "recordings [R, N]")
    table = state.table()
    iir_windows(y.shape[1], L, end, table.order)                         # (end in [1, L/2); end >= 2 order with more than one window)
    restore.check_batch(y, max_batch, seeds, "bandwidth extension of whole recordings")
    return table


def check_unclamped(y: torch.Tensor) -> None:
    """The "biquad" refusal that needs the samples: one reduction on the GPU, read once."""
    if y.numel() and float(y.abs().max()) >= 1.0:
        raise _lib.AidError("predict_bwe_iir_long: a 'biquad' recording holds a sample with |y| >= 1: torchaudio's clamp to [-1, 1] acted there, so the "
                            "recording no longer satisfies the recursion and its windows cannot be seeded from it")


def bwe_iir_group(y: torch.Tensor, table: IIRTable, state: IIRCall, L: int, end: int) -> restore.Group:
    """The part that plans and builds: y [R, N] recordings filtered through ``table`` on the GPU -> restore.Group(out = a copy of y,
    (jobs_A, jobs_B) of iir_plan, the iir_gather closure).  The table is the one every group of a call shares; the states of a job travel
    in the gathered rows."""
    table.to(y.device)
    if state.filt_type == "biquad":
        check_unclamped(y)
    R, N = y.shape
    out = y.clone(memory_format=torch.contiguous_format)
    return restore.Group(out, iir_plan(R, N, L, end, table.order), lambda jobs: iir_gather(y, out, jobs, L, table))


def bwe_iir_predict(sampler, state: IIRCall, L: int, device):
    """predict(win, c0, c1) of the mode: ``sampler.predict_resample`` through IIRObserved(the table on ``device``) over rows c0:c1 of the
    gathered (y', k)"""
    table = state.table().to(device)

    def predict(win, c0, c1):
        yw, kw = (t[c0:c1] for t in win)
        return sampler.predict_resample(yw, (c1 - c0, L), IIRObserved(table, kw))
    return predict


restore.long_task(name="bwe_iir", method="predict_bwe_iir_long", what="restored", consistency=None, guided=None, entries=(), call_args=bwe_long.FIR_CALL_ARGS,
                  prepare=bwe_iir_prepare, check=check_bwe_iir_args, build=bwe_iir_group, predict=bwe_iir_predict, step=restore.plain_step)


def bwe_iir_passes(sampler, y: torch.Tensor, filt, filt_type: str, L: int, end: int, max_batch: int = 8, seeds: Optional[Sequence[int]] = None) -> torch.Tensor:
    """The two passes over ``sampler.predict_resample(y'w [B, L], (B, L), IIRObserved(table, kw [B, L])) -> [B, L]`` with B <= max_batch:
    y [R, N] recordings filtered with ``filt`` on the GPU (rows contiguous, any row stride) -> restored [R, N].  Per pass: one aid_iir_gather
    and one mode-3 aid_iir_observed launch, the sampler calls, one aid_window_scatter launch per call (restore.run_task).  Seeds as
    restore.restore_passes."""
    return restore.run_task(restore.LONG_TASKS["bwe_iir"], sampler, bwe_iir_prepare(None, filt, filt_type), [(y,)], L, end, max_batch, seeds)[0]
