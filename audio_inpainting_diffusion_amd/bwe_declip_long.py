"""Bandwidth extension of whole recordings that are also clipped and have dropouts -- in two batched sampler passes
(include/aid_bwe_long.h: aid_fir_clip_observed; include/aid_restore.h: aid_gap_states).

The degradation model, applied to the recording as a whole, is

    y = mask * clamp(taps * x, -c_r, +c_r)

in THIS order and no other: the stride-1 FIR filter of bwe_long.py ("same" padding), then the hard clipper at one level c_r per recording, then
the dropouts (mask 1 = kept, 0 = dropped).  Restoring such a recording with the single-degradation modes one after the other is wrong:
declipping would "restore" peaks the low-pass had already removed, bandwidth extension would take the clipped samples as exact filtered
values, and inpainting would treat everything outside the gaps as clean.  Posterior sampling needs the chain as ONE observation operator, and
the window scheme already has the pieces.  The grid, the ownership, heads and tails are bwe_long's (restore.trimmed_windows(N, L, end, K):
every window a job, more than one window needs end >= 2 (K - 1)); the states are bwe_long's four (-2 absent, 1 known, -1 unobserved,
0 filtered) with one more rule: a filtered sample that was dropped is UNOBSERVED -- it exists and feeds its neighbours' filter sums, but has
no observation of its own -- which is exactly state -1 (``window_state``).  Clipping is pointwise after the filter, so it needs no state: a
filtered sample is observed through clamp(., -c_r, c_r), with c_r = +inf for a recording that is not clipped.

``FIRClipObserved`` is the window operator on one HIP kernel (aid_fir_clip_observed: aid_fir_observed's tile loop with the clipper in the
epilogue; the apply also writes the pre-clip sums, which gate the adjoint) -- one launch per apply and per adjoint.  ``bwe_declip_gather``
builds the rows of a pass: aid_bwe_gather unchanged, then aid_gap_states in place over its rows, and the level of every job.
``bwe_declip_passes`` is the pass code, driven with anything that has ``predict_resample``.  Guidance only: no projection onto the signals
consistent with a clipped, filtered observation exists.  GPU only; no fallback.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import bwe_long
from . import declip_long
from . import restore

NO_PROJECTION = "no projection exists for the clipped filter"


def window_state(N: int, L: int, K: int, s: int, head: int, tail: int, mask_row=None) -> np.ndarray:
    """The state of every sample of the window that starts at s (float32 [L]; host reference of aid_bwe_gather followed by aid_gap_states):
    bwe_long.window_state, then a state-0 sample whose mask is 0 becomes -1.  ``mask_row`` [N]: the mask of the window's recording (None: all
    ones)."""
    k = bwe_long.window_state(N, L, K, s, head, tail)
    if mask_row is not None:
        m = np.asarray(mask_row.detach().cpu().numpy() if torch.is_tensor(mask_row) else mask_row).reshape(-1)
        n_in = max(0, min(L, N - s))
        drop = np.zeros(L, dtype=bool)
        drop[:n_in] = m[s:s + n_in] == 0
        k[(k == 0) & drop] = -1.0
    return k


def levels_of(clip_value, R: int) -> np.ndarray:
    """clip_value -> R float32 levels: declip_long.clip_levels(clip_value, R) (a float or R floats, finite and > 0), or +inf for every
    recording when it is None (no clipping)."""
    if clip_value is None:
        return np.full((int(R),), np.inf, dtype=np.float32)
    return declip_long.clip_levels(clip_value, R)


def mask_rows(mask, R: int, N: int) -> Optional[torch.Tensor]:
    """mask [N], [1, N] or [R, N] (any dtype / device; 0 = dropped) -> [1|R, N] as it is, None for None; any other shape is refused"""
    if mask is None:
        return None
    if not torch.is_tensor(mask):
        raise _lib.AidError(f"mask must be a tensor [N], [1, N] or [R, N], got {type(mask).__name__}")
    if mask.dim() == 1:
        mask = mask.reshape(1, -1)
    if mask.dim() != 2 or mask.shape[1] != N or mask.shape[0] not in (1, R):
        raise _lib.AidError(f"mask {tuple(mask.shape)} does not match recordings {(R, N)} (y [R, N], mask [N], [1, N] or [R, N])")
    return mask


def check_observed(mask: Optional[torch.Tensor], R: int, N: int, L: int, end: int, K: int) -> None:
    """Refuse a recording with a job window that holds neither a filtered nor a known sample (a dropout that swallows a whole window): the
    sampler would draw that window from the prior alone.  Host code over a cumulative sum of the mask, as restore.restore_plan; the text names
    the recording and the window."""
    if mask is None:
        return
    rows = mask.shape[0]
    cum = torch.zeros((rows, N + 1), dtype=torch.int64)
    cum[:, 1:] = torch.cumsum(mask.detach().to("cpu") != 0, dim=1)
    P = (K - 1) // 2
    Q = K - 1 - P
    for w, (s, head, tail, lo, hi) in enumerate(restore.trimmed_windows(N, L, end, K)):
        n_in = min(L, N - s)
        known = min(head, n_in) + max(0, n_in - (L - tail))
        # filtered before the mask exactly on [f0, f1): not known, not within reach of a border the recording goes on behind, not absent
        f0, f1 = max(head, P if s > 0 else 0), min(L - tail, L - Q if s + L < N else L, n_in)
        if known or f1 <= f0:
            continue                                   # (a window bwe_long itself leaves without a filtered sample is not the mask's doing)
        for r in range(R):
            c = cum[r if rows > 1 else 0]
            if int(c[s + f1]) == int(c[s + f0]):
                raise _lib.AidError(f"recording {r}, window {w} (samples [{s}, {s + n_in})) holds neither a filtered nor a known sample: the "
                                    "dropout swallows the whole window, so nothing would condition it")


class FIRClipObserved(restore.WindowOperator):
    """Observation of x[B, L] through taps[K] ("same" correlation, as degrade.FIRFilter) followed by a hard clipper, with state[1|B, L]
    (float32 on the GPU; 0 filtered, 1 known, -1 unobserved, -2 absent) and clip[B] (levels > 0, +inf for "not clipped"; a float32 GPU tensor
    is used as it is and NOT inspected, anything else is checked on the host and uploaded).  With xin = 0 where absent, x elsewhere, and
    c = taps * xin:

        apply(x)       x where known, fminf(fmaxf(c, -c_b), c_b) where filtered, 0 where unobserved or absent
        adjoint(g)     with a = the FIRFilter adjoint of (g * [-c_b <= c <= c_b] where filtered, else 0), inclusive as HardClip, at the c of the
                       last ``apply`` on the current stream: 0 where absent, a + g where known, a elsewhere
        project(x, y)  raises: no projection onto the signals consistent with a clipped, filtered observation exists

    One aid_fir_clip_observed launch per call; composing FIRObserved and ClipObserved takes two and gives the same bits.  The operator
    protocol of degrade.py over restore.WindowOperator (``rows(lo, hi)``; the pre-clip c of an apply is kept per stream).  It holds one level
    per item, so it serves exactly B items even through a shared state row."""

    def __init__(self, taps, state: torch.Tensor, clip):
        super().__init__(state, "[1|B, L]")
        if torch.is_tensor(taps) and taps.is_cuda and taps.dtype == torch.float32 and taps.dim() == 1 and taps.is_contiguous() and taps.numel():
            self.taps = taps
        else:
            self.taps = bwe_long.fir_taps(taps).to(state.device)
        if torch.is_tensor(clip) and clip.is_cuda:
            if clip.dtype != torch.float32:
                raise _lib.AidError("FIRClipObserved: clip levels on the GPU must be float32")
            clip = clip.reshape(-1)
        else:
            c = np.asarray(clip.detach().cpu().numpy() if torch.is_tensor(clip) else clip, dtype=np.float64).reshape(-1).astype(np.float32)
            if c.size == 0 or not bool(np.all(c > 0)):
                raise _lib.AidError(f"every clip level must be > 0 (+inf: not clipped), got {c.tolist()}")
            clip = torch.from_numpy(c).to(state.device)
        if clip.numel() < 1 or state.shape[0] not in (1, clip.numel()):
            raise _lib.AidError(f"FIRClipObserved: {state.shape[0]} state rows for {clip.numel()} clip levels")
        self.clip = clip
        self.h = torch.cat([self.taps, clip])                                   # the table of the kernel: taps, then one level per item
        self.K, self.B, self.L = self.taps.numel(), clip.numel(), state.shape[1]

    @property
    def items_held(self) -> int:
        return self.B

    def _slice(self, lo: int, hi: int) -> "FIRClipObserved":
        return FIRClipObserved(self.taps, self._state_rows(lo, hi), self.clip[lo:hi])

    def _run(self, mode, x, y=None):
        x = self._signal(x, self.L)
        L, B = self.L, self.B
        out = torch.empty((2, B, L) if mode == 0 else (B, L), dtype=torch.float32, device=x.device)
        _lib.call("aid_fir_clip_observed", _lib.FirObservedParams(x.data_ptr(), _lib.ptr(y), self.state.data_ptr(), self.h.data_ptr(), out.data_ptr(),
                                                                  B, self.K, mode, L, L, L, self._state_ld, L))
        return out

    def apply(self, x):
        planes = self._run(0, x)
        self._keep(planes[1])
        return planes[0]

    def adjoint(self, g):
        return self._run(1, g, y=self._kept(g))

    def project(self, x, y):
        raise AttributeError(f"FIRClipObserved: {NO_PROJECTION}: set tester.data_consistency.use = False")


def gap_states(y: torch.Tensor, k: torch.Tensor, mask: torch.Tensor, jobs: torch.Tensor, R: int, N: int) -> None:
    """One aid_gap_states launch on the current stream, in place over the rows (y [J, L], k [J, L]) of bwe_long.bwe_gather for R recordings
    of N samples: a state-0 sample whose ``mask`` ([R, N] or [1, N], float32 on the GPU) is 0 becomes state -1 with observation 0."""
    restore._rows(mask, "mask")
    restore._table(jobs)
    J, R, N = jobs.shape[0], int(R), int(N)
    for t in (y, k):
        _lib._req(t)
    if not (y.dim() == 2 and y.shape[0] == J and y.shape == k.shape and y.is_contiguous() and k.is_contiguous()):
        raise _lib.AidError(f"gap_states: y and k must be contiguous [J = {J}, L], got {tuple(y.shape)} and {tuple(k.shape)}")
    if mask.shape[1] != N or mask.shape[0] not in (1, R):
        raise _lib.AidError(f"gap_states: mask {tuple(mask.shape)} does not match recordings {(R, N)} (mask [1, N] or [R, N])")
    if J:
        # (R bounds the r of a job; a shared mask row serves every recording through mask_ld = 0)
        _lib.call("aid_gap_states", _lib.WindowGatherParams(None, None, mask.data_ptr(), y.data_ptr(), k.data_ptr(), jobs.data_ptr(),
                                                            J, R, int(y.shape[1]), N, 0, 0, mask.stride(0) if mask.shape[0] > 1 else 0))


def bwe_declip_gather(rec: torch.Tensor, out: torch.Tensor, mask: Optional[torch.Tensor], levels: torch.Tensor, jobs: torch.Tensor, L: int, K: int):
    """The rows of a pass -> (y [J, L], state [J, L], c [J]): one aid_bwe_gather launch, one aid_gap_states launch over its rows (none without
    a mask: all ones changes nothing), and levels[r_j] per job, indexed on the device.  ``window_state`` is the host reference of the states."""
    y, k = bwe_long.bwe_gather(rec, out, jobs, L, K)
    if mask is not None:
        gap_states(y, k, mask, jobs, rec.shape[0], rec.shape[1])
    return y, k, levels[jobs[:, 0]]


def bwe_declip_prepare(args, filt, filt_type: str):
    """The filter type, judged before any recording -> bwe_long.fir_state(filt)"""
    if filt_type in bwe_long.NOT_WINDOWED:
        raise _lib.AidError(f"bandwidth extension of clipped whole recordings covers stride-1 FIR filters only ({', '.join(bwe_long.FIR_TYPES)}), "
                            f"not {filt_type!r}: " + bwe_long.NOT_WINDOWED[filt_type])
    if filt_type not in bwe_long.FIR_TYPES:
        raise NotImplementedError(f"predict_bwe_declip_long: unknown filt_type {filt_type!r}")
    return bwe_long.fir_state(filt)


def check_bwe_declip_args(y: torch.Tensor, clip_value, mask, state, L: int, end: int, max_batch: int, seeds) -> Tuple[torch.Tensor, np.ndarray, Optional[torch.Tensor]]:
    """The refusals of the mode after bwe_declip_prepare's, all raised before anything is launched -> (taps float32 [K] on the host, R levels
    float32 on the host, mask [1|R, N] or None).  What can be judged without a GPU is judged first -- the recordings, the taps and the grid as
    bwe_long.check_bwe_args, then the levels, the mask and the windows without any observation -- max_batch, the seeds and the device of y last."""
    restore.check_rows(y, "recordings [R, N]")
    taps = state()
    R, N = y.shape
    bwe_long.bwe_windows(N, L, end, taps.numel())                            # (end in [1, L/2); end >= 2 (K - 1) with more than one window)
    levels = levels_of(clip_value, R)
    mask = mask_rows(mask, R, N)
    check_observed(mask, R, N, L, end, taps.numel())
    restore.check_batch(y, max_batch, seeds, "bandwidth extension of clipped whole recordings")
    return taps, levels, mask


def bwe_declip_group(y: torch.Tensor, checked, state, L: int, end: int) -> restore.Group:
    """The part that plans and builds: y [R, N] degraded recordings on the GPU, (taps, levels, mask) of check_bwe_declip_args ->
    restore.Group(out = a copy of y, (jobs_A, jobs_B) of bwe_long.bwe_plan, the ``bwe_declip_gather`` closure).  The taps are shared by
    every group of a call (``bwe_declip_predict``); the states and the level of a job travel in the gathered rows, so groups of other
    lengths, levels and masks can share the predict closure."""
    taps, levels, mask = checked
    K = taps.numel()
    R, N = y.shape
    out = y.clone(memory_format=torch.contiguous_format)
    dlevels = torch.from_numpy(levels).to(y.device)
    dmask = None if mask is None else mask.to(y.device, torch.float32).contiguous()
    return restore.Group(out, bwe_long.bwe_plan(R, N, L, end, K), lambda table: bwe_declip_gather(y, out, dmask, dlevels, table, L, K))


def bwe_declip_predict(sampler, state, L: int, device):
    """predict(win, c0, c1) of the mode: ``sampler.predict_resample`` through FIRClipObserved(taps on ``device``) over rows c0:c1 of the
    gathered (y, k, c)"""
    dtaps = state().to(device)

    def predict(win, c0, c1):
        yw, kw, cw = (t[c0:c1] for t in win)
        return sampler.predict_resample(yw, (c1 - c0, L), FIRClipObserved(dtaps, kw, cw))
    return predict


restore.long_task(name="bwe_declip", method="predict_bwe_declip_long", what="restored", consistency=NO_PROJECTION, guided=None, entries=("clip_value", "mask"),
                  call_args=bwe_long.FIR_CALL_ARGS, prepare=bwe_declip_prepare, check=check_bwe_declip_args, build=bwe_declip_group,
                  predict=bwe_declip_predict, step=restore.plain_step)


def bwe_declip_passes(sampler, y: torch.Tensor, filt, filt_type: str, clip_value, mask, L: int, end: int, max_batch: int = 8,
                      seeds: Optional[Sequence[int]] = None) -> torch.Tensor:
    """The two passes over ``sampler.predict_resample(yw [B, L], (B, L), FIRClipObserved(taps, kw [B, L], cw [B])) -> [B, L]`` with
    B <= max_batch: y [R, N] recordings filtered with ``filt``, clipped at ``clip_value`` and dropped where ``mask`` is 0, on the GPU (rows
    contiguous, any row stride) -> restored [R, N].  Per pass: one aid_bwe_gather and one aid_gap_states launch, the sampler calls, one
    aid_window_scatter launch per call (restore.run_task).  Recordings and result stay on the GPU.  Seeds as restore.restore_passes."""
    return restore.run_task(restore.LONG_TASKS["bwe_declip"], sampler, bwe_declip_prepare(None, filt, filt_type), [(y, clip_value, mask)],
                            L, end, max_batch, seeds)[0]
