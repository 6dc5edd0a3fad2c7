"""Declipping of whole recordings, longer than one model segment, in two batched sampler passes (include/aid_declip.h).

Hard clipping is pointwise, so a window cut out of a clipped recording is exactly the clipped window, and the window scheme of restore.py
carries over unchanged: the autoregressive grid, sample ownership, the even windows as pass A, the odd ones as pass B, seeds and
aid_window_scatter.  A window is a job when its owned range holds a clipped sample (|y| >= c of its recording) -- the plan is
``restore.restore_plan`` over the mask |y| < c.  What differs from inpainting is the observation of a window: most samples are seen through
the clipper, the first and last ``end`` samples of a pass-B window are KNOWN (what pass A, or the recording, left there), and the samples
of a last window beyond the end of the recording are ABSENT.  ``ClipObserved`` is that operator, on one HIP kernel (aid_clip_known) with a
per-sample state (0 clipped, 1 known, -1 absent) and a clip level per item; ``declip_gather`` builds the observations, states and levels
of all windows of a pass in one launch; ``declip_passes`` is the pass code, driven with anything that has ``predict_resample``.
GPU only; no fallback.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import restore


class ClipObserved(restore.WindowOperator):
    """Observation of x[B, L] with state[1|B, L] (float32 on the GPU; 0 clipped, 1 known, -1 absent) and clip[B] (levels > 0; a float32 GPU
    tensor is used as it is and NOT inspected, anything else is checked on the host and uploaded):

        apply(x)       x where known, clamp(x, -c_b, c_b) where clipped, 0 where absent
        adjoint(g)     g where known, g * (-c_b <= x_hat <= c_b) where clipped (inclusive, as HardClip), 0 where absent, at the x_hat of the
                       last ``apply`` on the current stream
        project(x, y)  the point nearest to x among the signals consistent with y: y where known or |y| < c_b, max(x, c_b) where y >= c_b,
                       min(x, -c_b) where y <= -c_b, x where absent

    The operator protocol of degrade.py over restore.WindowOperator (``rows(lo, hi)``, the per-stream x_hat).  It holds one level per item,
    so it serves exactly B items even through a shared state row."""

    def __init__(self, state: torch.Tensor, clip):
        super().__init__(state, "[1|B, L]")
        if torch.is_tensor(clip) and clip.is_cuda:
            if clip.dtype != torch.float32:
                raise _lib.AidError("ClipObserved: clip levels on the GPU must be float32")
            clip = clip.reshape(-1).contiguous()
        else:
            clip = torch.from_numpy(clip_levels(clip)).to(state.device)
        if state.shape[0] not in (1, clip.numel()):
            raise _lib.AidError(f"ClipObserved: {state.shape[0]} state rows for {clip.numel()} clip levels")
        self.clip = clip
        self.B, self.L = clip.numel(), state.shape[1]

    @property
    def items_held(self) -> int:
        return self.B

    def _slice(self, lo: int, hi: int) -> "ClipObserved":
        return ClipObserved(self._state_rows(lo, hi), self.clip[lo:hi])

    def _run(self, mode, x, xref=None, y=None):
        x = self._signal(x, self.L)
        out = torch.empty_like(x)
        L = self.L
        _lib.call("aid_clip_known", _lib.ClipKnownParams(x.data_ptr(), _lib.ptr(xref), _lib.ptr(y), self.state.data_ptr(), self.clip.data_ptr(), out.data_ptr(),
                                                         self.B, mode, L, L, L, L, self._state_ld, L))
        return out, x

    def apply(self, x):
        out, x = self._run(0, x)
        self._keep(x)
        return out

    def adjoint(self, g):
        return self._run(1, g, xref=self._kept(g))[0]

    def project(self, x, y):
        return self._run(2, x, y=self._observation(x, y, self.L))[0]


def clip_levels(clip_value, R: Optional[int] = None) -> np.ndarray:
    """A float or a sequence / tensor of floats -> float32 levels (rounded to float32 as HardClip does), each finite and > 0; with ``R``, one level is
    repeated for R recordings and any other count than 1 or R is refused."""
    v = clip_value.detach().cpu().numpy() if torch.is_tensor(clip_value) else clip_value
    c = np.asarray(v, dtype=np.float64).reshape(-1).astype(np.float32)
    if c.size == 0 or not bool(np.all(np.isfinite(c) & (c > 0))):
        raise _lib.AidError(f"every clip level must be finite and > 0, got {c.tolist()}")
    if R is not None:
        if c.size not in (1, R):
            raise _lib.AidError(f"{c.size} clip levels for {R} recordings (one for all, or one each)")
        c = np.array(np.broadcast_to(c, (R,)))
    return c


def declip_gather(rec: torch.Tensor, out: torch.Tensor, clip: torch.Tensor, jobs: torch.Tensor, L: int):
    """One aid_declip_gather launch on the current stream -> (y [J, L], k [J, L], c [J]): the observations, the states and the clip level of every
    job's window; the first ``head`` / last ``tail`` samples known from ``out``, the rest the clipped ``rec``, samples from N on absent."""
    for t, what in ((rec, "rec"), (out, "out")):
        restore._rows(t, what)
    restore._table(jobs)
    R, N = rec.shape
    if out.shape != rec.shape or not (clip.is_cuda and clip.dtype == torch.float32 and clip.dim() == 1 and clip.numel() == R and clip.is_contiguous()):
        raise _lib.AidError(f"declip_gather: rec {tuple(rec.shape)}, out {tuple(out.shape)} and clip {tuple(clip.shape)} do not match (clip: float32 [R] on the GPU)")
    J = jobs.shape[0]
    y = torch.empty((J, L), dtype=torch.float32, device=rec.device)
    k = torch.empty((J, L), dtype=torch.float32, device=rec.device)
    c = torch.empty((J,), dtype=torch.float32, device=rec.device)
    if J:
        _lib.call("aid_declip_gather", _lib.DeclipGatherParams(rec.data_ptr(), out.data_ptr(), clip.data_ptr(), y.data_ptr(), k.data_ptr(), c.data_ptr(), jobs.data_ptr(),
                                                               J, R, int(L), N, rec.stride(0), out.stride(0)))
    return y, k, c


def check_declip_args(y: torch.Tensor, clip, state, L: int, end: int, max_batch: int, seeds) -> np.ndarray:
    """The refusals of a declipping run, all raised before anything is launched -> the R clip levels (float32, host).  What can be judged
    without a GPU is judged first; the device of y last."""
    restore.check_rows(y, "recordings [R, N]")
    levels = clip_levels(clip, y.shape[0])
    restore.restore_windows(y.shape[1], L, end)                       # (end in [1, L/2))
    restore.check_batch(y, max_batch, seeds, "declipping of whole recordings")
    return levels


def declip_plan(y: torch.Tensor, levels, L: int, end: int):
    """restore_plan over the mask |y| < c_r (float32 comparison, on y's device): a window is a job exactly when its owned range holds a sample
    with |y| >= c_r.  y [R, N], levels [R] -> (jobs_A, jobs_B, N_pad)."""
    c = torch.from_numpy(np.array(levels, dtype=np.float32)).to(y.device)
    return restore.restore_plan(y.abs() < c[:, None], L, end, y.shape[0])


def declip_group(y: torch.Tensor, levels: np.ndarray, state, L: int, end: int) -> restore.Group:
    """The part of a declipping run that plans and builds: y [R, N] clipped recordings on the GPU, the R levels of check_declip_args ->
    restore.Group(out = a copy of y, (jobs_A, jobs_B) of declip_plan, the aid_declip_gather closure).  The clip level of a job travels in
    the gathered rows, so groups of other lengths and levels can share ``declip_predict``."""
    jobs_A, jobs_B, _ = declip_plan(y, levels, L, end)
    out = y.clone(memory_format=torch.contiguous_format)
    dclip = torch.from_numpy(levels).to(y.device) if jobs_A or jobs_B else None
    return restore.Group(out, (jobs_A, jobs_B), lambda table: declip_gather(y, out, dclip, table, L))


def declip_predict(sampler, state, L: int, device):
    """predict(win, c0, c1) of a declipping run: ``sampler.predict_resample`` through ClipObserved over rows c0:c1 of the gathered (y, k, c)"""
    def predict(win, c0, c1):
        yw, kw, cw = (t[c0:c1] for t in win)
        return sampler.predict_resample(yw, (c1 - c0, L), ClipObserved(kw, cw))
    return predict


restore.long_task(name="declipping", method="predict_declipping_long", what="declipped", consistency=None, guided=None, entries=("clip_value",), call_args={},
                  prepare=lambda args: None, check=check_declip_args, build=declip_group, predict=declip_predict, step=restore.plain_step)


def declip_passes(sampler, y: torch.Tensor, clip, L: int, end: int, max_batch: int = 8, seeds: Optional[Sequence[int]] = None) -> torch.Tensor:
    """The two passes over ``sampler.predict_resample(yw [B, L], (B, L), ClipObserved(kw [B, L], cw [B])) -> [B, L]`` with B <= max_batch:
    y [R, N] clipped recordings on the GPU (rows contiguous, any row stride), clip a level or R levels -> declipped [R, N].  Per pass: one
    aid_declip_gather launch, the sampler calls, one aid_window_scatter launch per call (restore.run_task).  Recordings and result stay on
    the GPU; the plan is made on the host from |y| < c before pass A.  Seeds as restore.restore_passes."""
    return restore.run_task(restore.LONG_TASKS["declipping"], sampler, None, [(y, clip)], L, end, max_batch, seeds)[0]
