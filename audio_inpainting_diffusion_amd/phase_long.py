"""Phase retrieval of whole recordings, longer than one model segment, from their STFT magnitude -- in two batched sampler passes
(include/aid_phase_long.h).

The recording x [N] is known only by rec [F, T_rec] = |STFT| as the reference's SamplerPhaseRetrieval.apply_stft takes it (phase.py): win_size
zeros appended, periodic Hamming window, center=False, one-sided.  Frame t reads samples [t*hop, t*hop + n_fft) with zeros past the end, so
T_rec = 1 + N // hop.  A frame that straddles a window border is not the window's frame; a frame that lies inside a window that starts at a
multiple of hop is the recording's own frame -- the same n_fft samples times the same window.  The grid of restore.py carries over with the
requested overlap end = int(overlap * L) widened to

    end' = end + ((L - end) % hop)              so that step = L - end' and with it every window start is a multiple of hop
                                                (restore.aligned_end),

and windows, heads, tails and owned ranges are restore.trimmed_windows(N, L, end', K = n_fft), trimmed by m = n_fft - 1 as for a FIR filter of
n_fft taps (more than one window needs end' >= 2 m; always 2 end' < L).  Every window is a job.  A window's observation row has L + F*Tw
entries, Tw = 1 + L // hop: the first L are samples (1 known from the result so far, -1 no direct observation, -2 absent), the rest is the
[F, Tw] magnitude block with frames contiguous (STFTMagnitude's layout).  Its state row has L + Tw entries, one per sample and one per frame
(0 observed: y = the recording's magnitude column, -1 unobserved: the frame leaves the window although the recording goes on, -2 absent: past
the recording's last frame); ``window_state`` is the host reference.  A window that reaches the end of the recording sees the absent samples as
0, which is the recording's own appended zeros, so its last frames are exact too; there is no left reach.

THE GUIDANCE NORM.  ``STFTMagObserved`` declares no ``matrix_obs``: the guidance norm is the element-wise one over the whole row
(aid_guidance_seed: 2, 1 or "smoothl1").  This is a deliberate departure from predict_pr, where the reference's dim=(1, 2) makes ord 2 the
spectral norm of one segment's spectrogram: an induced matrix norm has no meaning across windows, and known samples do not fit in the matrix.

``STFTMagObserved`` is the operator, on the HIP kernels of csrc/aid_phase_long.hip (aid_stft_mag_observed: the frame and overlap-add bodies of
aid_stft_mag with selects); ``pr_gather`` builds the observations and states of all windows of a pass in one launch; ``pr_passes`` is the
pass code, driven with anything that has ``predict_resample``.  GPU only; no fallback.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import degrade
from . import phase
from . import restore
from .restore import aligned_end


def frames_of(N: int, hop: int) -> int:
    """T_rec: the number of STFT frames of a recording of N samples"""
    return 1 + int(N) // int(hop)


def default_length(T_rec: int, hop: int) -> int:
    """the largest N with frames_of(N, hop) == T_rec"""
    return int(T_rec) * int(hop) - 1


def check_length(T_rec: int, length, hop: int) -> int:
    """N for T_rec frames: ``length``, which must be consistent with T_rec, or the largest consistent one"""
    if length is None:
        N = default_length(T_rec, hop)
        if N < 1:
            raise _lib.AidError(f"{T_rec} frames at hop_size {hop} hold no sample")
        return N
    N = int(length)
    if N != length or N < 1 or frames_of(N, hop) != T_rec:
        raise _lib.AidError(f"length = {length!r} is not consistent with the {T_rec} frames of y at hop_size {hop}: a recording of {length!r} samples "
                            f"has {frames_of(N, hop) if N == length and N >= 1 else 'no'} frames (the default is {default_length(T_rec, hop)})")
    return N


def pr_windows(N: int, L: int, end: int, n_fft: int, hop: int):
    """(start s, head, tail, lo, hi) of every window, as restore.trimmed_windows(N, L, end', n_fft) with the aligned overlap end': every s
    is a multiple of hop."""
    return restore.trimmed_windows(N, L, aligned_end(L, end, hop), n_fft)


def pr_plan(R: int, N: int, L: int, end: int, n_fft: int, hop: int):
    """(jobs_A, jobs_B): every even / odd window of every recording as (r, s, head, tail, lo, hi), ordered by recording and window"""
    return restore.every_window_plan(R, pr_windows(N, L, end, n_fft, hop))


def window_state(N: int, L: int, n_fft: int, hop: int, s: int, head: int, tail: int) -> np.ndarray:
    """The state of every sample and every frame of the window that starts at s (float32 [L + Tw]; host reference of aid_pr_gather).
    Sample i: -2 absent, 1 known, -1 otherwise.  Frame j: -2 absent, -1 unobserved, 0 observed.  The first match decides."""
    if s % hop:
        raise _lib.AidError(f"window_state: the window start {s} is no multiple of hop_size {hop}")
    i = np.arange(L)
    known = (i < head) | (i >= L - tail)
    samples = np.where(s + i >= N, -2.0, np.where(known, 1.0, -1.0))
    j = np.arange(frames_of(L, hop))
    unobserved = (s + L < N) & (j * hop + n_fft > L)
    frames = np.where(s // hop + j >= frames_of(N, hop), -2.0, np.where(unobserved, -1.0, 0.0))
    return np.concatenate([samples, frames]).astype(np.float32)


def tables(n_fft: int, device):
    """(window [n_fft], twiddle [n_fft/2, 2]) of phase.hamming_tables as float32 on ``device``, built once per (n_fft, device)"""
    def build(device):
        return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device) for a in phase.hamming_tables(n_fft))
    return degrade.device_tables(("hamming", n_fft), device, build)


class STFTMagObserved(restore.WindowOperator):
    """Observation of x[B, L] through the STFT magnitude of phase.STFTMagnitude(win_size, hop_size, L) with state[1|B, L + Tw] (float32 on the
    GPU; Tw = 1 + L // hop, L is taken from the row length).  With kh the first L states, kf the rest, xin = 0 where kh is absent, x
    elsewhere, and M = |STFT(xin)| [F, Tw]:

        apply(x)       [B, L + F*Tw]: x where kh is known, 0 elsewhere  |  M[:, j] where kf[j] == 0, 0 elsewhere (frames contiguous)
        adjoint(g)     [B, L]: the VJP at the x_hat of the last apply on the current stream; with a = STFTMagnitude's VJP of the magnitude
                       part of g over the observed frames: 0 where kh is absent, a + g[:L] where known, a elsewhere

    The operator protocol of degrade.py over restore.WindowOperator (``rows(lo, hi)``; the tables and a shared state row stay shared; the
    x_hat per stream and the frame scratch per (B, stream)).  It declares NO ``matrix_obs``: the guidance norm is the element-wise norm over
    the whole row, not predict_pr's induced matrix norm of one segment's spectrogram (see the module docstring).  There is no
    data-consistency projection.  With every frame observed and no sample known or absent, the magnitude block of apply and the adjoint of
    [0 | g] give STFTMagnitude's bits."""

    def __init__(self, win_size: int, hop_size: int, state: torch.Tensor):
        self.N, self.hop = phase.check_sizes(win_size, hop_size)
        super().__init__(state, "[1|B, L + Tw]")
        q, m = divmod(state.shape[1] - 1, self.hop + 1)                  # L = q hop + m, m < hop  <=>  L + L // hop = q (hop + 1) + m
        self.L = q * self.hop + m
        if m == self.hop or self.L < 1:
            raise _lib.AidError(f"STFTMagObserved: a state row of {state.shape[1]} entries is no L + 1 + L // {self.hop} for any L >= 1")
        self.F, self.T = phase.observation_shape(self.N, self.hop, self.L)
        self.row = self.L + self.F * self.T
        self.window, self.twiddle = tables(self.N, state.device)

    def _slice(self, lo: int, hi: int) -> "STFTMagObserved":
        return STFTMagObserved(self.N, self.hop, self._state_rows(lo, hi))

    def project(self, x, y):
        raise AttributeError("STFTMagObserved: no data-consistency step exists for phase retrieval (the reference calls a "
                             "data_consistency_step_phase_retrieval it never defines): set tester.data_consistency.use = False")

    def _params(self, x, g, frames, out, mode):
        return _lib.StftMagObservedParams(x.data_ptr(), _lib.ptr(g), self.state.data_ptr(), self.window.data_ptr(), self.twiddle.data_ptr(),
                                          _lib.ptr(frames), out.data_ptr(), self.L, self.L, self.row, self._state_ld,
                                          out.shape[1], x.shape[0], self.N, self.hop, self.T, mode)

    def apply(self, x):
        """A(x): [B, L] -> [B, L + F*Tw]"""
        x = self._signal(x, self.L, ".apply")
        out = torch.empty((x.shape[0], self.row), dtype=torch.float32, device=x.device)
        _lib.call("aid_stft_mag_observed", self._params(x, None, None, out, 0))
        self._keep(x)
        return out

    def adjoint(self, g):
        """VJP of apply at the x_hat of the last apply on this stream: [B, L + F*Tw] -> [B, L]"""
        x = self._kept(g)
        g = self._signal(g, self.row, ".adjoint")
        B = g.shape[0]
        out = torch.empty((B, self.L), dtype=torch.float32, device=g.device)
        _lib.call("aid_stft_mag_observed", self._params(x, g, self._scratch(B, self.T, self.N, device=g.device), out, 1))
        return out


def pr_gather(rec: torch.Tensor, out: torch.Tensor, jobs: torch.Tensor, L: int, n_fft: int, hop: int):
    """One aid_pr_gather launch on the current stream -> (y [J, L + F*Tw], state [J, L + Tw]): the observations and the states of every
    job's window (``window_state``); known samples from ``out`` [R, N], observed magnitude columns from ``rec`` [R, F, T_rec] (any item and
    bin stride, unit stride along T), 0 elsewhere."""
    _lib._req(rec)
    restore._rows(out, "out")
    restore._table(jobs)
    n_fft, hop = phase.check_sizes(n_fft, hop)
    L, F = int(L), n_fft // 2 + 1
    if rec.dim() != 3 or (rec.stride(2) != 1 and rec.shape[2] > 1):
        raise _lib.AidError("rec must be [R, F, T_rec] with unit stride along T_rec")
    R, N = out.shape
    if rec.shape[0] != R or rec.shape[1] != F or L < 1 or N < 1 or rec.shape[2] != frames_of(N, hop):
        raise _lib.AidError(f"pr_gather: rec {tuple(rec.shape)} is no [R, {F}, {frames_of(N, hop)}] for out {tuple(out.shape)}, or L = {L} is below 1")
    J, Tw = jobs.shape[0], frames_of(L, hop)
    y = torch.empty((J, L + F * Tw), dtype=torch.float32, device=rec.device)
    k = torch.empty((J, L + Tw), dtype=torch.float32, device=rec.device)
    if J:
        _lib.call("aid_pr_gather", _lib.PrGatherParams(rec.data_ptr(), out.data_ptr(), y.data_ptr(), k.data_ptr(), jobs.data_ptr(),
                                                       L, N, rec.shape[2], rec.stride(0), rec.stride(1), out.stride(0), J, R, n_fft, hop, Tw))
    return y, k


def pr_prepare(args):
    """What the groups of a call share: (n_fft, hop), phase.check_sizes of win_size / hop_size where predict_pr reads them
    (sampler.phase_retrieval_sizes), judged before any spectrogram"""
    from .sampler import phase_retrieval_sizes
    return phase.check_sizes(*phase_retrieval_sizes(args))


def check_pr_args(y: torch.Tensor, length, sizes, L: int, end: int, max_batch: int, seeds):
    """The refusals of a phase retrieval of whole recordings after phase.check_sizes', all raised before anything is launched -> (n_fft, hop, N).
    What can be judged without a GPU is judged first; the device of y last."""
    n_fft, hop = sizes
    F = n_fft // 2 + 1
    if not (torch.is_tensor(y) and y.dtype == torch.float32 and y.dim() == 3 and y.shape[0] >= 1 and y.shape[1] == F and y.shape[2] >= 1):
        raise _lib.AidError(f"y must be float32 magnitude spectrograms [R, F = {F}, T_rec] (|STFT| with win_size {n_fft}, hop_size {hop}), "
                            f"got {tuple(y.shape) if torch.is_tensor(y) else type(y).__name__}")
    N = check_length(y.shape[2], length, hop)
    pr_windows(N, L, end, n_fft, hop)                                      # (end' in [1, L/2); end' >= 2 (n_fft - 1) with more than one window)
    restore.check_batch(y, max_batch, seeds, "phase retrieval of whole recordings")
    return n_fft, hop, N


def pr_group(y: torch.Tensor, checked, sizes, L: int, end: int) -> restore.Group:
    """The part of a phase retrieval that plans and builds: y [R, F, T_rec] magnitude spectrograms on the GPU (any strides; one copy
    unless T_rec has unit stride), (n_fft, hop, N) of check_pr_args -> restore.Group(out = zeros [R, N], (jobs_A, jobs_B) of pr_plan, the
    aid_pr_gather closure).  win_size and hop_size are shared by every group of a call (``pr_predict``); the states of a job travel in the
    gathered rows."""
    n_fft, hop, N = checked
    R, F, T_rec = y.shape
    if (T_rec > 1 and y.stride(2) != 1) or y.stride(1) < T_rec or y.stride(0) < (F - 1) * y.stride(1) + T_rec:
        y = y.contiguous()                                                   # (torch.stft hands out [R, F, T] with frames strided: one copy, before pass A)
    out = torch.zeros((R, N), dtype=torch.float32, device=y.device)          # (every sample is owned; pass B's heads and tails lie in ranges pass A owns)
    return restore.Group(out, pr_plan(R, N, L, end, n_fft, hop), lambda table: pr_gather(y, out, table, L, n_fft, hop))


def pr_predict(sampler, sizes, L: int, device):
    """predict(win, c0, c1) of a phase retrieval: ``sampler.predict_resample`` through STFTMagObserved over rows c0:c1 of the gathered (y, k)"""
    def predict(win, c0, c1):
        yw, kw = (t[c0:c1] for t in win)
        return sampler.predict_resample(yw, (c1 - c0, L), STFTMagObserved(*sizes, kw))
    return predict


restore.long_task(name="pr", method="predict_pr_long", what="restored", consistency="no data-consistency step exists for phase retrieval",
                  guided="the reference asserts xi > 0", entries=("length",), call_args={}, prepare=pr_prepare, check=check_pr_args, build=pr_group,
                  predict=pr_predict, step=lambda sizes, L, end: L - aligned_end(L, end, sizes[1]))


def pr_passes(sampler, y: torch.Tensor, win_size, hop_size, L: int, end: int, length=None, max_batch: int = 8,
              seeds: Optional[Sequence[int]] = None) -> torch.Tensor:
    """The two passes over ``sampler.predict_resample(yw [B, L + F*Tw], (B, L), STFTMagObserved(win_size, hop_size, kw [B, L + Tw])) -> [B, L]``
    with B <= max_batch: y [R, F, T_rec] magnitude spectrograms on the GPU (any strides; the gather reads them in place when T_rec has unit
    stride) -> restored [R, N].  Per pass: one aid_pr_gather launch, the sampler calls, one aid_window_scatter launch per call
    (restore.run_task, with the aligned step L - end').  Spectrograms and result stay on the GPU.  Seeds as restore.restore_passes."""
    return restore.run_task(restore.LONG_TASKS["pr"], sampler, phase.check_sizes(win_size, hop_size), [(y, length)], L, end, max_batch, seeds)[0]
