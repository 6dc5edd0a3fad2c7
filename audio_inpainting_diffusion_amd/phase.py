"""STFT-magnitude operator of phase retrieval on MI355X (include/aid_phase.h).

``STFTMagnitude(win_size, hop_size, audio_len)`` is the degradation of the reference's ``SamplerPhaseRetrieval.apply_stft``
(testing/edm_sampler.py:308-335): append ``win_size`` zeros, ``torch.stft(..., window=torch.hamming_window(win_size),
center=False)`` (periodic Hamming, one-sided, unnormalised), magnitude.  x [B, L] -> |X| [B, F = N/2 + 1, T = 1 + L // hop].
It follows the ``stft.SpectralMask`` / ``degrade`` protocol: ``apply``, ``adjoint`` (the VJP at the x_hat of the last ``apply``
on the current stream, which the reference obtains from torch.autograd), ``shared_mask``, ``__call__ = apply`` and a
``project`` that raises (the reference calls a data_consistency_step_phase_retrieval it never defines).

Its observations are a matrix per item (``matrix_obs = (F, T)``), so the guidance norm ``torch.linalg.norm(..., dim=(1, 2),
ord=1 | 2)`` of the reference is the induced matrix norm; ``network._denoise_guided_one`` seeds it with
``aid_matrix_norm_seed`` (power iteration for ord 2, whose per-item iteration count and final residual land in
``diagnostics`` when that is a list).  GPU only; no fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .degrade import _Operator, _check_signal

SEED_TOL = 1e-6             # ord 2: stop when ||R^T u - sigma v|| / sigma <= SEED_TOL ...
SEED_MAX_ITER = 1000        # ... or after this many power iterations


def check_sizes(win_size, hop_size):
    """(N, hop) as ints; AidError unless N is a power of two in [16, 8192] and 0 < hop <= N (the kernels' limits)."""
    N, hop = int(win_size), int(hop_size)
    if N != win_size or hop != hop_size or N & (N - 1) or not 16 <= N <= 8192:
        raise _lib.AidError(f"phase retrieval: win_size must be a power of two in [16, 8192], got {win_size}")
    if not 0 < hop <= N:
        raise _lib.AidError(f"phase retrieval: hop_size must be in [1, win_size], got {hop_size}")
    return N, hop


def observation_shape(win_size, hop_size, audio_len):
    """(F, T) of |STFT| for a signal of audio_len samples"""
    N, hop = check_sizes(win_size, hop_size)
    return N // 2 + 1, 1 + int(audio_len) // hop


def hamming_tables(N: int):
    """(periodic Hamming window [N], twiddles (cos, -sin)(2 pi m / N) [N/2, 2]), built in float64, rounded to fp32 once by the caller"""
    n = np.arange(N)
    w = 0.54 - 0.46 * np.cos(2 * np.pi * n / N)                  # torch.hamming_window(N) (periodic=True, alpha 0.54, beta 0.46)
    m = np.arange(N // 2)
    tw = np.stack([np.cos(2 * np.pi * m / N), -np.sin(2 * np.pi * m / N)], axis=1)
    return w, tw


class STFTMagnitude(_Operator):
    def __init__(self, win_size: int, hop_size: int, audio_len: int, device="cuda"):
        self.N, self.hop = check_sizes(win_size, hop_size)
        self.L = int(audio_len)
        if self.L < 1:
            raise _lib.AidError("STFTMagnitude: empty signal")
        self.F, self.T = observation_shape(self.N, self.hop, self.L)
        self.matrix_obs = (self.F, self.T)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.AidError("STFTMagnitude runs on the GPU only (no CPU fallback)")
        w, tw = hamming_tables(self.N)
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        self.window, self.twiddle = f32(w), f32(tw)
        self.seed_tol, self.seed_max_iter = SEED_TOL, SEED_MAX_ITER
        self.diagnostics = None                                   # set to [] to collect the ord-2 seed's [B, 2] (iterations, residual) per call
        self._x, self._frames = {}, {}

    def project(self, x, y):
        raise AttributeError("STFTMagnitude: no data-consistency step exists for phase retrieval (the reference calls a "
                             "data_consistency_step_phase_retrieval it never defines): set tester.data_consistency.use = False")

    def _params(self, x, g, out, frames, adjoint):
        return _lib.StftMagParams(x.data_ptr(), _lib.ptr(g), out.data_ptr(), _lib.ptr(frames), self.window.data_ptr(), self.twiddle.data_ptr(),
                                  x.shape[0], self.N, self.hop, self.T, int(adjoint), self.L, self.L, self.L)

    def apply(self, x):
        """|STFT(x)|: [B, L] -> [B, F, T]"""
        x = _check_signal(x.reshape(x.shape[0], -1), self.L, "STFTMagnitude")
        out = torch.empty(x.shape[0], self.F, self.T, device=x.device, dtype=torch.float32)
        _lib.call("aid_stft_mag", self._params(x, None, out, None, 0))
        self._x[torch.cuda.current_stream().cuda_stream] = x
        return out

    def adjoint(self, g):
        """VJP of apply at the x_hat of the last apply on this stream: [B, F, T] -> [B, L]"""
        stream = torch.cuda.current_stream().cuda_stream
        x = self._x.get(stream)
        B = g.shape[0]
        if x is None or x.shape[0] != B:
            raise _lib.AidError("STFTMagnitude.adjoint needs the matching apply on this stream first")
        g = g.reshape(B, -1)
        if not (g.is_cuda and g.dtype == torch.float32 and g.shape[1] == self.F * self.T):
            raise _lib.AidError(f"STFTMagnitude.adjoint: expected a float32 GPU tensor [B, {self.F}, {self.T}]")
        g = g.contiguous()
        key = (B, stream)                                         # (sub-batches on concurrent streams must not share the frame scratch)
        fr = self._frames.get(key)
        if fr is None:
            fr = self._frames[key] = torch.empty(B, self.T, self.N, device=g.device, dtype=torch.float32)
        out = torch.empty(B, self.L, device=g.device, dtype=torch.float32)
        _lib.call("aid_stft_mag", self._params(x, g, out, fr, 1))
        return out
