"""Blind bandwidth extension: the low-pass that degraded a segment is not given, it is fitted to the current estimate inside every guided
evaluation (include/aid_phase.h: aid_stft_band_stats, aid_lowpass_fit; include/aid_bwe_long.h: aid_fir_observed_items).

THE MODEL.  y [B, L] is taken to be h * x with "same" padding (predict_bwe "firwin"), h an unknown zero-phase low-pass of ONE knee.  On the
F = n_fft / 2 + 1 bins of an n_fft-point STFT, with the cut-off c in bins (c > 0) and the slope A < 0 in dB per octave,

    H_dB(k; c, A) = max(floor_dB, min(0, A log2(k / c)))  for k > c,   0 for k <= c;        H = 10^(H_dB / 20).

THE STATISTICS use the framing of phase.STFTMagnitude (n_fft zeros appended, center=False, T = 1 + L // hop frames) with a periodic Hann
window:  Sxx[k] = sum_t |X[k, t]|^2,  Sxy[k] = sum_t |X[k, t]| |Y[k, t]|,  X the STFT of the current x_hat; |Y| is computed once per call.

THE COST.  g[k] = clamp(Sxy[k] / Sxx[k], 10^(floor_dB / 20), 1); a bin is valid when k >= k_lo, Sxx[k] > 0 and Sxx[k] >= eps max_k Sxx[k];
cost(c, A) = mean over the valid bins of (H(k; c, A) - g[k])^2, in the LINEAR gain domain (in dB the leakage floor of the stop band decides
the fit and the knee lands an octave low); 0 without a valid bin.  THE SEARCH is exhaustive over two tables, cut-offs c_j and slopes A_i; the
lowest cost wins and ties go to the lowest j, then the lowest i.  Nothing is carried from one evaluation to the next.

THE TAPS.  Frequency sampling on the same grid: K odd, K <= n_fft - 1, P = (K - 1) / 2, N = n_fft, w a K-point Hamming window,

    h[n] = w[n] / N * (H_0 + 2 sum_{k=1}^{N/2-1} H_k cos(2 pi k (n - P) / N) + H_{N/2} cos(pi (n - P))).

THE GUIDANCE.  A(x_hat)_b = h_b * x_hat_b with the taps just fitted for item b; in the VJP the taps are constants (stop-gradient), so
``adjoint`` is the adjoint FIR with the same taps.  Guidance only: a projection onto the consistent set of an ESTIMATED filter is not a
projection onto the data.

``band_stats_host`` / ``fit_host`` / ``design_taps_host`` restate the three steps in float64 numpy: they are the definition the kernels are
tested against.  ``BlindLowpass`` is the operator (restore.WindowOperator's protocol); ``Sampler.predict_blind_bwe`` drives it.  GPU only for
the operator; no fallback.

Whole recordings, one filter per recording pooled over several of its windows: blind_long.py (``Sampler.predict_blind_bwe_long``).
Not covered: more than one knee, IIR or decimating models.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from . import degrade
from . import phase
from . import restore

MAX_N_FFT = 2048                                     # aid_lowpass_fit keeps five fp64 tables of F entries in static LDS
N_FFT, HOP, K_TAPS = 1024, 256, 501                  # the defaults, chosen at audio_len 184184 (fs 22050: 21.5 Hz bins, 720 frames)
FLOOR_DB, EPS, K_LO = -80.0, 1e-10, 2
N_SLOPES = 25


class Settings(NamedTuple):
    n_fft: int
    hop: int
    K: int
    floor_dB: float
    k_lo: int
    eps: float
    cutoffs: np.ndarray                              # [NC] float32, bins
    slopes: np.ndarray                               # [NA] float32, dB per octave

    @property
    def F(self) -> int:
        return self.n_fft // 2 + 1


def default_cutoffs(n_fft: int, k_lo: int = K_LO) -> np.ndarray:
    """every half bin from k_lo to F - 1 = n_fft / 2"""
    return np.arange(2 * int(k_lo), int(n_fft) + 1, dtype=np.float64) / 2


def default_slopes() -> np.ndarray:
    """25 slopes -6 * 2^(i/4) dB per octave: -6 ... -384"""
    return -6.0 * 2.0 ** (np.arange(N_SLOPES, dtype=np.float64) / 4)


def make_settings(n_fft=N_FFT, hop=HOP, K=K_TAPS, floor_dB=FLOOR_DB, k_lo=K_LO, eps=EPS, cutoffs=None, slopes=None) -> Settings:
    """The settings after every refusal that needs no GPU.  The grids are rounded to float32 here, once: the kernel and the host restatement
    read the same candidates."""
    if isinstance(n_fft, bool) or int(n_fft) != n_fft or int(n_fft) & (int(n_fft) - 1) or not 16 <= int(n_fft) <= MAX_N_FFT:
        raise _lib.AidError(f"blind bandwidth extension: n_fft must be a power of two in [16, {MAX_N_FFT}], got {n_fft!r}")
    n_fft = int(n_fft)
    if int(hop) != hop or not 0 < int(hop) <= n_fft:
        raise _lib.AidError(f"blind bandwidth extension: hop must be in [1, n_fft], got {hop!r}")
    if int(K) != K or int(K) < 1 or int(K) % 2 == 0:
        raise _lib.AidError(f"blind bandwidth extension: K = {K!r} taps must be odd (a zero-phase filter)")
    if int(K) >= n_fft:
        raise _lib.AidError(f"blind bandwidth extension: K = {K} taps must be at most n_fft - 1 = {n_fft - 1} (frequency sampling on the n_fft grid)")
    if int(k_lo) != k_lo or not 0 <= int(k_lo) <= n_fft // 2:
        raise _lib.AidError(f"blind bandwidth extension: k_lo must be a bin in [0, {n_fft // 2}], got {k_lo!r}")
    if not float(floor_dB) < 0.0 or not np.isfinite(float(floor_dB)):
        raise _lib.AidError(f"blind bandwidth extension: floor_dB must be a finite number below 0, got {floor_dB!r}")
    if not 0.0 <= float(eps) < 1.0:
        raise _lib.AidError(f"blind bandwidth extension: eps must be in [0, 1), got {eps!r}")
    cut = np.asarray(default_cutoffs(n_fft, k_lo) if cutoffs is None else cutoffs, dtype=np.float64).reshape(-1).astype(np.float32)
    slo = np.asarray(default_slopes() if slopes is None else slopes, dtype=np.float64).reshape(-1).astype(np.float32)
    if cut.size == 0 or slo.size == 0:
        raise _lib.AidError("blind bandwidth extension: the cut-off grid and the slope grid must hold at least one candidate each")
    if cut.size * slo.size >= 2 ** 31:
        raise _lib.AidError("blind bandwidth extension: more than 2^31 - 1 candidate pairs")
    if not (np.all(np.isfinite(cut)) and np.all(cut > 0)):
        raise _lib.AidError("blind bandwidth extension: every cut-off candidate must be a finite number of bins above 0")
    if not (np.all(np.isfinite(slo)) and np.all(slo < 0)):
        raise _lib.AidError("blind bandwidth extension: every slope candidate must be a finite number of dB per octave below 0 (a low-pass falls)")
    return Settings(n_fft, int(hop), int(K), float(floor_dB), int(k_lo), float(eps), cut, slo)


def settings_of(args) -> Settings:
    """args.tester.blind_bwe when the config has it (any of n_fft, hop, K, floor_dB, k_lo, eps, cutoffs, slopes), the module defaults for the rest"""
    node = getattr(getattr(args, "tester", None), "blind_bwe", None)
    names = ("n_fft", "hop", "K", "floor_dB", "k_lo", "eps", "cutoffs", "slopes")
    kw = {} if node is None else {k: node[k] for k in names if k in node and node[k] is not None}
    return make_settings(**kw)


# ---- the float64 restatements ---------------------------------------------------------------------------------------------------------
def hann_window(n_fft: int) -> np.ndarray:
    """periodic Hann (torch.hann_window(n_fft)), float64"""
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(int(n_fft)) / int(n_fft))


def tap_window(K: int) -> np.ndarray:
    """symmetric K-point Hamming (numpy.hamming), float64"""
    return np.hamming(int(K)).astype(np.float64)


def stft_mag_host(x, n_fft: int, hop: int, window=None) -> np.ndarray:
    """|STFT| [B, F, T] in float64 with aid_stft_mag's framing: n_fft zeros appended, center=False, T = 1 + L // hop"""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    w = hann_window(n_fft) if window is None else np.asarray(window, dtype=np.float64)
    B, L = x.shape
    T = 1 + L // hop
    xe = np.concatenate([x, np.zeros((B, n_fft))], axis=1)
    frames = np.stack([xe[:, t * hop:t * hop + n_fft] for t in range(T)], axis=1) * w            # [B, T, n_fft]
    return np.abs(np.fft.rfft(frames, axis=2)).transpose(0, 2, 1)


def band_stats_host(x_hat, y_mag, n_fft: int, hop: int, window=None) -> np.ndarray:
    """[B, 2, F] float64: Sxx = sum_t |X|^2, Sxy = sum_t |X| |Y| for x_hat [B, L] and |Y| [B, F, T]"""
    X = stft_mag_host(x_hat, n_fft, hop, window)
    Y = np.asarray(y_mag, dtype=np.float64).reshape(X.shape)
    return np.stack([(X * X).sum(axis=2), (X * Y).sum(axis=2)], axis=1)


def gain_host(k, c: float, A: float, floor_dB: float) -> np.ndarray:
    """H(k; c, A) in float64"""
    k = np.asarray(k, dtype=np.float64)
    with np.errstate(divide="ignore"):
        dB = np.maximum(floor_dB, np.minimum(0.0, A * np.log2(np.maximum(k, 1e-300) / c)))
    return np.where(k > c, 10.0 ** (dB / 20), 1.0)


def valid_bins_host(stats_row, floor_dB: float = FLOOR_DB, eps: float = EPS, k_lo: int = K_LO):
    """(valid [F] bool, g [F] float64; g is 0 where the bin is not valid) of one item's stats [2, F]"""
    sxx, sxy = (np.asarray(s, dtype=np.float64) for s in stats_row)
    valid = (np.arange(sxx.size) >= k_lo) & (sxx > 0) & (sxx >= eps * sxx.max())
    g = np.zeros_like(sxx)
    g[valid] = np.clip(sxy[valid] / sxx[valid], 10.0 ** (floor_dB / 20), 1.0)
    return valid, g


def costs_host(stats_row, cutoffs, slopes, floor_dB: float = FLOOR_DB, eps: float = EPS, k_lo: int = K_LO) -> np.ndarray:
    """cost [NC, NA] float64 of every candidate pair for one item's stats [2, F]; all 0 without a valid bin"""
    valid, g = valid_bins_host(stats_row, floor_dB, eps, k_lo)
    cut, slo = np.asarray(cutoffs, dtype=np.float64).reshape(-1), np.asarray(slopes, dtype=np.float64).reshape(-1)
    out = np.zeros((cut.size, slo.size))
    k = np.nonzero(valid)[0].astype(np.float64)
    if k.size:
        with np.errstate(divide="ignore"):
            octaves = np.log2(np.maximum(k, 1e-300)[None, :] / cut[:, None])                        # [NC, valid bins]
        for i, A in enumerate(slo):
            H = np.where(k[None, :] > cut[:, None], 10.0 ** (np.maximum(floor_dB, np.minimum(0.0, A * octaves)) / 20), 1.0)
            out[:, i] = ((H - g[valid][None, :]) ** 2).mean(axis=1)
    return out


def fit_host(stats, cutoffs, slopes, floor_dB: float = FLOOR_DB, eps: float = EPS, k_lo: int = K_LO):
    """stats [B, 2, F] -> (fit [B, 4] float64: c, A, cost, number of valid bins;  index [B, 2] int: (j, i)).  The lowest cost wins; ties go to
    the lowest j, then the lowest i (numpy's argmin over the row-major [NC, NA] costs)."""
    stats = np.asarray(stats, dtype=np.float64)
    stats = stats[None] if stats.ndim == 2 else stats
    cut, slo = np.asarray(cutoffs, dtype=np.float64).reshape(-1), np.asarray(slopes, dtype=np.float64).reshape(-1)
    fit, index = np.zeros((stats.shape[0], 4)), np.zeros((stats.shape[0], 2), dtype=np.int64)
    for b, row in enumerate(stats):
        cost = costs_host(row, cut, slo, floor_dB, eps, k_lo)
        j, i = np.unravel_index(int(np.argmin(cost)), cost.shape)
        fit[b] = cut[j], slo[i], cost[j, i], valid_bins_host(row, floor_dB, eps, k_lo)[0].sum()
        index[b] = j, i
    return fit, index


def design_taps_host(c: float, A: float, n_fft: int, K: int, floor_dB: float = FLOOR_DB, window=None) -> np.ndarray:
    """taps [K] float64 of the one-knee low-pass (c, A) by frequency sampling on the n_fft grid under the tap window (Hamming by default)"""
    N, K = int(n_fft), int(K)
    w = tap_window(K) if window is None else np.asarray(window, dtype=np.float64)
    H = gain_host(np.arange(N // 2 + 1), c, A, floor_dB)
    d = np.arange(K) - (K - 1) // 2
    k = np.arange(1, N // 2)
    s = H[0] + 2.0 * (H[None, 1:N // 2] * np.cos(2 * np.pi * k[None, :] * d[:, None] / N)).sum(axis=1) + H[N // 2] * np.cos(np.pi * d)
    return w * s / N


# ---- the operator -----------------------------------------------------------------------------------------------------------------------
def tables(cfg: Settings, device):
    """(Hann window [n_fft], twiddle [n_fft/2, 2], candidates [NC + NA + 2] = cut-offs | slopes | floor_dB, k_lo, tap window [K]) as float32 on
    ``device``, built once per (settings, device)"""
    def build(device):
        w, tw = hann_window(cfg.n_fft), phase.hamming_tables(cfg.n_fft)[1]
        cand = np.concatenate([cfg.cutoffs, cfg.slopes, np.array([cfg.floor_dB, cfg.k_lo], dtype=np.float32)])
        return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device) for a in (w, tw, cand, tap_window(cfg.K)))
    key = ("blind", cfg.n_fft, cfg.K, cfg.floor_dB, cfg.k_lo, cfg.cutoffs.tobytes(), cfg.slopes.tobytes())
    return degrade.device_tables(key, device, build)


def band_stats(x_hat, y_mag, cfg: Settings, out=None, scratch=None):
    """One aid_stft_band_stats launch on the current stream: x_hat [B, L], |Y| [B, F, T] (contiguous, float32, GPU) -> stats [B, 2, F]"""
    _lib._req(x_hat)
    _lib._req(y_mag)
    B, L = x_hat.shape
    F, T = cfg.F, 1 + L // cfg.hop
    if x_hat.dim() != 2 or x_hat.stride(1) != 1 or tuple(y_mag.shape) != (B, F, T) or not y_mag.is_contiguous():
        raise _lib.AidError(f"band_stats: x_hat must be [B, L] with contiguous rows and |Y| contiguous [B, {F}, {T}], got {tuple(x_hat.shape)} and {tuple(y_mag.shape)}")
    window, twiddle, _, _ = tables(cfg, x_hat.device)
    out = torch.empty((B, 2, F), dtype=torch.float32, device=x_hat.device) if out is None else out
    scratch = torch.empty((B, T, 2, F), dtype=torch.float32, device=x_hat.device) if scratch is None else scratch
    _lib.call("aid_stft_band_stats", _lib.StftMagParams(x_hat.data_ptr(), y_mag.data_ptr(), out.data_ptr(), scratch.data_ptr(), window.data_ptr(),
                                                        twiddle.data_ptr(), B, cfg.n_fft, cfg.hop, T, 0, L, x_hat.stride(0), L))
    return out


def lowpass_fit(stats, cfg: Settings, fit=None, taps=None):
    """One aid_lowpass_fit launch on the current stream: stats [B, 2, F] -> (fit [B, 4] = c, A, cost, valid bins;  taps [B, K])"""
    _lib._req(stats)
    B = stats.shape[0]
    if tuple(stats.shape) != (B, 2, cfg.F) or not stats.is_contiguous() or B < 1:
        raise _lib.AidError(f"lowpass_fit: stats must be contiguous [B, 2, {cfg.F}], got {tuple(stats.shape)}")
    _, _, cand, wtap = tables(cfg, stats.device)
    fit = torch.empty((B, 4), dtype=torch.float32, device=stats.device) if fit is None else fit
    taps = torch.empty((B, cfg.K), dtype=torch.float32, device=stats.device) if taps is None else taps
    _lib.call("aid_lowpass_fit", _lib.MatrixNormParams(stats.data_ptr(), cand.data_ptr(), taps.data_ptr(), fit.data_ptr(), wtap.data_ptr(), None,
                                                       B, cfg.F, cfg.cutoffs.size, cfg.slopes.size, cfg.K, cfg.eps))
    return fit, taps


def stft_mag(y, cfg: Settings):
    """|Y| [B, F, T] of y [B, L] by aid_stft_mag under the Hann window of the statistics"""
    _lib._req(y)
    y = y.contiguous()
    B, L = y.shape
    T = 1 + L // cfg.hop
    window, twiddle, _, _ = tables(cfg, y.device)
    out = torch.empty((B, cfg.F, T), dtype=torch.float32, device=y.device)
    _lib.call("aid_stft_mag", _lib.StftMagParams(y.data_ptr(), None, out.data_ptr(), None, window.data_ptr(), twiddle.data_ptr(),
                                                 B, cfg.n_fft, cfg.hop, T, 0, L, L, L))
    return out


class BlindLowpass(restore.WindowOperator):
    """A(x_hat)_b = taps_b * x_hat_b ("same" correlation, as degrade.FIRFilter), the taps of item b fitted to x_hat_b and the observation y_b
    in ``apply``: three launches -- aid_stft_band_stats, aid_lowpass_fit, aid_fir_observed_items -- and no host round trip.  ``adjoint`` is one
    launch, the adjoint FIR with the taps the last ``apply`` left (constants in the VJP).  After an apply ``taps`` [B, K] and ``fit`` [B, 4]
    (cut-off in bins, slope in dB per octave, cost, valid bins) hold what it found.

    ``frozen=True`` skips statistics and fit and filters with the taps it was given (``taps`` [B, K] or one row [K] for every item): for
    callers who know a filter per item, and for tests -- with equal rows it is degrade.FIRFilter bit for bit.
    ``log``: set to [] to record (taps.clone(), fit.clone()) per apply (per sub-batch when the network splits the batch).

    The operator protocol of degrade.py over restore.WindowOperator: ``shared_mask`` False, ``rows(lo, hi)`` hands out views of taps, fit, |Y|
    and stats, so sub-batches run on concurrent streams; scratch is kept per (B, stream).  There is no projection."""

    def __init__(self, y: torch.Tensor, cfg: Optional[Settings] = None, taps=None, frozen: bool = False):
        cfg = make_settings() if cfg is None else cfg
        if not (torch.is_tensor(y) and y.is_cuda and y.dtype == torch.float32 and y.dim() == 2 and y.shape[0] >= 1 and y.shape[1] >= 1):
            raise _lib.AidError("BlindLowpass: y must be a float32 GPU tensor [B, L] (no CPU fallback)")
        B, L = y.shape
        dev = y.device
        if frozen:
            if taps is None:
                raise _lib.AidError("BlindLowpass: frozen=True needs the taps to filter with")
            held = frozen_rows(taps, B, cfg.K).to(dev).contiguous()
            y_mag = stats = None
        else:
            if taps is not None:
                raise _lib.AidError("BlindLowpass: taps are given with frozen=True only (the fit overwrites them otherwise)")
            held = torch.zeros((B, cfg.K), dtype=torch.float32, device=dev)
            y_mag = stft_mag(y, cfg)
            stats = torch.zeros((B, 2, cfg.F), dtype=torch.float32, device=dev)
        self._build(cfg, L, held, torch.zeros((B, 4), dtype=torch.float32, device=dev), y_mag, stats,
                    torch.zeros((1, L), dtype=torch.float32, device=dev), frozen, None)

    def _build(self, cfg, L, taps, fit, y_mag, stats, state, frozen, log):
        super().__init__(state, "[1, L]")                          # (every sample is filtered: one shared row of zeros)
        self.cfg, self.L, self.K = cfg, int(L), cfg.K
        self.taps, self.fit, self.y_mag, self.stats = taps, fit, y_mag, stats
        self.frozen, self.log = bool(frozen), log
        return self

    @property
    def items_held(self) -> int:
        return self.taps.shape[0]

    def _slice(self, lo: int, hi: int) -> "BlindLowpass":
        sub = object.__new__(BlindLowpass)
        rows = lambda t: None if t is None else t[lo:hi]
        return sub._build(self.cfg, self.L, self.taps[lo:hi], self.fit[lo:hi], rows(self.y_mag), rows(self.stats), self.state, self.frozen, self.log)

    def rows(self, lo: int, hi: int):
        sub = super().rows(lo, hi)
        sub.log = self.log                                         # (a log installed after the first split is still the one the parts write to)
        return sub

    def project(self, x, y):
        raise AttributeError("BlindLowpass: no data-consistency step (a projection onto the consistent set of an estimated filter is not a "
                             "projection onto the data): set tester.data_consistency.use = False")

    def _fir(self, mode, x):
        x = self._signal(x, self.L)
        out = torch.empty_like(x)
        L = self.L
        _lib.call("aid_fir_observed_items", _lib.FirObservedParams(x.data_ptr(), None, self.state.data_ptr(), self.taps.data_ptr(), out.data_ptr(),
                                                                    x.shape[0], self.K, mode, L, L, L, 0, L))
        return out

    def refit(self, x_hat):
        """statistics and fit of x_hat [B, L] into ``stats``, ``fit`` and ``taps`` (two launches)"""
        x_hat = self._signal(x_hat, self.L, ".refit")
        B, T = x_hat.shape[0], 1 + self.L // self.cfg.hop
        band_stats(x_hat, self.y_mag, self.cfg, out=self.stats, scratch=self._scratch(B, T, 2, self.cfg.F, device=x_hat.device))
        lowpass_fit(self.stats, self.cfg, fit=self.fit, taps=self.taps)

    def apply(self, x_hat):
        if not self.frozen:
            self.refit(x_hat)
        if self.log is not None:
            self.log.append((self.taps.clone(), self.fit.clone()))
        return self._fir(0, x_hat)

    def adjoint(self, g):
        return self._fir(1, g)


def frozen_rows(taps, B: int, K: int) -> torch.Tensor:
    """taps [B, K], or one row [K] / [1, K] for every item -> float32 [B, K] (on the device of ``taps``)"""
    t = torch.as_tensor(taps).detach().to(torch.float32)
    t = t.reshape(1, -1) if t.dim() == 1 else t
    if t.dim() != 2 or t.shape[1] != K or t.shape[0] not in (1, B):
        raise _lib.AidError(f"blind bandwidth extension: frozen taps must be [{B}, {K}] or one row [{K}] (K = the configured tap count), got {tuple(t.shape)}")
    return t.expand(B, K).contiguous()


def fit_in_hz(fit: torch.Tensor, cfg: Settings, fs: float) -> torch.Tensor:
    """fit [B, 4] -> [B, 2]: cut-off in Hz (bins * fs / n_fft) and slope in dB per octave"""
    return torch.stack([fit[:, 0] * (float(fs) / cfg.n_fft), fit[:, 1]], dim=1)
