"""Objective restoration metrics: log-spectral distance, SNR and SI-SDR of an estimate against a reference, over the samples and the band a
restoration is judged on (include/aid_phase_long.h: aid_stft_logspec_dist; include/aid_bwe_long.h: aid_eval_sums; csrc/aid_eval.hip).

THE FRAMES are those of phase.STFTMagnitude and blind.py: n_fft zeros appended, center=False, T = 1 + N // hop frames, a periodic Hann
window, unnormalised one-sided spectra R (reference) and E (estimate) of F = n_fft / 2 + 1 bins.

THE REGION is a row of weights per recording, non-zero = evaluate here (0 or non-zero, not fractional); None = every sample.  A frame is
COUNTED when it holds at least one sample q < N with a non-zero weight; without a region that is every frame with t * hop < N (the trailing
frame at t = N / hop when hop divides N holds appended zeros only).

THE METRICS, per recording:
    lsd_frames[t] = sqrt( 1/(k_hi - k_lo + 1) * sum_{k = k_lo .. k_hi} (log10(|R_k|^2 + floor) - log10(|E_k|^2 + floor))^2 )   counted t; -1 else
    lsd           = the mean of lsd_frames over the counted frames                                   (nan when no frame is counted)
    snr_db        = 10 log10( sum r^2 / sum (r - e)^2 )                                              over the samples of the region
    si_sdr_db     = 10 log10( (sum r e)^2 / (sum r^2 sum e^2 - (sum r e)^2) )                         (invariant to the scale of e)
    max_abs_err   = max |r - e|
A denominator <= 0 gives +inf; a region without a sample gives nan for the sample metrics and 0 for n_samples: an answer, not an error.

THE BAND (lo_hz, hi_hz) selects the bins whose centre frequency k * sample_rate / n_fft lies in [lo_hz, hi_hz]:
k_lo = ceil(lo_hz * n_fft / sample_rate), k_hi = floor(hi_hz * n_fft / sample_rate), in exact rational arithmetic.  None = all F bins.
A band that holds no bin centre is refused.  The band restricts lsd only; the sample metrics are time-domain and see every frequency.

``evaluate`` is two launches -- the frame distances, then the sums, which also add up the frames -- with no host round trip between them
and ONE read-back of [R, 8] doubles.  ``logspec_dist_host`` / ``eval_sums_host`` restate the two kernels in float64 numpy from the formulas
above: they are the definition the kernels are tested against; ``from_sums`` turns the eight sums into the metrics for both, and
``evaluate_host`` chains the three.  ``region_of`` names the region and band each restoration mode is judged on.  GPU only for
``evaluate``; no fallback.

Not covered: perceptual metrics (PEMO-Q / ODG, FAD: they need models), windows other than Hann, fractional weights.
"""
from __future__ import annotations

import ctypes
import math
from fractions import Fraction
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from . import blind
from . import degrade
from . import phase

N_FFT, HOP, FLOOR = 2048, 512, 1e-10
SUMS = ("n_samples", "sum_rr", "sum_ee", "sum_re", "sum_dd", "max_abs_err", "n_frames", "sum_lsd")     # the columns of aid_eval_sums
METRICS = ("lsd", "snr_db", "si_sdr_db", "max_abs_err")                                                # what a summary averages
TASKS = ("inpainting", "declipping", "bwe", "spectrogram_inpainting", "pr", "compsens")


# ---- settings and their refusals (no GPU needed) -------------------------------------------------------------------------------------------
def check_sizes(n_fft, hop) -> Tuple[int, int]:
    if isinstance(n_fft, bool) or int(n_fft) != n_fft or int(n_fft) & (int(n_fft) - 1) or not 16 <= int(n_fft) <= 8192:
        raise _lib.AidError(f"metrics: n_fft must be a power of two in [16, 8192], got {n_fft!r}")
    if isinstance(hop, bool) or int(hop) != hop or not 0 < int(hop) <= int(n_fft):
        raise _lib.AidError(f"metrics: hop must be in [1, n_fft], got {hop!r}")
    return int(n_fft), int(hop)


def band_bins(band, sample_rate, n_fft: int) -> Tuple[int, int]:
    """(k_lo, k_hi): the bins whose centre k * sample_rate / n_fft lies in [lo_hz, hi_hz]; None -> (0, n_fft / 2)"""
    if band is None:
        return 0, int(n_fft) // 2
    try:
        sample_rate = float(sample_rate)
        lo, hi = (float(v) for v in band)
    except (TypeError, ValueError):
        raise _lib.AidError(f"metrics: band must be (lo_hz, hi_hz) and sample_rate a number, got {band!r} and {sample_rate!r}") from None
    if not (math.isfinite(sample_rate) and sample_rate > 0):
        raise _lib.AidError(f"metrics: sample_rate must be a finite number above 0, got {sample_rate!r}")
    if not (math.isfinite(lo) and math.isfinite(hi)) or lo < 0 or hi > sample_rate / 2:
        raise _lib.AidError(f"metrics: band {(lo, hi)} must lie inside [0, sample_rate / 2] = [0, {sample_rate / 2}] Hz")
    if lo > hi:
        raise _lib.AidError(f"metrics: band {(lo, hi)} has lo_hz above hi_hz")
    k_lo = math.ceil(Fraction(lo) * int(n_fft) / Fraction(sample_rate))
    k_hi = math.floor(Fraction(hi) * int(n_fft) / Fraction(sample_rate))
    if k_lo > k_hi:
        raise _lib.AidError(f"metrics: band {(lo, hi)} Hz holds no bin centre at n_fft = {n_fft} and sample_rate = {sample_rate} "
                            f"(the bins are {sample_rate / n_fft:g} Hz apart)")
    return k_lo, k_hi


def _check_floor(floor) -> float:
    if not (isinstance(floor, (int, float)) and math.isfinite(floor) and floor >= 0):
        raise _lib.AidError(f"metrics: floor must be a finite number >= 0, got {floor!r}")
    return float(floor)


def _check_window(window) -> None:
    if window != "hann":
        raise _lib.AidError(f"metrics: the window is 'hann' (periodic); {window!r} is not built")


def region_of(task: str, **kw):
    """(region, band) a restoration mode is judged on; either may be None (every sample / every bin).
      "inpainting"              mask= [N] | [1, N] | [R, N], 1 = observed          ->  1 - mask, every bin
      "declipping"              y= the clipped recordings [R, N], clip_value= one level or one per recording
                                                                                    ->  |y| >= clip_value (per recording), every bin
      "bwe"                     cutoff_hz=, sample_rate=                            ->  every sample, the band (cutoff_hz, sample_rate / 2)
      "spectrogram_inpainting" / "pr" / "compsens"                                  ->  every sample, every bin
    Compositions ("bwe_declip") are out of scope."""
    def take(*names):
        if set(kw) != set(names):
            raise _lib.AidError(f"metrics.region_of({task!r}) takes {', '.join(n + '=' for n in names) or 'no keyword'}, got {sorted(kw)}")
        return [kw[n] for n in names]
    if task == "inpainting":
        mask, = take("mask")
        return 1.0 - torch.as_tensor(mask).to(torch.float32), None
    if task == "declipping":
        y, clip = take("y", "clip_value")
        y = torch.as_tensor(y)
        y = y.reshape(1, -1) if y.dim() == 1 else y
        c = torch.as_tensor(clip, dtype=y.dtype, device=y.device).reshape(-1)
        if y.dim() != 2 or c.numel() not in (1, y.shape[0]) or not bool((c > 0).all()):
            raise _lib.AidError(f"metrics.region_of('declipping'): y must be [R, N] and clip_value one level above 0 or one per recording, "
                                f"got {tuple(y.shape)} and {c.numel()} levels")
        return (y.abs() >= c.reshape(-1, 1)).to(torch.float32), None
    if task == "bwe":
        cutoff, fs = take("cutoff_hz", "sample_rate")
        return None, (float(cutoff), float(fs) / 2)
    if task in TASKS:
        take()
        return None, None
    raise _lib.AidError(f"metrics.region_of: task must be one of {TASKS}, got {task!r} (compositions such as 'bwe_declip' are out of scope)")


# ---- the float64 restatements ----------------------------------------------------------------------------------------------------------------
def _rows(a, what):
    a = np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float64)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    if a.ndim != 2 or a.shape[1] < 1:
        raise _lib.AidError(f"metrics: {what} must be [R, N] with N >= 1, got {a.shape}")
    return a


def _region_rows(region, R, N):
    if region is None:
        return None
    w = _rows(region, "region")
    if w.shape[1] != N or w.shape[0] not in (1, R):
        raise _lib.AidError(f"metrics: region must be [{N}], [1, {N}] or [{R}, {N}], got {w.shape}")
    return np.broadcast_to(w != 0, (R, N))


def counted_frames_host(region, R: int, N: int, n_fft: int, hop: int) -> np.ndarray:
    """[R, T] bool: frame t holds a sample q < N, t * hop <= q < t * hop + n_fft, with a non-zero weight (None: any sample)"""
    w = _region_rows(region, R, N)
    w = np.ones((R, N), dtype=bool) if w is None else w
    T = 1 + N // hop
    return np.stack([w[:, t * hop:t * hop + n_fft].any(axis=1) for t in range(T)], axis=1)


def logspec_dist_host(ref, est, region=None, *, n_fft: int = N_FFT, hop: int = HOP, k_lo: int = 0, k_hi: Optional[int] = None,
                      floor: float = FLOOR, dtype=np.float64) -> np.ndarray:
    """[R, T] float64: the frame distances of aid_stft_logspec_dist, -1 where the frame is not counted.  ``dtype`` = numpy.float32 runs the
    whole formula (window, FFT, powers, logarithms, sum) in single precision instead, through torch.stft: the yardstick that says how far
    an fp32 evaluation of these inputs may lie from the float64 one (tests/test_gpu_metrics.py)."""
    n_fft, hop = check_sizes(n_fft, hop)
    r, e = _rows(ref, "ref"), _rows(est, "est")
    if r.shape != e.shape:
        raise _lib.AidError(f"metrics: ref {r.shape} and est {e.shape} differ in shape")
    R, N = r.shape
    k_hi = n_fft // 2 if k_hi is None else int(k_hi)
    if not 0 <= int(k_lo) <= k_hi <= n_fft // 2:
        raise _lib.AidError(f"metrics: the band must hold 0 <= k_lo <= k_hi <= n_fft / 2, got ({k_lo}, {k_hi})")
    counted = counted_frames_host(region, R, N, n_fft, hop)
    T = counted.shape[1]
    if dtype == np.float32:
        def power(x):
            xe = torch.cat([torch.from_numpy(x).float(), torch.zeros(R, n_fft)], dim=1)
            X = torch.stft(xe, n_fft, hop, window=torch.hann_window(n_fft), center=False, return_complex=True)[:, k_lo:k_hi + 1, :T]
            return X.real ** 2 + X.imag ** 2                                                     # [R, bins, T] float32
        fl = torch.tensor(float(floor), dtype=torch.float32)
        d = torch.log10(power(r) + fl) - torch.log10(power(e) + fl)
        dist = torch.sqrt((d * d).mean(dim=1)).double().numpy()
    else:
        w = blind.hann_window(n_fft)

        def power(x):
            xe = np.concatenate([x, np.zeros((R, n_fft))], axis=1)
            fr = np.stack([xe[:, t * hop:t * hop + n_fft] for t in range(T)], axis=1) * w           # [R, T, n_fft]
            return np.abs(np.fft.rfft(fr, axis=2)[:, :, k_lo:k_hi + 1]) ** 2
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.log10(power(r) + floor) - np.log10(power(e) + floor)
            dist = np.sqrt((d * d).mean(axis=2))
    return np.where(counted, dist, -1.0)


def eval_sums_host(ref, est, region=None, frames=None) -> np.ndarray:
    """[R, 8] float64, the columns of ``SUMS``: the sums of aid_eval_sums over the samples with a non-zero weight, and over the frame
    distances ``frames`` [R, T] that are >= 0 (None: no frames)"""
    r, e = _rows(ref, "ref"), _rows(est, "est")
    if r.shape != e.shape:
        raise _lib.AidError(f"metrics: ref {r.shape} and est {e.shape} differ in shape")
    R, N = r.shape
    w = _region_rows(region, R, N)
    w = np.ones((R, N), dtype=bool) if w is None else w
    out = np.zeros((R, 8))
    for b in range(R):
        rb, eb = r[b][w[b]], e[b][w[b]]
        d = rb - eb
        out[b, :6] = rb.size, math.fsum(rb * rb), math.fsum(eb * eb), math.fsum(rb * eb), math.fsum(d * d), np.abs(d).max() if d.size else 0.0
        if frames is not None:
            f = np.asarray(frames, dtype=np.float64).reshape(R, -1)[b]
            out[b, 6:] = (f >= 0).sum(), math.fsum(f[f >= 0])
    return out


def from_sums(sums) -> dict:
    """[R, 8] float64 (numpy or torch, the columns of ``SUMS``) -> the dict of float64 torch tensors [R] that ``evaluate`` returns (without
    lsd_frames)"""
    s = torch.as_tensor(np.asarray(sums) if not torch.is_tensor(sums) else sums, dtype=torch.float64).cpu().reshape(-1, 8)
    n, rr, ee, re, dd, mx, nf, sf = s.unbind(1)
    nan, inf = torch.full_like(n, float("nan")), torch.full_like(n, float("inf"))

    def ratio_db(num, den):
        db = 10 * torch.log10(num / torch.where(den > 0, den, torch.ones_like(den)))
        return torch.where(n > 0, torch.where(den > 0, db, inf), nan)
    return {"lsd": torch.where(nf > 0, sf / torch.where(nf > 0, nf, torch.ones_like(nf)), nan),
            "snr_db": ratio_db(rr, dd), "si_sdr_db": ratio_db(re * re, rr * ee - re * re),
            "max_abs_err": torch.where(n > 0, mx, nan), "n_samples": n, "n_frames": nf}


def evaluate_host(ref, est, region=None, *, sample_rate, n_fft=N_FFT, hop=HOP, band=None, floor=FLOOR, window="hann") -> dict:
    """``evaluate`` restated in float64 on the CPU (any array-likes): the definition, not a fallback"""
    n_fft, hop = check_sizes(n_fft, hop)
    _check_window(window)
    k_lo, k_hi = band_bins(band, sample_rate, n_fft)
    frames = logspec_dist_host(ref, est, region, n_fft=n_fft, hop=hop, k_lo=k_lo, k_hi=k_hi, floor=_check_floor(floor))
    out = from_sums(eval_sums_host(ref, est, region, frames))
    out["lsd_frames"] = torch.from_numpy(frames)
    return out


# ---- the kernels -----------------------------------------------------------------------------------------------------------------------------
def tables(n_fft: int, device):
    """(periodic Hann window [n_fft], twiddle [n_fft/2, 2]) as float32 on ``device``, built once per (n_fft, device)"""
    def build(device):
        return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
                     for a in (blind.hann_window(n_fft), phase.hamming_tables(n_fft)[1]))
    return degrade.device_tables(("metrics", int(n_fft)), device, build)


def _signals(ref, est, region):
    for name, t in (("ref", ref), ("est", est)) + ((("region", region),) if region is not None else ()):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise _lib.AidError(f"metrics.evaluate: {name} must be a tensor on the GPU (no CPU fallback; evaluate_host restates it in float64)")
    if ref.dtype != torch.float32 or est.dtype != torch.float32:
        raise _lib.AidError(f"metrics.evaluate: ref and est must be float32, got {ref.dtype} and {est.dtype}")
    if ref.dim() != 2 or tuple(ref.shape) != tuple(est.shape) or ref.shape[0] < 1 or ref.shape[1] < 1:
        raise _lib.AidError(f"metrics.evaluate: ref and est must both be [R, N], got {tuple(ref.shape)} and {tuple(est.shape)}")
    if ref.device != est.device or (region is not None and region.device != ref.device):
        raise _lib.AidError("metrics.evaluate: ref, est and region must be on one device")
    R, N = ref.shape
    # (rows of a wider buffer are read in place; anything else is copied)
    rows = lambda t: t if (t.stride(1) == 1 or N == 1) and (t.shape[0] == 1 or t.stride(0) >= N) else t.contiguous()      # noqa: E731
    if region is not None:
        region = region.reshape(1, -1) if region.dim() == 1 else region
        if region.dim() != 2 or region.shape[1] != N or region.shape[0] not in (1, R):
            raise _lib.AidError(f"metrics.evaluate: region must be [{N}], [1, {N}] or [{R}, {N}], got {tuple(region.shape)}")
        region = rows(region if region.dtype == torch.float32 else (region != 0).to(torch.float32))
    return rows(ref), rows(est), region


def _ld(t) -> int:
    """the row stride the kernels are told: that of the tensor, or its row length when there is one row (whose stride may be anything)"""
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def logspec_dist(ref, est, region=None, *, n_fft=N_FFT, hop=HOP, k_lo=0, k_hi=None, floor=FLOOR, out=None):
    """One aid_stft_logspec_dist launch on the current stream: ref, est [R, N] (float32, GPU, unit stride along N), region None | [1, N] |
    [R, N] -> the frame distances [R, T] float32, -1 where the frame is not counted"""
    ref, est, region = _signals(ref, est, region)
    R, N = ref.shape
    T = 1 + N // int(hop)
    window, twiddle = tables(n_fft, ref.device)
    out = torch.empty((R, T), dtype=torch.float32, device=ref.device) if out is None else out
    band = (ctypes.c_float * 3)(float(k_lo), float(int(n_fft) // 2 if k_hi is None else k_hi), float(floor))     # (host memory: read by the launcher)
    state_ld = 0 if region is None or region.shape[0] == 1 else _ld(region)
    _lib.call("aid_stft_logspec_dist", _lib.StftMagObservedParams(
        est.data_ptr(), ref.data_ptr(), _lib.ptr(region), window.data_ptr(), twiddle.data_ptr(), ctypes.addressof(band), out.data_ptr(),
        N, _ld(est), _ld(ref), state_ld, _ld(out), R, int(n_fft), int(hop), T, 0))
    return out


def eval_sums(ref, est, region, frames, out=None):
    """One aid_eval_sums launch on the current stream: ref, est [R, N], region None | [1, N] | [R, N], frames [R, T] contiguous (an output of
    ``logspec_dist``) -> sums [R, 8] float64 on the GPU, the columns of ``SUMS``"""
    ref, est, region = _signals(ref, est, region)
    R, N = ref.shape
    if not (torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.float32 and frames.dim() == 2 and frames.shape[0] == R
            and frames.shape[1] >= 1 and frames.is_contiguous()):
        raise _lib.AidError(f"metrics.eval_sums: frames must be a contiguous float32 GPU tensor [{R}, T]")
    out = torch.empty((R, 8), dtype=torch.float64, device=ref.device) if out is None else out
    state_ld = 0 if region is None or region.shape[0] == 1 else _ld(region)
    _lib.call("aid_eval_sums", _lib.FirObservedParams(est.data_ptr(), ref.data_ptr(), _lib.ptr(region), frames.data_ptr(), out.data_ptr(),
                                                      R, frames.shape[1], 0, N, _ld(est), _ld(ref), state_ld, 8))
    return out


def evaluate(ref, est, region=None, *, sample_rate, n_fft=N_FFT, hop=HOP, band=None, floor=FLOOR, window="hann") -> dict:
    """ref, est [R, N] float32 on the GPU (any N >= 1), region None | [N] | [1, N] | [R, N] (non-zero = evaluate here), band None |
    (lo_hz, hi_hz) -> float64 tensors [R] on the CPU: lsd, snr_db, si_sdr_db, max_abs_err, n_samples, n_frames; and lsd_frames [R, T], the
    float32 frame distances as the kernel left them on the GPU (-1 = not counted).  Definitions and the band rule: the module docstring.
    Two launches on the current stream, one read-back of [R, 8] doubles."""
    n_fft, hop = check_sizes(n_fft, hop)
    _check_window(window)
    k_lo, k_hi = band_bins(band, sample_rate, n_fft)
    floor = _check_floor(floor)
    ref, est, region = _signals(ref, est, region)
    if ref.shape[0] * (1 + ref.shape[1] // hop) >= 2 ** 31:
        raise _lib.AidError(f"metrics.evaluate: {ref.shape[0]} recordings of {1 + ref.shape[1] // hop} frames are 2^31 frames or more: evaluate fewer at a time")
    frames = logspec_dist(ref, est, region, n_fft=n_fft, hop=hop, k_lo=k_lo, k_hi=k_hi, floor=floor)
    out = from_sums(eval_sums(ref, est, region, frames).cpu())
    out["lsd_frames"] = frames
    return out
