"""Native degradation operators of bandwidth extension and declipping on MI355X (include/aid_degrade.h).

The reference builds these degradations as torch lambdas (testing/edm_sampler.py:245-300, :359-385) and differentiates
through them with torch.autograd.  Here each one is an operator object of the ``stft.SpectralMask`` protocol --
``apply`` (A), ``adjoint`` (A^T), ``project(x, y)`` (y + x - A(x), where the reference's data_consistency_step is
defined, :47-54), ``shared_mask`` and ``__call__ = apply`` -- running on HIP kernels on the caller's stream:

  * ``FIRFilter(taps, L, stride=1, pad="same")``: conv1d(x[:, None], taps[1, 1, K], padding="same") (apply_FIR_filter, :245-251),
    or a strided correlation with symmetric integer padding;
  * ``Decimate(factor, L)``: x[..., 0:-1:factor] (:259-260);
  * ``IIRFilter(b, a, L, clamp=False)`` / ``IIRFilter.biquad(...)``: lfilter (:253-258), recursion in fp64;
  * ``HardClip(clip_value)``: clip(x, -c, c) (:366-368);
  * ``SincResample(orig_freq, new_freq, L)`` / ``SincResample.from_factor(factor, L)``: torchaudio.functional.resample with its default
    Hann-windowed sinc kernel (:262-264), [B, L] -> [B, ceil(new*L/orig)] (aid_resample_poly and, include/aid_resample_op.h, its adjoint).

None holds per-item data, so sub-batches on concurrent streams may share one (``shared_mask`` is True); per-call state
(the clip's x_hat, the IIR scratch) is keyed by the current stream.  Tables are built once on the host in float64 and
kept on the device.  GPU only; no fallback.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib

IIR_MAX_ORDER = 16
IIR_CHUNK = 256


def _check_signal(x, n, what):
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == n):
        raise _lib.AidError(f"{what}: expected a float32 GPU tensor [B, {n}], got "
                            f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
    return x.contiguous()


class _Operator:
    shared_mask = True          # no per-item data: sub-batches on concurrent streams may share the operator

    def project(self, x, y):
        raise AttributeError(f"{type(self).__name__}: the data-consistency step y + x - A(x) is undefined here (it needs a linear "
                             "operator that keeps the signal length): set tester.data_consistency.use = False")

    def __call__(self, x):
        return self.apply(x)


class FIRFilter(_Operator):
    """out[b, i] = sum_k taps[k] * x[b, i*stride + k - pad_left] (zero padding), i < L_out.  pad="same" (stride 1 only) is
    torch's conv1d padding="same": pad_left = (K-1)//2, L_out = L.  An integer pad pads both sides (conv1d padding=pad)."""

    def __init__(self, taps, audio_len: int, stride: int = 1, pad="same", device="cuda"):
        t = torch.as_tensor(taps).detach()
        if t.dim() == 0 or t.numel() != t.shape[-1] or t.numel() == 0:
            raise _lib.AidError(f"FIRFilter: taps must be [K], [1, K] or [1, 1, K], got {tuple(t.shape)}")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.AidError("FIRFilter runs on the GPU only (no CPU fallback)")
        self.taps = t.reshape(-1).to(dev, torch.float32).contiguous()
        self.K, self.L, self.stride = self.taps.numel(), int(audio_len), int(stride)
        if not 1 <= self.stride <= 16:
            raise _lib.AidError("FIRFilter: stride must be in [1, 16]")
        if self.stride > 1 and self.K > 4096:
            raise _lib.AidError("FIRFilter: strided filters take at most 4096 taps")
        if pad == "same":
            if self.stride != 1:
                raise _lib.AidError("FIRFilter: padding='same' needs stride 1 (as torch conv1d)")
            self.pad_left, self.L_out = (self.K - 1) // 2, self.L
        else:
            self.pad_left = int(pad)
            if self.pad_left < 0:
                raise _lib.AidError("FIRFilter: negative padding")
            self.L_out = (self.L + 2 * self.pad_left - self.K) // self.stride + 1
        if self.L_out < 1:
            raise _lib.AidError("FIRFilter: no output samples for this length / padding")

    def _run(self, x, adjoint, c0=1.0, add1=None, add2=None):
        n_in, n_out = (self.L_out, self.L) if adjoint else (self.L, self.L_out)
        x = _check_signal(x.reshape(x.shape[0], -1), n_in, type(self).__name__)
        out = torch.empty(x.shape[0], n_out, device=x.device, dtype=torch.float32)
        _lib.call("aid_fir", _lib.FirParams(x.data_ptr(), out.data_ptr(), self.taps.data_ptr(), _lib.ptr(add1), _lib.ptr(add2), float(c0),
                                            x.shape[0], self.K, self.stride, self.pad_left, int(adjoint), self.L, self.L_out, n_in, n_out))
        return out

    def apply(self, x):
        """A(x): [B, L] -> [B, L_out]"""
        return self._run(x, 0)

    def adjoint(self, g):
        """A^T(g): [B, L_out] -> [B, L]"""
        return self._run(g, 1)

    def project(self, x, y):
        """y + x - A(x)      (data_consistency_step, edm_sampler.py:47-54) -- linear filters that keep the length only"""
        if self.stride != 1 or self.L_out != self.L:
            return super().project(x, y)
        x = _check_signal(x, self.L, "FIRFilter.project")
        return self._run(x, 0, c0=-1.0, add1=_check_signal(y, self.L, "FIRFilter.project"), add2=x)


class Decimate(FIRFilter):
    """x[..., 0:-1:factor] (the reference's decimate, edm_sampler.py:259-260): L_out = ceil((L - 1) / factor)."""

    def __init__(self, factor: int, audio_len: int, device="cuda"):
        f = int(factor)
        if not 1 <= f <= 16 or int(audio_len) < 2:
            raise _lib.AidError("Decimate: factor must be in [1, 16] and the signal at least 2 samples long")
        super().__init__(torch.ones(1), audio_len, stride=f, pad=0, device=device)
        self.factor = f
        self.L_out = (self.L - 2) // f + 1

    def project(self, x, y):
        return _Operator.project(self, x, y)


def iir_coefficients(b, a):
    """(b, a) -> normalised float64 coefficient rows [N+1] as the kernels run them: rounded to float32 first (the reference's
    torch.Tensor(...), edm_sampler.py:281-290), divided by a[0] in float32, zero-padded to a common length.  Refuses a[0] == 0,
    orders above 16 and unstable filters -- stability is judged on these rounded coefficients, because they are what runs."""
    b32 = np.atleast_1d(np.asarray(b, dtype=np.float64).astype(np.float32)).reshape(-1)
    a32 = np.atleast_1d(np.asarray(a, dtype=np.float64).astype(np.float32)).reshape(-1)
    if b32.size == 0 or a32.size == 0:
        raise _lib.AidError("IIRFilter: empty coefficient list")
    if a32[0] == 0:
        raise _lib.AidError("IIRFilter: a[0] must not be 0")
    N = max(b32.size, a32.size, 2) - 1
    if N > IIR_MAX_ORDER:
        raise _lib.AidError(f"IIRFilter: order {N} above {IIR_MAX_ORDER}")
    bn = np.zeros(N + 1, np.float64)
    an = np.zeros(N + 1, np.float64)
    bn[:b32.size] = (b32 / a32[0]).astype(np.float32)
    an[:a32.size] = (a32 / a32[0]).astype(np.float32)
    an[0] = 1.0
    r = np.abs(np.roots(an)).max(initial=0.0) if np.any(an[1:]) else 0.0
    if not r < 1.0:
        raise _lib.AidError(f"IIRFilter: unstable filter after float32 rounding (largest pole |z| = {r:.4f} >= 1)")
    return bn, an


def iir_tables(a, C: int):
    """H[C, N] float64: H[m, j] = y[m] of the input-free recursion y[n] = -sum_k a[k] y[n-k] started from y[-1-i] = (i == j)."""
    N = a.size - 1
    Y = np.zeros((N + C, N), np.float64)
    Y[:N] = np.eye(N)[::-1]                    # rows 0..N-1 are y[-N] .. y[-1]
    for m in range(C):
        n = N + m
        Y[n] = -(a[1:, None] * Y[n - 1::-1][:N]).sum(axis=0)
    return Y[N:]


def iir_amplification(a, horizon: int = 8192) -> float:
    """Largest |y| of the input-free recursion started from a unit output state, over ``horizon`` samples.  The chunked recursion
    carries the state across chunks as last-N outputs; a rounding error of the carried state is amplified by up to this factor,
    and the state itself is a sum of terms this large, so the result is accurate to about 2^-53 * amplification^2."""
    return float(np.abs(iir_tables(a, horizon)).max())


IIR_MAX_REL_ERROR = 1e-7


class IIRFilter(_Operator):
    """lfilter(b, a) with zero initial state over L samples (scipy.signal.lfilter(b, a, x); torchaudio.functional.lfilter(x, a, b,
    clamp)), block-parallel over chunks of ``chunk`` samples, recursion in fp64.  clamp=True clamps the output to [-1, 1] after the
    recursion (torchaudio's clamp) and the adjoint takes the clamp's zero gradient outside [-1, 1].  The reference calls lfilter with
    clamp=False for "cheby1" (edm_sampler.py:253-255); its "biquad" goes through torchaudio.functional.biquad, which to our knowledge
    calls lfilter with the default clamp=True -- ``IIRFilter.biquad`` therefore defaults to clamp=True."""

    def __init__(self, b, a, audio_len: int, clamp: bool = False, chunk: int = IIR_CHUNK, device="cuda"):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.AidError("IIRFilter runs on the GPU only (no CPU fallback)")
        self.b, self.a = iir_coefficients(b, a)
        self.amplification = iir_amplification(self.a)
        if 2.0 ** -53 * self.amplification ** 2 > IIR_MAX_REL_ERROR:
            raise _lib.AidError(f"IIRFilter: the direct-form state of this filter is too ill-conditioned for the chunked recursion "
                                f"(amplification {self.amplification:.3g}: error ~{2.0 ** -53 * self.amplification ** 2:.1e} > "
                                f"{IIR_MAX_REL_ERROR:.0e}); use a lower order or a higher cut-off")
        self.N, self.C, self.L, self.clamp = self.b.size - 1, max(int(chunk), self.b.size - 1), int(audio_len), bool(clamp)
        self.L_out = self.L
        self.n_chunks = -(-self.L // self.C)
        self.coef = torch.from_numpy(np.concatenate([self.b, self.a])).to(dev)
        self.H = torch.from_numpy(np.ascontiguousarray(iir_tables(self.a, self.C))).to(dev)
        self._scratch, self._pre = {}, {}

    @classmethod
    def biquad(cls, b0, b1, b2, a0, a1, a2, audio_len: int, clamp: bool = True, device="cuda"):
        """torchaudio.functional.biquad(x, b0, b1, b2, a0, a1, a2) (edm_sampler.py:256-258)"""
        f = lambda v: float(torch.as_tensor(v, dtype=torch.float32).reshape(-1)[0])
        return cls([f(b0), f(b1), f(b2)], [f(a0), f(a1), f(a2)], audio_len, clamp=clamp, device=device)

    def _run(self, x, adjoint, c0=1.0, add1=None, add2=None):
        x = _check_signal(x.reshape(x.shape[0], -1), self.L, "IIRFilter")
        B = x.shape[0]
        stream = torch.cuda.current_stream().cuda_stream
        key = (B, stream)                               # (sub-batches on concurrent streams must not share the scratch)
        sc = self._scratch.get(key)
        if sc is None:
            sc = self._scratch[key] = (torch.empty(B, self.L, device=x.device, dtype=torch.float64),
                                       torch.empty(B, self.n_chunks, self.N, device=x.device, dtype=torch.float64))
        pre = None
        if self.clamp:
            if adjoint:
                pre = self._pre.get(stream)
                if pre is None or pre.shape[0] != B:
                    raise _lib.AidError("IIRFilter.adjoint with clamp needs the matching apply on this stream first")
            else:
                pre = self._pre[stream] = torch.empty(B, self.L, device=x.device, dtype=torch.float32)
        out = torch.empty_like(x)
        _lib.call("aid_iir", _lib.IirParams(x.data_ptr(), out.data_ptr(), _lib.ptr(pre), self.coef.data_ptr(), self.H.data_ptr(),
                                            sc[0].data_ptr(), sc[1].data_ptr(), _lib.ptr(add1), _lib.ptr(add2), float(c0),
                                            B, self.N, self.C, int(self.clamp), int(adjoint), self.L, self.L, self.L))
        return out

    def apply(self, x):
        """A(x) (clamped when clamp=True)"""
        return self._run(x, 0)

    def adjoint(self, g):
        """A^T(g): the recursion over reversed indices (J A J); with clamp the g of samples the forward clamped is dropped first"""
        return self._run(g, 1)

    def project(self, x, y):
        """y + x - A(x)      (data_consistency_step, edm_sampler.py:47-54) -- the unclamped (linear) filter only"""
        if self.clamp:
            return super().project(x, y)
        x = _check_signal(x, self.L, "IIRFilter.project")
        return self._run(x, 0, c0=-1.0, add1=_check_signal(y, self.L, "IIRFilter.project"), add2=x)


class HardClip(_Operator):
    """clip(x, -c, c) (SamplerDeclipping.apply_clip, edm_sampler.py:366-368); adjoint g * (-c <= x_hat <= c) at the x_hat of the
    last ``apply`` on the current stream (inclusive bounds, as torch.clamp's backward)."""

    def __init__(self, clip_value):
        self.clip = float(torch.as_tensor(clip_value, dtype=torch.float32).reshape(-1)[0]) if torch.is_tensor(clip_value) else float(np.float32(clip_value))
        if not self.clip >= 0:
            raise _lib.AidError("HardClip: the clip value must be >= 0")
        self._x = {}

    def _run(self, x, adjoint, xref=None):
        x = x.reshape(x.shape[0], -1)
        x = _check_signal(x, x.shape[1], "HardClip")
        out = torch.empty_like(x)
        _lib.call("aid_clip", _lib.ClipParams(x.data_ptr(), _lib.ptr(xref), out.data_ptr(), None, None, 1.0, self.clip,
                                              x.shape[0], int(adjoint), x.shape[1], x.shape[1], x.shape[1]))
        return out

    def apply(self, x):
        out = self._run(x, 0)
        self._x[torch.cuda.current_stream().cuda_stream] = x.reshape(x.shape[0], -1).contiguous()
        return out

    def adjoint(self, g):
        xref = self._x.get(torch.cuda.current_stream().cuda_stream)
        if xref is None or xref.numel() != g.numel():
            raise _lib.AidError("HardClip.adjoint needs the matching apply on this stream first")
        return self._run(g, 1, xref=xref)


# ---- the resampling degradation: torchaudio's default resampler and its adjoint -------------------------------------------------------
def sinc_kernel(orig: int, new: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """Hann-windowed sinc per output phase, [new, 2*width + orig] float64 -- torchaudio's default resampling kernel."""
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    idx = np.arange(-width, width + orig, dtype=np.float64)[None, :] / orig
    t = np.arange(0, -new, -1, dtype=np.float64)[:, None] / new + idx
    t = np.clip(t * base, -lowpass_filter_width, lowpass_filter_width)
    window = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    k = np.where(t == 0, 1.0, np.sin(t) / np.where(t == 0, 1.0, t)) * window * (base / orig)
    return k, width


def resample_host_tables(orig: int, new: int):
    """(k [new, K] float32 -- the table aid_resample_poly takes --, width, kT [K, new] float32 = k transposed, j_lo [K], j_hi [K] int32):
    [j_lo[t], j_hi[t]) is the tight range of phases outside which tap t of the float32 table is exactly 0.0f (the clamped Hann window;
    an all-zero tap gets the empty range [0, 0)), so the adjoint may skip every other term without changing its sum."""
    k64, width = sinc_kernel(orig, new)
    k = np.ascontiguousarray(k64, dtype=np.float32)
    kT = np.ascontiguousarray(k.T)
    nz = kT != 0
    any_nz = nz.any(axis=1)
    j_lo = np.where(any_nz, nz.argmax(axis=1), 0).astype(np.int32)
    j_hi = np.where(any_nz, new - nz[:, ::-1].argmax(axis=1), 0).astype(np.int32)
    return k, width, kT, j_lo, j_hi


_DEVICE_TABLES = {}


def device_tables(key, device, build):
    """``build(device)`` -> a tuple of tables on ``device``, made once per (key, device) and kept.  The upload is waited for, so that any
    stream may read the tables afterwards."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    tab = _DEVICE_TABLES.get((key, device))
    if tab is None:
        tab = build(device)
        if device.type == "cuda":
            torch.cuda.current_stream(device).synchronize()
        _DEVICE_TABLES[(key, device)] = tab
    return tab


def resample_tables(orig: int, new: int, device):
    """The device copies of resample_host_tables, built once per (ratio, device) and shared by harness.resample and SincResample:
    (k, width, kT, j_lo, j_hi)."""
    def build(device):
        k, width, kT, j_lo, j_hi = resample_host_tables(orig, new)
        return (torch.from_numpy(k).to(device), width) + tuple(torch.from_numpy(a).to(device) for a in (kT, j_lo, j_hi))
    return device_tables(("resample", orig, new), device, build)


def resample_poly(x, orig: int, new: int):
    """x [B, L] contiguous float32 on the GPU -> [B, ceil(new*L/orig)] (aid_resample_poly), orig / new already divided by their gcd"""
    k, width = resample_tables(orig, new, x.device)[:2]
    B, L = x.shape
    Lout = (new * L + orig - 1) // orig
    y = torch.empty(B, Lout, device=x.device, dtype=torch.float32)
    p = _lib.ResamplePolyParams(x.data_ptr(), y.data_ptr(), k.data_ptr(), x.stride(0), y.stride(0), L, Lout, B, orig, new, width, k.shape[1])
    _lib.call("aid_resample_poly", p)
    return y


def bwe_resample_ratio(factor):
    """(orig, new) of the reference's "resample" degradation for a bandwidth-extension factor: orig_freq = int(100 * factor), new_freq = 100
    (edm_sampler.py:262-264, truncation included: 1.15 -> 114:100), divided by their gcd."""
    try:
        f = float(factor)
    except (TypeError, ValueError):
        raise _lib.AidError(f"resample: the factor must be a number, got {factor!r}") from None
    if not 0 < f <= 16:
        raise _lib.AidError(f"resample: the factor must lie in (0, 16], got {factor!r}")
    o = int(100 * f)
    if o < 1:
        raise _lib.AidError(f"resample: int(100 * factor) = {o} for factor {factor!r}: no input rate")
    g = math.gcd(o, 100)
    return o // g, 100 // g


class SincResample(_Operator):
    """torchaudio.functional.resample(x, orig_freq, new_freq) with its default kernel (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99):
    y[b, i*new + j] = sum_t k[j][t] * x[b, i*orig + t - width], [B, L] -> [B, L_out = ceil(new*L/orig)] -- the reference's "resample"
    degradation of bandwidth extension (edm_sampler.py:262-264).  ``apply`` is harness.resample's launch on harness.resample's table;
    ``adjoint`` is the exact transpose (aid_resample_poly_adj).  Ratio 1:1 is the identity (torchaudio returns its input): no launch.
    The tables are built at the first launch; the object itself holds no device memory and no per-call state."""

    def __init__(self, orig_freq: int, new_freq: int, audio_len: int, device="cuda"):
        o, n = int(orig_freq), int(new_freq)
        if o < 1 or n < 1:
            raise _lib.AidError(f"SincResample: the frequencies must be >= 1, got {orig_freq!r} and {new_freq!r}")
        if int(audio_len) < 1:
            raise _lib.AidError(f"SincResample: the signal must hold at least 1 sample, got audio_len = {audio_len!r}")
        if torch.device(device).type != "cuda":
            raise _lib.AidError("SincResample runs on the GPU only (no CPU fallback)")
        g = math.gcd(o, n)
        self.orig, self.new, self.L = o // g, n // g, int(audio_len)
        self.L_out = (self.new * self.L + self.orig - 1) // self.orig
        self.identity = self.orig == self.new

    @classmethod
    def from_factor(cls, factor, audio_len: int, device="cuda"):
        """the operator of predict_bwe(ylpf, factor, "resample"): ratio bwe_resample_ratio(factor)"""
        return cls(*bwe_resample_ratio(factor), audio_len, device=device)

    def apply(self, x):
        """A(x): [B, L] -> [B, L_out]"""
        if self.identity:
            return x
        return resample_poly(_check_signal(x.reshape(x.shape[0], -1), self.L, "SincResample"), self.orig, self.new)

    def adjoint(self, g):
        """A^T(g): [B, L_out] -> [B, L]"""
        if self.identity:
            return g
        g = _check_signal(g.reshape(g.shape[0], -1), self.L_out, "SincResample.adjoint")
        k, width, kT, j_lo, j_hi = resample_tables(self.orig, self.new, g.device)
        gx = torch.empty(g.shape[0], self.L, device=g.device, dtype=torch.float32)
        _lib.call("aid_resample_poly_adj", _lib.ResamplePolyAdjParams(g.data_ptr(), gx.data_ptr(), kT.data_ptr(), j_lo.data_ptr(), j_hi.data_ptr(),
                                                                      g.stride(0), gx.stride(0), self.L, self.L_out, g.shape[0],
                                                                      self.orig, self.new, width, kT.shape[0]))
        return gx
