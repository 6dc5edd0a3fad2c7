"""aid_fft_pass (csrc/aid_fft.hip) at its edges: the radices 17, 19, 29 and 31, repeated odd primes (11025 = 3*3*5*5*7*7, 44100), one-pass
transforms (N = R, where the real / half-spectrum input and output modes meet in one launch: N = 2, 4, 16), N / R below one block of 256, odd N
(complex-to-complex only), unit impulses, the imaginary part of DC / Nyquist on the way into irfft, a real or half-spectrum end with a complex other
end (where alone a DC / Nyquist imaginary part that was not zeroed shows), a given ``out``, batch invariance and the refusals of the host checks.

The passes are driven the way ``CQTransform._fft`` drives them (the class over a stub plan, as tests/test_gpu_kernels.py does); the twiddle table is
computed in float64 and rounded to float32 as ``CQTPlan`` does.  References are numpy float64 on the CPU.

Bounds.  Whole tensor: rel-L2 < 2e-6, the project's figure for this kernel.  Per bin: the largest |error| of any bin over the RMS modulus of the
item's reference; the bound is made from the reference side alone: ``_fft32`` below evaluates the pass formula of include/aid_kernels.h in numpy
complex64 with the same float32 table, and the kernel's worst bin may be at most 4 x that evaluation's worst bin on the same input, with a floor of
1e-7 (the kernel may contract FMAs and sum in another order; a wrong operand is an error of order 1 in a bin, not a factor of four).  Every case
prints the kernel's error, the yardstick's error and their ratio (profiles/r23_spectral_front_end_edges.txt)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 123.0
PAD = 64
WHOLE_TOL = 2e-6
FACTOR, FLOOR = 4.0, 1e-7

C2C_ONE_PASS = [2, 3, 5, 16, 17, 19, 29, 31]
C2C_MULTI = [34, 323, 899, 646, 1798, 18734, 11025]       # [2,17] [17,19] [29,31] [2,17,19] [2,29,31] [2,17,19,29] [3,3,5,5,7,7]
REAL_N = [2, 4, 6, 16, 32, 512, 646, 1798, 22050, 44100]  # 2, 4, 16: one launch with in_mode and out_mode both real / half spectrum


@pytest.fixture(scope="module")
def L():
    from audio_inpainting_diffusion_amd import _lib
    _lib.lib()
    return _lib


def _table(N):
    """exp(-2 pi i m / N), float64 -> float32, [N, 2] (CQTPlan.twiddle_L)"""
    m = np.arange(N)
    return np.stack([np.cos(2 * np.pi * m / N), -np.sin(2 * np.pi * m / N)], axis=-1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _stub(N):
    """a CQTransform that owns nothing but the length-N FFT plan"""
    from audio_inpainting_diffusion_amd.cqt import CQTransform, fft_radices
    tr = CQTransform.__new__(CQTransform)
    tr.plan = SimpleNamespace(L=N, Lh=N // 2 + 1, radices=fft_radices(N))
    tr._dev = dict(device=torch.device(DEV, 0), twiddle_L=torch.from_numpy(_table(N).reshape(-1)).to(DEV))
    tr._tables = lambda device: tr._dev
    return tr


def _hermitian(Y, N):
    """[B, N/2+1] -> [B, N]: Hermitian extension with the imaginary part of DC and Nyquist dropped (what irfft is defined on)"""
    Y = Y.copy()
    Y[:, 0] = Y[:, 0].real
    if N % 2 == 0:
        Y[:, N // 2] = Y[:, N // 2].real
    idx = np.arange(N // 2 + 1, N)
    return np.concatenate([Y, np.conj(Y[:, N - idx])], axis=1)


def _fft32(x, N, sign, in_mode=0, out_mode=0, out_scale=1.0):
    """The pass formula of include/aid_kernels.h in numpy complex64 / float32 with the float32 table, one pass per radix of fft_radices(N):
         v[r] = in[j + r N/R] W_N^{r k N/(Ns R)}, k = j mod Ns;   out[(j/Ns) Ns R + k + q Ns] = sum_r v[r] W_R^{q r}   (r ascending)"""
    from audio_inpainting_diffusion_amd.cqt import fft_radices
    tw = _table(N)
    W = (tw[:, 0] + 1j * (tw[:, 1] * np.float32(-sign))).astype(np.complex64)
    if in_mode == 1:
        cur = x.astype(np.float32).astype(np.complex64)
    elif in_mode == 2:
        cur = _hermitian(x.astype(np.complex64), N).astype(np.complex64)
    else:
        cur = x.astype(np.complex64)
    B, Ns = cur.shape[0], 1
    for R in fft_radices(N):
        nb = N // R
        j = np.arange(nb)
        k = j % Ns
        tstep = N // (Ns * R)
        r = np.arange(R)[:, None]
        v = cur.reshape(B, R, nb)
        if Ns > 1:
            v = (v * W[(r * k[None, :]) * tstep][None]).astype(np.complex64)
        wr = W[np.arange(R) * nb]
        out = np.empty((B, N), dtype=np.complex64)
        for q in range(R):
            acc = v[:, 0].copy()
            for rr in range(1, R):
                acc = (acc + v[:, rr] * wr[(q * rr) % R]).astype(np.complex64)
            out[:, (j // Ns) * Ns * R + k + q * Ns] = acc
        cur, Ns = out, Ns * R
    if out_mode == 1:
        return (cur.real * np.float32(out_scale)).astype(np.float32)
    if out_mode == 2:
        return cur[:, : N // 2 + 1]
    return cur


def _bin_err(got, ref):
    """largest |error| of any bin over the RMS modulus of the item's reference; the worst item"""
    got, ref = np.asarray(got), np.asarray(ref)
    rms = np.sqrt(np.mean(np.abs(ref) ** 2, axis=-1))
    return float((np.abs(got - ref).max(axis=-1) / np.maximum(rms, 1e-300)).max())


def _as_t(a):
    a = np.asarray(a)
    return torch.view_as_real(torch.from_numpy(np.ascontiguousarray(a.astype(np.complex128)))) if np.iscomplexobj(a) else torch.from_numpy(a.astype(np.float64))


_worst = {}


def _check(tag, got, y32, ref):
    assert np.isfinite(np.asarray(got)).all(), f"{tag}: not finite (an element was not written)"
    e, e32 = rel_l2(_as_t(got), _as_t(ref)), rel_l2(_as_t(y32), _as_t(ref))
    b, b32 = _bin_err(got, ref), _bin_err(y32, ref)
    btol = max(FACTOR * b32, FLOOR)
    kind = tag.split()[0]
    if b32 > 0:
        _worst[kind] = max(_worst.get(kind, 0.0), b / b32)
    print(f"fft-edges {tag}: whole kernel {e:.2e} fp32-cpu {e32:.2e} ratio {e / max(e32, 1e-300):.2f} (bound {WHOLE_TOL:.1e}) | "
          f"worst bin kernel {b:.2e} fp32-cpu {b32:.2e} ratio {b / max(b32, 1e-300):.2f} (bound {btol:.1e}) "
          f"[largest bin ratio of '{kind}' so far {_worst.get(kind, 0.0):.2f}]")
    assert e < WHOLE_TOL, f"{tag}: whole-tensor rel-L2 {e:.3e} >= {WHOLE_TOL:.1e}"
    assert b <= btol, f"{tag}: worst bin {b:.3e} > {btol:.3e} (float32 CPU evaluation: {b32:.3e})"


def _noise(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32).numpy()


AMPL = np.array([1.0, 1j, 0.6 + 0.8j])       # unit modulus, one per item: every output bin of an impulse has modulus 1


@functools.lru_cache(maxsize=None)
def _c2c_inputs(N):
    """name -> [3, N] complex64: seeded white noise, a unit impulse at n = 1 and at n = N - 1 (a different unit-modulus amplitude per item)"""
    out = {"noise": (_noise(3, N, seed=N) + 1j * _noise(3, N, seed=N + 1)).astype(np.complex64)}
    for name, n0 in (("impulse@1", 1), ("impulse@N-1", N - 1)):
        x = np.zeros((3, N), dtype=np.complex64)
        x[:, n0] = AMPL
        out[name] = x
    return out


@functools.lru_cache(maxsize=None)
def _real_inputs(N):
    out = {"noise": _noise(3, N, seed=7 * N)}
    for name, n0 in (("impulse@1", 1), ("impulse@N-1", N - 1)):
        x = np.zeros((3, N), dtype=np.float32)
        x[:, n0] = (1.0, -1.0, 1.0)
        out[name] = x
    return out


def _c2c(tr, x, sign):
    """[B, N] complex64 -> [B, N] complex64 through aid_fft_pass, in_mode = out_mode = 0; the destination lies between sentinel bands"""
    B, N = x.shape
    src = torch.view_as_real(torch.from_numpy(np.ascontiguousarray(x))).to(DEV).contiguous()
    buf = torch.full((2 * PAD + B * N * 2,), SENT, device=DEV)
    out = buf[PAD:PAD + B * N * 2]
    out.fill_(float("nan"))
    tr._fft(src, B, 0, 0, float(sign), 1.0, out)
    torch.cuda.synchronize()
    assert bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + B * N * 2:] == SENT).all()), "aid_fft_pass wrote outside its output"
    return torch.view_as_complex(out.reshape(B, N, 2)).cpu().numpy()


@pytest.mark.parametrize("sign", [-1, 1], ids=["forward", "inverse"])
@pytest.mark.parametrize("N", C2C_ONE_PASS + C2C_MULTI)
def test_complex_transform(L, N, sign):
    """complex-to-complex, forward and unnormalised inverse, B = 3 and B = 1"""
    tr = _stub(N)
    for name, x in _c2c_inputs(N).items():
        x64 = x.astype(np.complex128)
        ref = np.fft.fft(x64, axis=-1) if sign < 0 else np.fft.ifft(x64, axis=-1) * N
        y32 = _fft32(x, N, sign)
        got = _c2c(tr, x, sign)
        _check(f"c2c N={N} {tr.plan.radices} sign={sign:+d} {name} B=3", got, y32, ref)
        if name != "noise":
            # an impulse: every bin has modulus 1, a wrong index is an error of order 1 in that bin
            assert np.abs(np.abs(got) - 1.0).max() < 1e-5
        got1 = _c2c(tr, x[:1], sign)
        assert np.array_equal(got1, got[:1]), f"N={N} {name}: item 0 of a batch of 3 differs from its B = 1 run"
        _check(f"c2c N={N} {tr.plan.radices} sign={sign:+d} {name} B=1", got1, y32[:1], ref[:1])


@pytest.mark.parametrize("N", REAL_N)
def test_rfft(L, N):
    tr = _stub(N)
    for name, x in _real_inputs(N).items():
        ref = np.fft.rfft(x.astype(np.float64), axis=-1)
        y32 = _fft32(x, N, -1, in_mode=1, out_mode=2)
        got = tr.rfft(torch.from_numpy(x).to(DEV)).cpu().numpy()
        _check(f"rfft N={N} {tr.plan.radices} {name} B=3", got, y32, ref)
        if name != "noise":
            assert np.abs(np.abs(got) - 1.0).max() < 1e-5
        for b in range(3):
            got1 = tr.rfft(torch.from_numpy(x[b:b + 1]).to(DEV)).cpu().numpy()
            assert np.array_equal(got1, got[b:b + 1]), f"N={N} {name}: item {b} of a batch of 3 differs from its B = 1 run"


@functools.lru_cache(maxsize=None)
def _spectra(N):
    """name -> [3, N/2+1] complex64.  noise: DC and Nyquist carry an imaginary part (irfft must ignore it); impulse: the spectrum of a unit impulse
    at n = 1 | N - 1 | 1, with an imaginary part ADDED to DC and Nyquist"""
    Lh = N // 2 + 1
    Y = (_noise(3, Lh, seed=11 * N) + 1j * _noise(3, Lh, seed=11 * N + 1)).astype(np.complex64)
    assert np.all(Y[:, 0].imag != 0) and np.all(Y[:, -1].imag != 0)
    k = np.arange(Lh)
    n0 = np.array([1, N - 1, 1])[:, None]
    Z = np.exp(-2j * np.pi * k[None, :] * n0 / N)
    Z[:, 0] += 0.75j
    Z[:, -1] -= 1.25j
    return {"noise": Y, "impulse": Z.astype(np.complex64)}


def _irfft_ref(Y, N):
    """from the definition: extend Hermitian-ly, zero the imaginary part of DC and Nyquist, real part of the float64 inverse DFT"""
    return np.fft.ifft(_hermitian(Y.astype(np.complex128), N), axis=-1).real


@pytest.mark.parametrize("N", REAL_N)
def test_irfft(L, N):
    tr = _stub(N)
    for name, Y in _spectra(N).items():
        ref = _irfft_ref(Y, N)
        y32 = _fft32(Y, N, +1, in_mode=2, out_mode=1, out_scale=1.0 / N)
        Yd = torch.from_numpy(Y).to(DEV)
        # B = 3 into a given contiguous ``out`` between sentinel bands
        buf = torch.full((2 * PAD + 3 * N,), SENT, device=DEV)
        out = buf[PAD:PAD + 3 * N].reshape(3, N)
        out.fill_(float("nan"))
        ret = tr.irfft(Yd, out=out)
        torch.cuda.synchronize()
        assert ret.data_ptr() == out.data_ptr()
        assert bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + 3 * N:] == SENT).all()), "irfft wrote outside ``out``"
        got = out.cpu().numpy()
        _check(f"irfft N={N} {tr.plan.radices} {name} B=3 out=given", got, y32, ref)
        # B = 1, no ``out``
        for b in range(3):
            got1 = tr.irfft(Yd[b:b + 1]).cpu().numpy()
            assert got1.shape == (1, N)
            assert np.array_equal(got1, got[b:b + 1]), f"N={N} {name}: item {b} of a batch of 3 differs from its B = 1 run"
        # the imaginary part of DC / Nyquist changes nothing, bit for bit
        Yz = Y.copy()
        Yz[:, 0] = Yz[:, 0].real
        Yz[:, -1] = Yz[:, -1].real
        assert np.array_equal(tr.irfft(torch.from_numpy(Yz).to(DEV)).cpu().numpy(), got), f"N={N} {name}: irfft depends on Im(DC) or Im(Nyquist)"


@pytest.mark.parametrize("N", REAL_N)
def test_real_round_trip(L, N):
    tr = _stub(N)
    x = _real_inputs(N)["noise"]
    got = tr.irfft(tr.rfft(torch.from_numpy(x).to(DEV))).cpu().numpy()
    y32 = _fft32(_fft32(x, N, -1, in_mode=1, out_mode=2), N, +1, in_mode=2, out_mode=1, out_scale=1.0 / N)
    _check(f"irfft(rfft) N={N} {tr.plan.radices} noise B=3", got, y32, x.astype(np.float64))


MIXED_N = [2, 16, 29, 646, 11025, 44100]
MODE_NAMES = {(2, 0): "half->complex", (1, 0): "real->complex", (0, 1): "complex->real", (0, 2): "complex->half"}
MIXED = [(N, m) for N in MIXED_N for m in MODE_NAMES if not (N % 2 and 2 in m)]      # a half spectrum of N/2+1 bins belongs to an even N


@pytest.mark.parametrize("N,modes", MIXED, ids=[f"{N}-{MODE_NAMES[m]}" for N, m in MIXED])
def test_mixed_modes(L, N, modes):
    """One real / half-spectrum end with a complex other end, which rfft and irfft never ask for.  half -> complex is where the zeroing of Im(DC) and
    Im(Nyquist) shows: the real part of an inverse transform does not depend on them, its imaginary part does."""
    in_mode, out_mode = modes
    tr = _stub(N)
    Lh = N // 2 + 1
    sign = +1 if in_mode == 2 or out_mode == 1 else -1
    scale = 1.0 / N if out_mode == 1 else 1.0
    if in_mode == 2:
        x = _spectra(N)["noise"]
        full = _hermitian(x.astype(np.complex128), N)
    elif in_mode == 1:
        x = _real_inputs(N)["noise"]
        full = x.astype(np.complex128)
    else:
        x = _c2c_inputs(N)["noise"]
        full = x.astype(np.complex128)
    ref = np.fft.fft(full, axis=-1) if sign < 0 else np.fft.ifft(full, axis=-1) * N
    ref = (ref.real * scale) if out_mode == 1 else ref[:, :Lh] if out_mode == 2 else ref
    y32 = _fft32(x, N, sign, in_mode=in_mode, out_mode=out_mode, out_scale=scale)
    xt = torch.from_numpy(np.ascontiguousarray(x))
    src = (torch.view_as_real(xt) if xt.is_complex() else xt).to(DEV).contiguous()
    n_out = 3 * N if out_mode == 1 else 3 * Lh * 2 if out_mode == 2 else 3 * N * 2
    buf = torch.full((2 * PAD + n_out,), SENT, device=DEV)
    out = buf[PAD:PAD + n_out]
    out.fill_(float("nan"))
    tr._fft(src, 3, in_mode, out_mode, float(sign), scale, out)
    torch.cuda.synchronize()
    assert bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + n_out:] == SENT).all()), "aid_fft_pass wrote outside its output"
    got = out.reshape(3, N).cpu().numpy() if out_mode == 1 else torch.view_as_complex(out.reshape(3, -1, 2)).cpu().numpy()
    _check(f"mixed N={N} {tr.plan.radices} in_mode={in_mode} out_mode={out_mode} noise B=3", got, y32, ref)
    if in_mode == 2:
        # a Hermitian input: the imaginary part of the output is rounding, whatever Im(DC) and Im(Nyquist) held
        assert np.abs(got.imag).max() <= max(FACTOR * np.abs(y32.imag).max(), FLOOR * np.sqrt(np.mean(np.abs(ref) ** 2)))


# ---------------------------------------------------------------------------------------------------------
# refusals: every argument below is rejected by a host check of aid_fft_pass, as read, before the radix switch (no launch)
REFUSED = {
    "B=0": dict(B=0), "B=65536": dict(B=65536),
    "in_mode=3": dict(in_mode=3), "in_mode=-1": dict(in_mode=-1), "out_mode=3": dict(out_mode=3), "out_mode=-1": dict(out_mode=-1),
    "in_mode=1 at Ns=2": dict(in_mode=1, R=2, Ns=2), "in_mode=2 at Ns=4": dict(in_mode=2, R=2, Ns=4),
    "out_mode=1 at Ns*R<N": dict(out_mode=1, R=2, Ns=1), "out_mode=2 at Ns*R<N": dict(out_mode=2, R=4, Ns=2),
    "sign=0": dict(sign=0.0), "sign=2": dict(sign=2.0), "sign=nan": dict(sign=float("nan")),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refusals(L, name):
    N = 16
    good = dict(B=1, N=N, R=16, Ns=1, in_mode=0, out_mode=0, sign=-1.0, out_scale=1.0)
    x = _c2c_inputs(N)["noise"][:1]
    src = torch.view_as_real(torch.from_numpy(np.ascontiguousarray(x))).to(DEV).contiguous()
    tw = torch.from_numpy(_table(N).reshape(-1)).to(DEV)
    dst = torch.full((4 * N * 2,), SENT, device=DEV)
    a = dict(good, **REFUSED[name])
    with pytest.raises(L.AidError):
        L.call("aid_fft_pass", L.FftPassParams(src.data_ptr(), dst.data_ptr(), tw.data_ptr(), a["B"], a["N"], a["R"], a["Ns"], a["in_mode"],
                                               a["out_mode"], a["sign"], a["out_scale"]))
    torch.cuda.synchronize()
    assert bool((dst == SENT).all()), f"{name}: the refused call wrote to its destination"
    a = good
    L.call("aid_fft_pass", L.FftPassParams(src.data_ptr(), dst.data_ptr(), tw.data_ptr(), a["B"], a["N"], a["R"], a["Ns"], a["in_mode"],
                                           a["out_mode"], a["sign"], a["out_scale"]))
    torch.cuda.synchronize()
    got = torch.view_as_complex(dst[:2 * N].reshape(1, N, 2)).cpu().numpy()
    assert rel_l2(_as_t(got), _as_t(np.fft.fft(x.astype(np.complex128), axis=-1))) < WHOLE_TOL
    assert bool((dst[2 * N:] == SENT).all())
