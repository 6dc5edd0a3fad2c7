"""CPU tests (no GPU) of the restoration degradations (include/aid_degrade.h, audio_inpainting_diffusion_amd/degrade.py):
the three-pass chunked IIR decomposition driven by the host tables, and the refusals."""

import numpy as np
import pytest
import scipy.signal



def emulate_chunked_iir(b, a, x, C):
    """numpy float64 transcription of the three launches of aid_iir (csrc/aid_degrade.hip), driven by degrade.iir_tables."""
    from audio_inpainting_diffusion_amd.degrade import iir_tables
    N = a.size - 1
    H = iir_tables(a, C)
    L = x.size
    nC = -(-L // C)
    v = np.convolve(x, b)[:L]                                  # the FIR part reads the true input across chunk borders
    z = np.zeros(L)
    zend = np.zeros((nC, N))
    for c in range(nC):                                        # 1. zero-state recursion per chunk
        hist = np.zeros(N)                                     # hist[j] = z[n-1-j]
        for n in range(c * C, min(c * C + C, L)):
            zn = v[n] - a[1:] @ hist
            hist = np.concatenate(([zn], hist[:-1]))
            z[n] = zn
        zend[c] = hist
    state = np.zeros((nC, N))
    s = np.zeros(N)
    phi = H[C - 1 - np.arange(N)]                              # 2. carry scan: s_{c+1} = zend_c + Phi s_c
    for c in range(nC):
        state[c] = s
        s = zend[c] + phi @ s
    m = np.arange(L)                                           # 3. correction
    return z + np.einsum("ni,ni->n", H[m % C], state[m // C])


def _cases():
    out = []
    for fs in (22050, 44100):
        for fc in (1000, 4000):
            for order in (2, 4, 8):
                if (order, fc) == (8, 1000):
                    continue                                   # unstable after float32 rounding at 44.1 kHz, ill-conditioned at 22.05 kHz (refused, see below)
                out.append(("cheby1", order, fc, fs))
        out.append(("biquad", 2, 3000, fs))
    return out


@pytest.mark.parametrize("case", _cases())
@pytest.mark.parametrize("C", [256, 300])
def test_chunked_iir_decomposition_matches_scipy_lfilter(case, C):
    from audio_inpainting_diffusion_amd.degrade import iir_amplification, iir_coefficients
    kind, order, fc, fs = case
    if kind == "cheby1":
        b, a = scipy.signal.cheby1(order, 0.05, fc, fs=fs)
    else:
        b, a = scipy.signal.iirpeak(fc, 2.0, fs=fs)
        b, a = b * 1.7, a * 1.7                                 # a[0] != 1: exercises the normalisation
    bn, an = iir_coefficients(b, a)
    L = 3000                                                   # divisible by 300, not by 256
    x = np.random.default_rng(order + fc).standard_normal(L).astype(np.float32).astype(np.float64)
    ref = scipy.signal.lfilter(bn, an, x)
    y = emulate_chunked_iir(bn, an, x, C)
    # 1e-12 for well-conditioned filters; the carried last-N-outputs state of a high-order filter with clustered poles loses up to
    # 2^-53 * amplification^2 (measured: 2.7e-11 for order 4 at 1 kHz / 44.1 kHz, 4.4e-9 for order 8 at 4 kHz / 44.1 kHz)
    tol = max(1e-12, 4 * 2.0 ** -53 * iir_amplification(an) ** 2)
    err = np.linalg.norm(y - ref) / np.linalg.norm(ref)
    print(f"chunked IIR {case} C={C}: rel-L2 vs scipy.signal.lfilter = {err:.2e} (bound {tol:.1e})")
    assert err <= tol


def test_iir_coefficients_round_to_float32_before_normalising():
    from audio_inpainting_diffusion_amd.degrade import iir_coefficients
    b, a = scipy.signal.cheby1(4, 0.05, 4000, fs=22050)
    bn, an = iir_coefficients(b, a)
    assert np.array_equal(bn, b.astype(np.float32).astype(np.float64)) and np.array_equal(an, a.astype(np.float32).astype(np.float64))
    bn, an = iir_coefficients([1.0, 2.0], [3.0, 0.5])
    assert np.array_equal(an, np.array([1.0, np.float32(np.float32(0.5) / np.float32(3.0))]))


def test_iir_refuses_unstable_degenerate_and_high_order_filters():
    from audio_inpainting_diffusion_amd._lib import AidError
    from audio_inpainting_diffusion_amd.degrade import iir_coefficients
    b, a = scipy.signal.cheby1(8, 0.05, 1000, fs=44100)
    assert np.abs(np.roots(a)).max() < 1                       # stable in float64 ...
    with pytest.raises(AidError, match="unstable"):
        iir_coefficients(b, a)                                 # ... but not after float32 rounding
    iir_coefficients(*scipy.signal.cheby1(8, 0.05, 1000, fs=22050))   # stable after rounding (largest pole 0.990) ...
    from audio_inpainting_diffusion_amd.degrade import IIRFilter
    with pytest.raises(AidError, match="ill-conditioned"):              # ... but its direct-form state would lose ~1e-4 across chunks
        IIRFilter(*scipy.signal.cheby1(8, 0.05, 1000, fs=22050), audio_len=1000)
    with pytest.raises(AidError, match="unstable"):
        iir_coefficients([1.0], [1.0, -1.0])                   # pole on the unit circle
    with pytest.raises(AidError, match="a\\[0\\]"):
        iir_coefficients([1.0, 0.5], [0.0, 1.0])
    with pytest.raises(AidError, match="order"):
        iir_coefficients(np.ones(18), [1.0])


def test_predict_bwe_refuses_unknown_types_and_resample():
    import torch
    from audio_inpainting_diffusion_amd._lib import AidError
    from audio_inpainting_diffusion_amd.config import make_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.sampler import Sampler
    args = make_args(audio_len=2048, T=2, xi=0.25)
    smp = Sampler(model=None, diff_params=EDM(args), args=args)
    y = torch.zeros(1, 2048)
    with pytest.raises(AidError, match="resample.*not built"):
        smp.predict_bwe(y, 2, "resample")
    with pytest.raises(NotImplementedError):
        smp.predict_bwe(y, None, "no_such_filter")
