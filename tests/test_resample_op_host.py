"""CPU tests (no GPU) of the resampling degradation of bandwidth extension (include/aid_resample_op.h, degrade.SincResample,
Sampler.predict_bwe(..., "resample")): the ratio rule, the host tables and their support ranges, the adjoint gather over them
against autograd through the oracle's resampler, and the refusals."""
import math

import numpy as np
import pytest
import torch


RATIOS = [(2, 1), (5, 2), (3, 2), (57, 50), (1, 2), (147, 100), (160, 147), (320, 147)]
ADJOINT_CASES = [(2, 1, 37), (5, 2, 41), (147, 100, 300), (147, 100, 146), (3, 1, 2), (2, 1, 1)]


def test_bwe_resample_ratio_is_the_reference_rule():
    from audio_inpainting_diffusion_amd._lib import AidError
    from audio_inpainting_diffusion_amd.degrade import bwe_resample_ratio
    assert bwe_resample_ratio(2) == (2, 1)
    assert bwe_resample_ratio(2.5) == (5, 2)
    assert bwe_resample_ratio(1.47) == (147, 100)
    assert bwe_resample_ratio(1.15) == (57, 50)                 # int(100 * 1.15) = 114: the reference's truncation
    assert bwe_resample_ratio(1.5) == (3, 2)
    assert bwe_resample_ratio(1) == (1, 1) and bwe_resample_ratio(1.005) == (1, 1)
    assert bwe_resample_ratio(0.5) == (1, 2) and bwe_resample_ratio(16) == (16, 1)
    for bad in (0, -1, 16.5, float("nan"), float("inf"), 0.001, "fast", None):
        with pytest.raises(AidError):
            bwe_resample_ratio(bad)


@pytest.mark.parametrize("o,n", RATIOS)
def test_tables_are_the_harness_table_and_the_ranges_are_tight(o, n):
    from audio_inpainting_diffusion_amd import harness
    from audio_inpainting_diffusion_amd.degrade import resample_host_tables
    k, width, kT, j_lo, j_hi = resample_host_tables(o, n)
    k64, w2 = harness._sinc_kernel(o, n)
    K = 2 * width + o
    assert width == w2 and k.dtype == np.float32 and k.shape == (n, K) and np.array_equal(k, k64.astype(np.float32))
    assert kT.dtype == np.float32 and kT.shape == (K, n) and np.array_equal(kT, k.T) and kT.flags["C_CONTIGUOUS"]
    assert j_lo.dtype == np.int32 and j_hi.dtype == np.int32 and j_lo.shape == (K,) and j_hi.shape == (K,)
    terms = 0
    for t in range(K):
        lo, hi = int(j_lo[t]), int(j_hi[t])
        assert 0 <= lo <= hi <= n
        assert not kT[t, :lo].any() and not kT[t, hi:].any()                    # exactly 0.0f outside the range
        if hi > lo:
            assert kT[t, lo] != 0 and kT[t, hi - 1] != 0                        # the range ends are non-zero: tight
        else:
            assert (lo, hi) == (0, 0)
        terms += hi - lo
    print(f"{o}:{n}: K = {K}, {terms} of {K * n} table entries inside the ranges ({terms / o:.1f} terms per input sample)")
    assert terms >= np.count_nonzero(k)
    if (o, n) == (147, 100):
        assert terms / o < 20                                                   # (about 12 terms per input sample instead of K * n / o = 112)


def emulate_adjoint(g, o, n, L, kT, j_lo, j_hi, width):
    """numpy float64 transcription of resample_poly_adj_kernel (csrc/aid_resample_adj.hip) over the float32 table"""
    K, Lout = kT.shape[0], g.shape[1]
    kT = kT.astype(np.float64)
    gx = np.zeros((g.shape[0], L))
    i_last = (Lout - 1) // n
    for q in range(L):
        top = q + width
        num = top - (K - 1)
        i_lo = 0 if num <= 0 else (num + o - 1) // o
        for i in range(i_lo, min(top // o, i_last) + 1):
            t = top - i * o
            assert 0 <= t < K
            lo, hi = int(j_lo[t]), min(int(j_hi[t]), Lout - i * n)
            if hi > lo:
                gx[:, q] += g[:, i * n + lo:i * n + hi] @ kT[t, lo:hi]
    return gx


@pytest.mark.parametrize("o,n,L", ADJOINT_CASES)
def test_gather_over_the_ranges_is_the_adjoint_of_the_oracle_resampler(o, n, L):
    from audio_inpainting_diffusion_amd.degrade import resample_host_tables
    from oracle.resample import resample
    k, width, kT, j_lo, j_hi = resample_host_tables(o, n)
    gen = torch.Generator().manual_seed(o * 1000 + L)
    x = torch.randn(3, L, generator=gen, dtype=torch.float64).requires_grad_()
    y = resample(x, o, n)
    Lout = math.ceil(n * L / o)
    assert y.shape == (3, Lout)
    g = torch.randn(3, Lout, generator=gen, dtype=torch.float64)
    (ref,) = torch.autograd.grad(y, x, g)
    got = emulate_adjoint(g.numpy(), o, n, L, kT, j_lo, j_hi, width)
    err = float(np.linalg.norm(got - ref.numpy()) / np.linalg.norm(ref.numpy()))
    print(f"adjoint gather {o}:{n} L = {L}: rel-L2 vs autograd through the oracle = {err:.2e}")
    assert err <= 1e-6                                          # the project's bound for these operators; the table's float32 rounding is 6e-8


# ---- the operator's geometry and the refusals (all raised before anything touches a GPU) -----------------------------------------------
def test_operator_geometry_needs_no_gpu():
    from audio_inpainting_diffusion_amd.degrade import SincResample, _Operator
    op = SincResample(44100, 22050, 37)
    assert (op.orig, op.new, op.L, op.L_out, op.identity) == (2, 1, 37, 19, False) and op.shared_mask is True
    op = SincResample.from_factor(1.47, 300)
    assert (op.orig, op.new, op.L_out) == (147, 100, math.ceil(100 * 300 / 147))
    op = SincResample.from_factor(0.5, 100)
    assert (op.orig, op.new, op.L_out) == (1, 2, 200)
    op = SincResample.from_factor(1.005, 64)
    assert op.identity and op.L_out == 64
    x = torch.zeros(2, 64)
    assert op.apply(x) is x and op.adjoint(x) is x and op(x) is x       # ratio 1:1: the input itself, no launch
    assert SincResample.project is _Operator.project
    with pytest.raises(AttributeError, match="data-consistency"):
        op.project(x, x)


def test_constructor_refusals():
    from audio_inpainting_diffusion_amd._lib import AidError
    from audio_inpainting_diffusion_amd.degrade import SincResample
    for factor in (0, -2, 16.01, 0.001, float("nan")):
        with pytest.raises(AidError, match="factor"):
            SincResample.from_factor(factor, 1000)
    for audio_len in (0, -5):
        with pytest.raises(AidError, match="audio_len"):
            SincResample.from_factor(2, audio_len)
        with pytest.raises(AidError, match="audio_len"):
            SincResample(2, 1, audio_len)
    with pytest.raises(AidError, match="GPU only"):
        SincResample.from_factor(2, 1000, device="cpu")
    with pytest.raises(AidError, match="GPU only"):
        SincResample(2, 1, 1000, device=torch.device("cpu"))
    with pytest.raises(AidError, match="frequencies"):
        SincResample(0, 1, 1000)
    op = SincResample(2, 1, 1000)
    with pytest.raises(AidError, match=r"\[B, 1000\]"):                 # host tensors and wrong lengths never reach a launch
        op.apply(torch.zeros(1, 1000))
    with pytest.raises(AidError, match=r"\[B, 500\]"):
        op.adjoint(torch.zeros(1, 500))


def _stub_sampler(audio_len=2048):
    from audio_inpainting_diffusion_amd.config import make_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.sampler import Sampler
    args = make_args(audio_len=audio_len, T=2, xi=0.25)
    return Sampler(model=None, diff_params=EDM(args), args=args)


def test_predict_bwe_resample_refuses_host_tensors_first():
    """a CPU observation is refused whatever its shape and whatever the factor: the device check comes first"""
    from audio_inpainting_diffusion_amd._lib import AidError
    smp = _stub_sampler()
    for y, factor in ((torch.zeros(1, 1024), 2), (torch.zeros(1, 2048), 2), (torch.zeros(1, 7), 1.47), (torch.zeros(1, 1024), 99)):
        with pytest.raises(AidError, match="GPU only"):
            smp.predict_bwe(y, factor, "resample")
    assert smp.y is None and smp.spectral is None and smp.n_evals == 0


def test_predict_bwe_resample_refuses_a_wrong_observation_length_and_a_factor_out_of_range():
    """GPU observations that exist as shapes only (fake tensors: no device is touched): everything is refused before a launch, the
    wrong length with the expected shape in the message."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    from audio_inpainting_diffusion_amd._lib import AidError
    smp = _stub_sampler(2048)
    with FakeTensorMode():
        ys = {n: torch.empty(2, n, device="cuda") for n in (2048, 1023, 1025, 1394)}
        y3 = torch.empty(2, 1, 1024, device="cuda")
    for n in (2048, 1023, 1025):
        with pytest.raises(AidError, match=r"\[B, 1024\]"):
            smp.predict_bwe(ys[n], 2, "resample")
    with pytest.raises(AidError, match=r"\[B, 1024\]"):
        smp.predict_bwe(y3, 2, "resample")
    with pytest.raises(AidError, match=r"147:100.*\[B, 1394\]"):       # ceil(100 * 2048 / 147) = 1394
        smp.predict_bwe(ys[1023], 1.47, "resample")
    for factor in (0, 17, -1):
        with pytest.raises(AidError, match="factor"):
            smp.predict_bwe(ys[1394], factor, "resample")
    assert smp.y is None and smp.spectral is None and smp.n_evals == 0
