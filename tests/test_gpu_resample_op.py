"""GPU tests of the resampling degradation of bandwidth extension (csrc/aid_resample_adj.hip, degrade.SincResample,
Sampler.predict_bwe(..., "resample")): the operator against harness.resample and the oracle's restatement of torchaudio's
default resampler in float64, its adjoint against autograd through that oracle and bit-exactly on one-hot gradients, the
operator protocol, and the sampler against the generic lambda path and the CPU oracle sampler."""
import math

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = ([(2, 1, L, 3) for L in (1, 2, 37, 4096, 4097)] + [(5, 2, L, 3) for L in (41, 1000, 1003)] + [(3, 2, 1201, 3), (57, 50, 2000, 3), (1, 2, 100, 3)] +
         [(147, 100, L, 3) for L in (146, 147, 300, 4097)] + [(2, 1, 184184, 1), (147, 100, 184184, 1)])


def _gpu_resampler(o, n):
    """oracle.resample.resample restated for GPU tensors (its kernel is built on the CPU)"""
    from oracle.resample import sinc_resample_kernel
    k64, width = sinc_resample_kernel(o, n)

    def deg(x):
        k = k64.float().to(x.device)
        xp = torch.nn.functional.pad(x, (width, width + o))
        y = torch.nn.functional.conv1d(xp[:, None], k, stride=o).transpose(1, 2).reshape(x.shape[0], -1)
        return y[..., :math.ceil(n * x.shape[-1] / o)]
    return deg


@pytest.mark.parametrize("o,n,L,B", CASES)
def test_resample_forward_adjoint_and_dot_product(o, n, L, B):
    from audio_inpainting_diffusion_amd import harness
    from audio_inpainting_diffusion_amd.degrade import SincResample
    from oracle.resample import resample
    op = SincResample(o, n, L, device=DEV)
    Lout = math.ceil(n * L / o)
    assert op.L_out == Lout
    gen = torch.Generator().manual_seed(1000 * o + L)
    x, gy = torch.randn(B, L, generator=gen), torch.randn(B, Lout, generator=gen)
    xd = x.double().requires_grad_()
    ref = resample(xd, o, n)
    (adj,) = torch.autograd.grad(ref, xd, gy.double())
    ax = op.apply(x.to(DEV))
    assert tuple(ax.shape) == (B, Lout) and torch.equal(ax, harness.resample(x.to(DEV), o, n))
    assert torch.equal(op(x.to(DEV)), ax)
    ax = ax.cpu()
    atg = op.adjoint(gy.to(DEV)).cpu()
    assert tuple(atg.shape) == (B, L)
    e_fwd, e_adj = rel_l2(ax, ref.detach()), rel_l2(atg, adj)
    lhs, rhs = float((ax.double() * gy.double()).sum()), float((x.double() * atg.double()).sum())
    scale = float(ax.double().norm() * gy.double().norm())
    print(f"resample {o}:{n} L = {L}: apply {e_fwd:.2e}, adjoint {e_adj:.2e} vs the float64 oracle; "
          f"<Ax,g> - <x,A^T g> = {abs(lhs - rhs) / scale:.2e} of |Ax||g|")
    assert e_fwd <= 1e-6
    assert e_adj <= 1e-6
    assert abs(lhs - rhs) <= 1e-6 * scale


@pytest.mark.parametrize("o,n,L", [(2, 1, 37), (5, 2, 41), (147, 100, 300)])
def test_adjoint_of_a_one_hot_gradient_is_a_table_column_bit_for_bit(o, n, L):
    """adjoint(e_m)[q] = k[j][q + width - i*orig] for m = i*new + j, zero where that tap does not exist: every other term of the
    gather is an exact zero, so an off-by-one in a support range or at either border shows as a wrong bit."""
    from audio_inpainting_diffusion_amd.degrade import SincResample, resample_host_tables
    k, width, _, _, _ = resample_host_tables(o, n)
    K = k.shape[1]
    op = SincResample(o, n, L, device=DEV)
    Lout = op.L_out
    ms = sorted({0, n - 1, n, Lout - 1})
    assert all(0 <= m < Lout for m in ms)
    g = torch.zeros(len(ms), Lout)
    want = torch.zeros(len(ms), L)
    for r, m in enumerate(ms):
        g[r, m] = 1.0
        i, j = divmod(m, n)
        for q in range(L):
            t = q + width - i * o
            if 0 <= t < K:
                want[r, q] = float(k[j, t])
    assert bool((want != 0).any(dim=1).all())
    got = op.adjoint(g.to(DEV)).cpu()
    assert torch.equal(got, want)


def test_operator_protocol_identity_and_concurrent_streams():
    from audio_inpainting_diffusion_amd._lib import AidError
    from audio_inpainting_diffusion_amd.degrade import SincResample
    L = 3000
    op = SincResample.from_factor(1.47, L, device=DEV)
    assert op.shared_mask is True and (op.orig, op.new) == (147, 100)
    gen = torch.Generator().manual_seed(9)
    xd, gd = torch.randn(4, L, generator=gen).to(DEV), torch.randn(4, op.L_out, generator=gen).to(DEV)
    with pytest.raises(AttributeError):
        op.project(xd, xd)
    with pytest.raises(AidError):
        op.apply(xd[:, :-1])
    with pytest.raises(AidError):
        op.adjoint(gd[:, :-1])
    one = SincResample.from_factor(1.005, L, device=DEV)
    assert one.apply(xd) is xd and one.adjoint(xd) is xd                 # ratio 1:1: the input, no launch
    seq = [(op.apply(xd[:2]), op.adjoint(gd[:2])), (op.apply(xd[2:]), op.adjoint(gd[2:]))]
    assert torch.equal(torch.cat([s[0] for s in seq]), op.apply(xd)) and torch.equal(torch.cat([s[1] for s in seq]), op.adjoint(gd))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [None, None]
    cur = torch.cuda.current_stream()
    for s in streams:
        s.wait_stream(cur)
    with torch.cuda.stream(streams[0]):
        outs[0] = (op.apply(xd[:2]), op.adjoint(gd[:2]))
    with torch.cuda.stream(streams[1]):
        outs[1] = (op.apply(xd[2:]), op.adjoint(gd[2:]))
    for s in streams:
        cur.wait_stream(s)
    torch.cuda.synchronize()
    for a, b in zip(outs, seq):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- sampler ------------------------------------------------------------------------------------------------------------------
def test_predict_bwe_resample_refuses_a_wrong_observation_length():
    from test_gpu_generic import _sampler
    from audio_inpainting_diffusion_amd._lib import AidError
    smp = _sampler(2048, 3, 0.25, **{"data_consistency.use": False})
    for n in (2048, 1023, 1025):
        with pytest.raises(AidError, match=r"\[B, 1024\]"):
            smp.predict_bwe(torch.zeros(2, n, device=DEV), 2, "resample")
    assert smp.n_evals == 0


def test_toy_predict_bwe_resample_equals_predict_resample_with_the_reference_lambda():
    from test_gpu_generic import _sampler
    L = 2048
    deg = _gpu_resampler(2, 1)
    clean = torch.randn(2, L, generator=torch.Generator().manual_seed(1)) * 0.063
    y = deg(clean).to(DEV)
    assert tuple(y.shape) == (2, L // 2)
    outs = []
    for run in ("native", "lambda"):
        smp = _sampler(L, 3, 0.25, **{"data_consistency.use": False})
        smp.seeds = [3, 4]
        outs.append(smp.predict_bwe(y, 2, "resample") if run == "native" else smp.predict_resample(y, (2, L), deg))
    e = rel_l2(outs[0].cpu(), outs[1].cpu())
    print(f"toy predict_bwe resample vs predict_resample lambda: {e:.2e}")
    assert e <= 2e-5


@pytest.mark.parametrize("factor", [2, 1.47])
def test_hip_network_bwe_resample_vs_oracle(factor):
    from test_gpu_degrade import _small_net
    from audio_inpainting_diffusion_amd.degrade import bwe_resample_ratio
    from oracle.resample import resample
    smp, osmp, Ls, _ = _small_net()
    smp.args.exp.audio_len = Ls
    o, n = bwe_resample_ratio(factor)
    deg = lambda x: resample(x, o, n)
    clean = torch.stack([torch.randn(Ls, generator=torch.Generator().manual_seed(40 + i)) for i in range(2)]) * 0.063
    y = deg(clean)
    smp.seeds = [7, 8]
    out = smp.predict_bwe(y.to(DEV), factor, "resample")
    ref = osmp.predict_resample(y, (2, Ls), deg, seeds=[7, 8])
    e = rel_l2(out.cpu(), ref)
    print(f"HIP network, resample factor {factor} ({o}:{n}): rel-L2 vs oracle = {e:.2e}")
    assert e <= 5e-4


def test_predict_bwe_resample_batch_of_four_takes_the_sub_batch_streams():
    from test_gpu_degrade import _small_net
    from oracle.resample import resample
    smp, _, Ls, net = _small_net()
    smp.args.exp.audio_len = Ls
    clean = torch.stack([torch.randn(Ls, generator=torch.Generator().manual_seed(60 + i)) for i in range(4)]) * 0.063
    y = resample(clean, 147, 100).to(DEV)
    calls = []
    orig = net._split_plan
    net._split_plan = lambda B: calls.append(B) or orig(B)
    smp.seeds = [1, 2, 3, 4]
    out = smp.predict_bwe(y, 1.47, "resample")
    net._split_plan = orig
    assert 4 in calls
    for i in range(4):
        smp.seeds = [i + 1]
        one = smp.predict_bwe(y[i:i + 1].contiguous(), 1.47, "resample")
        e = rel_l2(out[i:i + 1].cpu(), one.cpu())
        print(f"batch of 4, item {i} vs its B = 1 run: {e:.2e}")
        assert e <= 5e-6, (i, e)
