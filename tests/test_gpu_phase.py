"""GPU tests of phase retrieval (csrc/aid_phase.hip, phase.py, Sampler.predict_pr): the STFT-magnitude operator against fp64 torch.stft,
its VJP against fp64 autograd, the induced-matrix-norm seed against torch.linalg, and the sampler against the CPU oracle and the
reference's torch lambda."""
import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ref_stft_mag(x, N, hop):
    """SamplerPhaseRetrieval.apply_stft (testing/edm_sampler.py:315-320) in x's dtype"""
    x2 = torch.cat((x, torch.zeros(x.shape[0], N, dtype=x.dtype, device=x.device)), -1)
    X = torch.view_as_real(torch.stft(x2, N, hop_length=hop, window=torch.hamming_window(N, dtype=x.dtype, device=x.device), center=False,
                                      return_complex=True))
    return torch.sqrt(X[..., 0] ** 2 + X[..., 1] ** 2)


@pytest.mark.parametrize("N", [256, 1024, 2048])
@pytest.mark.parametrize("hop_div", [4, 2])
def test_stft_magnitude_forward_and_vjp_vs_fp64_torch(N, hop_div):
    from audio_inpainting_diffusion_amd.phase import STFTMagnitude
    hop = N // hop_div
    g = torch.Generator().manual_seed(N + hop)
    for L, B in ((8 * N, 1), (8 * N + 37, 3), (8 * N, 3), (8 * N + 37, 1)):
        x = torch.randn(B, L, generator=g) * 0.1
        op = STFTMagnitude(N, hop, L, device=DEV)
        xd = x.double().requires_grad_()
        ref = _ref_stft_mag(xd, N, hop)
        assert ref.shape == (B, op.F, op.T)
        if L % hop == 0:
            assert float(ref[:, :, -1].abs().max()) == 0.0                         # the all-zero last frame
        out = op.apply(x.to(DEV))
        e = rel_l2(out.cpu(), ref.detach())
        assert e <= 2e-6, (L, B, e)
        gy = torch.randn(ref.shape, generator=g)
        (adj,) = torch.autograd.grad(ref, xd, gy.double())
        assert torch.isfinite(adj).all()
        ea = rel_l2(op.adjoint(gy.to(DEV)).cpu(), adj)
        print(f"N={N} hop={hop} L={L} B={B}: forward {e:.2e}, VJP {ea:.2e}")
        assert ea <= 1e-5, (L, B, ea)


def _seed(den, y, order, max_iter=1000, tol=1e-6):
    from audio_inpainting_diffusion_amd import _lib
    den, y = den.to(DEV).float().contiguous(), y.to(DEV).float().contiguous()
    B, F, T = den.shape
    g, norm = torch.empty_like(den), torch.empty(B, device=DEV)
    r, diag = torch.empty_like(den), torch.empty(B, 2, device=DEV)
    _lib.call("aid_matrix_norm_seed", _lib.MatrixNormParams(den.data_ptr(), y.data_ptr(), g.data_ptr(), norm.data_ptr(), r.data_ptr(),
                                                            diag.data_ptr(), B, F, T, order, max_iter, tol))
    torch.cuda.synchronize()
    return norm.cpu(), g.cpu(), diag.cpu()


def test_matrix_norm_seed_ord1_vs_autograd_with_an_exact_tie():
    gen = torch.Generator().manual_seed(11)
    B, F, T = 3, 129, 40
    y, den = torch.randn(B, F, T, generator=gen), torch.randn(B, F, T, generator=gen)
    y[1, :, 7] = y[1, :, 30] = torch.randn(F, generator=gen) * 3          # item 1: two identical dominant columns -> an exact tie
    den[1, :, 7] = den[1, :, 30] = 0.0
    y[2, 5, :] = 0.0
    den[2, 5, :] = y[2, 5, :]                                              # item 2: a row of exact zeros (sign 0)
    d = den.double().requires_grad_()
    ref = torch.linalg.matrix_norm(y.double() - d, ord=1)
    (gref,) = torch.autograd.grad(ref.sum(), d)
    cs = (y.double() - den.double()).abs().sum(1)
    assert cs[1, 7] == cs[1, 30] == cs[1].max()
    norm, g, _ = _seed(den, y, 1)
    assert rel_l2(norm, ref.detach()) <= 1e-6
    assert torch.equal(g, gref.float())
    assert float(g[1, :, 7].abs().max()) == 0.5


def _planted(F, T, gap, seed):
    gen = torch.Generator().manual_seed(seed)
    U = torch.linalg.qr(torch.randn(F, F, generator=gen, dtype=torch.float64))[0]
    V = torch.linalg.qr(torch.randn(T, T, generator=gen, dtype=torch.float64))[0]
    k = min(F, T)
    s = torch.empty(k, dtype=torch.float64)
    s[0], s[1] = 1.0, 1.0 / gap
    s[2:] = (1.0 / gap) * torch.linspace(0.9, 0.01, k - 2, dtype=torch.float64)
    return (U[:, :k] * s) @ V[:, :k].T * 3.0


def _check_ord2(R, den, label):
    """R (fp32) = y - den; the seed against the fp64 SVD of the same fp32 matrix"""
    y = (R + den).float()
    Rf = (y - den.float()).double()                                        # what the seed sees after its fp32 subtraction
    Us, S, Vh = torch.linalg.svd(Rf)
    norm, g, diag = _seed(den, y, 2)
    uv = torch.einsum("bf,bt->bft", Us[..., 0], Vh[:, 0, :])
    es, eg = rel_l2(norm, S[:, 0]), rel_l2(-g, uv)
    print(f"{label}: sigma1/sigma2 = {[round(float(v), 3) for v in S[:, 0] / S[:, 1]]}, iterations {diag[:, 0].tolist()}, "
          f"residual {diag[:, 1].tolist()}, sigma rel {es:.2e}, u1v1^T rel-L2 {eg:.2e}")
    assert es <= 1e-5 and eg <= 1e-4
    assert (diag[:, 0] < 1000).all() and (diag[:, 1] <= 1e-6).all()


@pytest.mark.parametrize("gap", [1.05, 1.5, 10.0])
def test_matrix_norm_seed_ord2_planted_gaps_vs_fp64_svd(gap):
    F, T = 257, 300
    R = torch.stack([_planted(F, T, gap, 3), _planted(F, T, gap, 4)]).float()
    den = torch.randn(R.shape, generator=torch.Generator().manual_seed(5)).abs()
    _check_ord2(R, den, f"planted gap {gap}")


def _harmonic(L, B, seed, fs=22050):
    gen = torch.Generator().manual_seed(seed)
    t = torch.arange(L, dtype=torch.float64) / fs
    out = []
    for _ in range(B):
        f0 = 110.0 + 220.0 * float(torch.rand(1, generator=gen))
        out.append(sum((0.5 / k) * torch.sin(2 * np.pi * k * f0 * t + float(torch.rand(1, generator=gen)) * 6.28) for k in range(1, 9)))
    return (torch.stack(out) * 0.063).float()


def test_matrix_norm_seed_ord2_full_size_spectrogram_residual():
    L, N, hop = 184184, 1024, 256
    clean = _harmonic(L, 2, 1)
    est = clean + torch.randn(clean.shape, generator=torch.Generator().manual_seed(2)) * 0.02
    y, den = _ref_stft_mag(clean, N, hop), _ref_stft_mag(est, N, hop)
    assert y.shape == (2, 513, 720)
    _check_ord2(y - den, den, "513 x 720 spectrogram residual")


# ---- sampler ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [2, 1, "smoothl1"])
def test_hip_network_predict_pr_vs_oracle(norm):
    from test_gpu_degrade import _small_net
    smp, osmp, Ls, _ = _small_net()
    smp.args.tester.posterior_sampling.norm = osmp.norm = norm
    N, hop = smp.args.tester.phase_retrieval.win_size, smp.args.tester.phase_retrieval.hop_size
    clean = _harmonic(Ls, 2, 3)
    deg = lambda x: _ref_stft_mag(x, N, hop)                                            # noqa: E731
    y = deg(clean)
    smp.seeds = [7, 8]
    out = smp.predict_pr(y.to(DEV))
    ref = osmp.predict_resample(y, (2, Ls), deg, seeds=[7, 8])
    e = rel_l2(out.cpu(), ref)
    print(f"HIP network, predict_pr norm={norm}: rel-L2 vs oracle = {e:.2e}")
    assert e <= 5e-4


def test_predict_pr_batch_of_four_takes_the_sub_batch_streams():
    from test_gpu_degrade import _small_net
    smp, _, Ls, net = _small_net()
    N, hop = smp.args.tester.phase_retrieval.win_size, smp.args.tester.phase_retrieval.hop_size
    y = _ref_stft_mag(_harmonic(Ls, 4, 5), N, hop).to(DEV)
    calls = []
    orig = net._split_plan
    net._split_plan = lambda B: calls.append(B) or orig(B)
    smp.seeds = [1, 2, 3, 4]
    out = smp.predict_pr(y)
    net._split_plan = orig
    assert 4 in calls
    for i in range(4):
        smp.seeds = [i + 1]
        one = smp.predict_pr(y[i:i + 1].contiguous())
        e = rel_l2(out[i:i + 1].cpu(), one.cpu())
        assert e <= 5e-6, (i, e)


def test_get_score_with_stft_magnitude_and_data_consistency_raises():
    from test_gpu_degrade import _small_net
    from audio_inpainting_diffusion_amd.phase import STFTMagnitude
    smp, _, Ls, _ = _small_net(dc=True)
    op = STFTMagnitude(1024, 256, Ls, device=DEV)
    y = op.apply(_harmonic(Ls, 2, 6).to(DEV))
    x = torch.randn(2, Ls, generator=torch.Generator().manual_seed(1)).to(DEV)
    with pytest.raises(AttributeError):
        smp.get_score(x, y, torch.tensor(1.3), op)


def _full_size(norm):
    from audio_inpainting_diffusion_amd.config import make_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.init import seeded_init_
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    from audio_inpainting_diffusion_amd.sampler import Sampler
    args = make_args(audio_len=184184, T=2, xi=0.25)
    args.tester.data_consistency.use = False
    args.tester.posterior_sampling.norm = norm
    net = seeded_init_(Unet_CQT_oct_with_attention(args, torch.device(DEV)), 0)
    return Sampler(model=net, diff_params=EDM(args), args=args)


def test_full_size_predict_pr_smoothl1_vs_lambda():
    """configs[1] shape (B = 8, L = 184184), 2 Heun steps, norm "smoothl1": the native operator (sub-batch streams) against
    predict_resample through the reference's torch lambda (one stream), with the run's own fp64 sensitivity as the yardstick."""
    L, N, hop = 184184, 1024, 256
    smp = _full_size("smoothl1")
    y = _ref_stft_mag(_harmonic(L, 8, 7), N, hop).to(DEV)
    runs = {}
    for name, fn in (("native", None), ("lambda32", lambda x: _ref_stft_mag(x, N, hop)),
                     ("lambda64", lambda x: _ref_stft_mag(x.double(), N, hop).float())):
        smp.seeds = list(range(8))
        runs[name] = (smp.predict_pr(y) if fn is None else smp.predict_resample(y, (8, L), fn)).cpu()
    e = rel_l2(runs["native"], runs["lambda32"])
    sens = rel_l2(runs["lambda64"], runs["lambda32"])
    print(f"full size (8 x 184184, 2 steps) predict_pr smoothl1 vs lambda: {e:.2e}; the lambda in fp64 vs fp32: {sens:.2e}")
    assert torch.isfinite(runs["native"]).all()
    # the guided steps amplify fp32-level differences of the degradation: the native operator may differ from the fp32 lambda by
    # a few times what evaluating that same lambda in fp64 changes (floored at 1e-4, the order of what the sub-batch split alone moves
    # the full-size FIR run) and never by more than 2e-3, the bound of the full-size FIR test
    assert e <= min(2e-3, 5 * max(sens, 1e-4))


def test_full_size_predict_pr_norm2_converges():
    import audio_inpainting_diffusion_amd.sampler as sampler_mod
    from audio_inpainting_diffusion_amd.phase import STFTMagnitude
    L, N, hop = 184184, 1024, 256
    smp = _full_size(2)
    ops = []

    class _Recording(STFTMagnitude):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.diagnostics = []
            ops.append(self)
    y = _ref_stft_mag(_harmonic(L, 8, 8), N, hop).to(DEV)
    smp.seeds = list(range(8))
    orig = sampler_mod.STFTMagnitude
    sampler_mod.STFTMagnitude = _Recording
    try:
        out = smp.predict_pr(y)
    finally:
        sampler_mod.STFTMagnitude = orig
    assert torch.isfinite(out).all()
    diag = [d.cpu() for d in ops[0].diagnostics]
    assert sum(d.shape[0] for d in diag) == 8 * 3                          # 3 evaluations (Heun, T = 2) of 8 items, whatever the sub-batching
    it = torch.cat([d[:, 0] for d in diag])
    res = torch.cat([d[:, 1] for d in diag])
    print(f"full size norm 2: seed iterations per item and evaluation {it.int().tolist()}, max residual {float(res.max()):.2e}")
    assert (it < ops[0].seed_max_iter).all() and (res <= ops[0].seed_tol).all()
