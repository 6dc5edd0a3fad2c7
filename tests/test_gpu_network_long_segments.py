"""The reduced network on segments whose attention levels are longer than 128 time steps, against the CPU oracle, in the manner (and with the
bounds) of tests/test_gpu_network.py, test_gpu_vjp.py and test_gpu_training.py.

 config X: 3 octaves of 8 bins, L = 4096, attention on levels 1, 2 and the bottleneck: level T = 512 / 256 / 128 -- one level on
           aid_time_attention_long, two blocks' worth on aid_time_attention (the plan test holds that split);
 config Y: the same with attention on every level and L = 8192: level T = 1024 / 512 / 256 -- every instance of the long kernels.
The oracle takes under half a second for either."""
import functools
import math

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
_BASE = dict(num_octs=3, bins_per_oct=8, Ns=(8, 8, 16), num_dils=(1, 2, 2), emb_dim=32)
CONFIGS = {"X": dict(_BASE, attention=(0, 1, 1, 1), audio_len=4096), "Y": dict(_BASE, attention=(1, 1, 1, 1), audio_len=8192)}
LEVEL_T = {"X": [512, 256, 128], "Y": [1024, 512, 256]}


def _setup(name, seed=3, **extra):
    from audio_inpainting_diffusion_amd.config import small_args
    from audio_inpainting_diffusion_amd.init import seeded_init_
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    from oracle.nsgt_cqt import OracleCQT
    from oracle.unet import OracleUnet
    kw = dict(CONFIGS[name], **extra)
    args = small_args(**kw)
    net = seeded_init_(Unet_CQT_oct_with_attention(args, torch.device(DEV)), seed, gate_scale=10.0, affine_scale=10.0)
    plan = net.CQTransform.plan
    assert [plan.T_oct[kw["num_octs"] - 1 - i] for i in range(kw["num_octs"])] == LEVEL_T[name]
    cqt = OracleCQT(kw["num_octs"], kw["bins_per_oct"], "oct", ("kaiser", 1), 22050, kw["audio_len"])
    orc = OracleUnet(kw["num_octs"], kw["bins_per_oct"], cqt).load_state_dict(net.state_dict())
    return net, orc, args, kw["audio_len"]


@functools.lru_cache(maxsize=None)
def _inputs(B, Ls):
    """x [B, Ls], cnoise [B, 1] (seeded, shared, never modified)"""
    from audio_inpainting_diffusion_amd.init import seeded_normal
    x = torch.from_numpy(seeded_normal(9, 0, B * Ls)).reshape(B, Ls) * 0.5
    cn = torch.linspace(-0.7, 0.1, B).reshape(B, 1)
    return x, cn


def _attention_ops(net, B):
    return [(o.name, int(o.params.T)) for o in net._state(B)["plan_body"].ops if o.name.startswith("aid_time_attention")]


@pytest.mark.parametrize("name", ["X", "Y"])
def test_forward_vs_oracle(name):
    net, orc, _, Ls = _setup(name)
    x, cn = _inputs(2, Ls)
    with torch.no_grad():
        y = net(x.to(DEV), cn.to(DEV))
        ref = orc(x, cn)
        y2 = net(x.to(DEV), cn.to(DEV))
    e = rel_l2(y.cpu(), ref)
    print(f"long segments, config {name}: forward rel-L2 vs oracle = {e:.3e}")
    assert e < TOL
    assert torch.equal(y, y2)                 # the launch plan replayed: the same bits


def test_plan_puts_the_long_kernel_on_the_long_blocks_only():
    net, _, _, Ls = _setup("X")
    x, cn = _inputs(2, Ls)
    with torch.no_grad():
        net(x.to(DEV), cn.to(DEV))
    ops = _attention_ops(net, 2)
    assert ops and all(nm in ("aid_time_attention", "aid_time_attention_long") for nm, _ in ops)
    assert {T for nm, T in ops if nm == "aid_time_attention_long"} == {256}
    assert {T for nm, T in ops if nm == "aid_time_attention"} == {128}
    n_long, n_old = sum(nm == "aid_time_attention_long" for nm, _ in ops), sum(nm == "aid_time_attention" for nm, _ in ops)
    assert n_long >= 1 and n_old >= 2                                      # level 2 and the bottleneck both run at T = 128
    # a configuration that ran before plans what it planned: no long op
    from test_gpu_network import _net_from_golden
    gnet, z, _, _ = _net_from_golden("a")
    with torch.no_grad():
        gnet(torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["cnoise"]).to(DEV))
    gops = _attention_ops(gnet, z["x"].shape[0])
    assert gops and all(nm == "aid_time_attention" and T <= 128 for nm, T in gops)


@pytest.mark.parametrize("name", ["X", "Y"])
def test_input_vjp_vs_oracle_autograd(name):
    """torch.autograd.grad through the drop-in network (autograd bridge -> hand-written VJP plan) vs the oracle"""
    net, orc, _, Ls = _setup(name)
    x, cn = _inputs(2, Ls)
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(3))
    xr = x.clone().requires_grad_()
    ref = torch.autograd.grad((orc(xr, cn) * g).sum(), xr)[0]
    xd = x.to(DEV).requires_grad_()
    got = torch.autograd.grad((net(xd, cn.to(DEV)) * g.to(DEV)).sum(), xd)[0]
    e = rel_l2(got.cpu(), ref)
    print(f"long segments, config {name}: input-VJP rel-L2 vs oracle autograd = {e:.3e}")
    assert e < TOL


def test_parameter_gradients_vs_oracle_autograd():
    """config X with the qk bias and the relative-position embedding switched on: their gradients come out of the long backward's dS scratch"""
    from test_gpu_training import _oracle_grads
    net, orc, _, Ls = _setup("X", bias_qkv=True, use_rel_pos=True)
    x, cn = _inputs(2, Ls)
    target = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)) * 0.2
    loss, _ = net.loss_and_grads(x.to(DEV), cn.to(DEV), target.to(DEV), hpf_error=False)
    ref_loss, ref = _oracle_grads(orc, x, cn, target, False)
    assert abs(float(loss) - ref_loss) < 1e-5 * abs(ref_loss)
    got = {k: v.detach().cpu() for k, v in net.train_state(x.shape[0])["builder"].pgrad.items()}
    assert any(k.endswith("relative_attention_bias.weight") for k in ref) and any(k.endswith("qk.bias") for k in ref)
    tot_num = tot_den = 0.0
    worst = ("", 0.0)
    gmax = max(float(v.norm()) for v in ref.values())
    for k, r in ref.items():
        if k.endswith("RFF_freq") or k.endswith("kernel") or k.endswith("embeddings"):
            assert float(got[k].abs().max()) == 0.0              # frozen tensors
            continue
        d = float((got[k].double() - r.double()).norm())
        tot_num += d * d
        tot_den += float(r.double().norm()) ** 2
        e = d / (float(r.norm()) + 1e-6 * gmax)
        if e > worst[1]:
            worst = (k, e)
    tot = math.sqrt(tot_num / tot_den)
    print(f"long segments, config X (bias_qkv, use_rel_pos): parameter gradients, all tensors together rel-L2 = {tot:.2e}; "
          f"worst tensor {worst[0]} {worst[1]:.2e}; loss {float(loss):.6f}")
    assert tot < 1e-4 and worst[1] < 1e-3


def test_batch_of_four_vs_single_items():
    """B = 4 runs as two sub-batch streams with graph replay; every item against its own B = 1 evaluation"""
    net, _, _, Ls = _setup("X")
    x, cn = _inputs(4, Ls)
    with torch.no_grad():
        four = net(x.to(DEV), cn.to(DEV)).cpu()
        errs = [rel_l2(net(x[j:j + 1].to(DEV), cn[j:j + 1].to(DEV)).cpu(), four[j:j + 1]) for j in range(4)]
    print("long segments, config X: B = 4 against B = 1, rel-L2 per item:", ["%.2e" % e for e in errs])
    assert max(errs) < 1e-6


def _sampler(net, args):
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.sampler import Sampler
    args.tester.T, args.tester.posterior_sampling.xi = 3, 0.25
    args.tester.data_consistency.hann_size = 20
    return Sampler(model=net, diff_params=EDM(args), args=args)


def test_guided_sampler_vs_oracle():
    from oracle.edm import OracleEDM
    from oracle.sampler import OracleSampler
    net, orc, args, Ls = _setup("X")
    y = _inputs(2, Ls)[0] * 0.126
    mask = torch.ones(1, Ls)
    mask[:, 1800:2300] = 0
    smp = _sampler(net, args)
    smp.seeds, smp.trace = [5, 6], []
    out = smp.predict_inpainting((y * mask).to(DEV), mask.to(DEV))
    osmp = OracleSampler(orc, OracleEDM(), T=3, xi=0.25, hann_size=20, audio_len=Ls)
    ref = osmp.predict_inpainting(y * mask, mask, seeds=[5, 6], record=True)
    errs = [rel_l2(a.cpu(), b) for a, b in zip(smp.trace, osmp.trace)]
    print("long segments, config X: guided per-evaluation x_hat rel-L2:", ["%.2e" % e for e in errs], " final:", "%.2e" % rel_l2(out.cpu(), ref))
    assert len(errs) == 5 and errs[0] < 1e-4 and max(errs) < 5e-4


def test_restore_long_runs_and_its_first_window_is_predict_inpainting():
    """one recording of 2.5 windows with a gap in every window through harness.restore_long; window 0 (pass A, seed seeds[0] * 65536 + 0) against
    predict_inpainting on the same gathered window, bit for bit over the samples that window owns"""
    from audio_inpainting_diffusion_amd import harness
    from audio_inpainting_diffusion_amd.restore import job_table, restore_plan, window_gather
    from audio_inpainting_diffusion_amd.sampler import autoregressive_overlap
    net, _, args, Ls = _setup("X")
    smp = _sampler(net, args)
    end = int(autoregressive_overlap(smp.args) * Ls)
    N, seed = 2 * Ls + Ls // 2, 23
    rec = torch.randn(N, generator=torch.Generator().manual_seed(4)) * 0.063
    mask = torch.ones(N)
    for w in range(3):
        s = w * (Ls - end)
        mask[s + Ls // 3:s + Ls // 3 + 300] = 0
    A, B, _ = restore_plan(mask[None], Ls, end)
    assert len(A) + len(B) == 3 and A[0][:2] == (0, 0)
    out = harness.restore_long(smp, [rec], [mask], seeds=[seed], max_batch=1)[0]
    assert out.is_cuda and out.shape == (N,) and bool(torch.isfinite(out).all())
    assert not torch.equal(out.cpu()[mask == 0], rec[mask == 0])
    rec_d = rec[None].to(DEV)
    yw, mw = window_gather(rec_d, rec_d, mask[None].to(DEV), job_table(A[:1], DEV), Ls)
    smp.seeds = [seed * 65536]
    ref = smp.predict_inpainting(yw, mw)
    _, s, _, _, lo, hi = A[0]
    assert hi - lo >= Ls // 2 and torch.equal(out[s + lo:s + hi], ref[0, lo:hi])
