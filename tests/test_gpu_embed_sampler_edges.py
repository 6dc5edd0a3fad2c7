"""The embedding kernels (csrc/aid_embed.hip) and the sampler's element-wise and per-item kernels (csrc/aid_sampler.hip), each directly against a
float64 reference of the same operation on the same float32 inputs: aid_embed at the widest layers it accepts and at the narrowest, aid_modulation
across its 16-sample launches with a ragged last workgroup, aid_axpby and aid_score_step in every scalar / NULL / broadcast form and one element
past the 1024-block grid (second trip of the grid-stride loop), aid_row_norm, aid_guidance_step and aid_guidance_seed around the 1024-thread
stride with an all-zero item, aid_set_rows with a padded leading dimension, and the refusals.  Outputs are NaN pre-filled between two sentinels.

Bounds (header of test_gpu_kernels.py): 2e-6 rel-L2 element-wise, 1e-5 reductions, 2e-5 aid_embed.  aid_score_step and aid_guidance_step are held
elementwise: max-abs error at most FOUR times that of the same formula in float32 on the CPU (torch, same operand order) against the float64
reference, the CPU figure taken over all lengths of the case (a length of 1 has three elements, too few to measure a rounding error on).
Every case prints its figures (profiles/r32_norm_pointwise_sampler_edges.txt)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
SENT = 123.0
B3 = 3
GRID_L = 1024 * 256 + 257            # one element past the 1024-block grid plus a ragged block: the grid-stride loop takes a second trip
LS_GRID = [1, 255, 257, GRID_L]
LS_ITEM = [1, 1000, 1024, 1025, 50000]      # 1024 threads per item: below, exactly one trip, one element into the second, many trips


@pytest.fixture(scope="module")
def L():
    from audio_inpainting_diffusion_amd import _lib
    _lib.lib()
    return _lib


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def f32(v):
    return float(np.float32(v))


class Out:
    """n float32 values pre-filled with NaN between two sentinels"""

    def __init__(self, *shape, fill=NAN):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2,), SENT, device=DEV)
        self.buf[1:-1] = fill
        self.t = self.buf[1:-1].view(*shape)

    def ptr(self):
        return self.t.data_ptr()

    def cpu(self):
        torch.cuda.synchronize()
        assert float(self.buf[0]) == SENT and float(self.buf[-1]) == SENT, "wrote outside the output"
        return self.t.cpu()


def _dev(*ts):
    return [None if t is None else t.to(DEV).contiguous() for t in ts]


def _abs_errs(got, ref, cpu32):
    g = got.double()
    assert bool(torch.isfinite(g).all())
    return float((g - ref).abs().max()), float((cpu32.double() - ref).abs().max())


def _hold(tag, pairs):
    """pairs: (label, kernel max-abs error, fp32-CPU max-abs error) of one case over all its lengths"""
    bound = 4 * max(c for _, _, c in pairs)
    print(f"{tag}: fp32-cpu max |err| {bound / 4:.2e}, bound {bound:.2e}; kernel " + " ".join(f"{lab} {g:.2e}" for lab, g, _ in pairs))
    assert all(g <= bound for _, g, _ in pairs), tag


# ---------------------------------------------------------------------------------------------------------
# aid_embed
def _embed_case(rff, h0, h1, E, B, seed):
    """the RFF angle in float32 with the kernel's association ((2 pi) sigma) freq, so that both sides round the ~1e2-rad argument alike; sin / cos and
    the three ReLU layers in float64"""
    freq = 5 * _rand(rff, seed=seed)
    dims = [(h0, 2 * rff), (h1, h0), (E, h1)]
    Ws = [_rand(o, i, seed=seed + 1 + k, scale=1 / math.sqrt(i)) for k, (o, i) in enumerate(dims)]
    bs = [0.1 * _rand(o, seed=seed + 5 + k) for k, (o, i) in enumerate(dims)]
    sig = torch.tensor([-0.9, 0.4, -0.3][:B])
    two_pi = torch.tensor(2.0) * torch.tensor(3.14159265358979323846)
    ang = ((two_pi * sig)[:, None] * freq[None]).double()
    x = torch.cat([torch.sin(ang), torch.cos(ang)], dim=1)
    for W, b in zip(Ws, bs):
        x = torch.relu(x @ W.double().t() + b.double())
    return sig, freq, Ws, bs, x, float(ang.abs().max())


def _embed_params(L, d, emb_ptr, B, rff, h0, h1, E):
    return L.EmbedParams(*[t.data_ptr() for t in d], emb_ptr, B, rff, h0, h1, E)


@pytest.mark.parametrize("widths", [(512, 1024, 300, 700),          # 2 rff = h0 = EMB_MAX; every += 256 loop with several trips, two ragged
                                    (3, 5, 7, 1)])                  # a handful of threads live in every loop
def test_embed(L, widths):
    rff, h0, h1, E = widths
    sig, freq, Ws, bs, ref, amax = _embed_case(rff, h0, h1, E, B3, seed=40)
    d = _dev(sig, freq, Ws[0], bs[0], Ws[1], bs[1], Ws[2], bs[2])
    emb = Out(B3, E)
    L.call("aid_embed", _embed_params(L, d, emb.ptr(), B3, rff, h0, h1, E))
    got = emb.cpu()
    e = rel_l2(got, ref)
    print(f"embed {widths}: max |angle| {amax:.0f} rad, rel-L2 {e:.2e}")
    assert bool(torch.isfinite(got).all()) and float(ref.abs().max()) > 0 and e < 2e-5


@pytest.mark.parametrize("widths", [(513, 64, 64, 8), (16, 1025, 64, 8)])       # 2 rff = 1026 and h0 = 1025: one past the LDS buffers
def test_embed_refuses_wide_layers(L, widths):
    rff, h0, h1, E = widths
    sig, freq, Ws, bs, _, _ = _embed_case(rff, h0, h1, E, B3, seed=43)
    d = _dev(sig, freq, Ws[0], bs[0], Ws[1], bs[1], Ws[2], bs[2])
    emb = Out(B3, E, fill=SENT)
    with pytest.raises(L.AidError):
        L.call("aid_embed", _embed_params(L, d, emb.ptr(), B3, rff, h0, h1, E))
    assert bool((emb.cpu() == SENT).all())


# ---------------------------------------------------------------------------------------------------------
# aid_modulation
@pytest.mark.parametrize("E", [48, 200])             # below one wave; three full trips of a wave and a ragged fourth
@pytest.mark.parametrize("B", [1, 16, 17, 33])       # one, one, two and three launches of 16 samples
def test_modulation(L, B, E):
    N = 1002                                         # 250 workgroups of four rows and one of two
    W, bias, emb = _rand(N, E, seed=50 + E, scale=1 / math.sqrt(E)), _rand(N, seed=51), _rand(B, E, seed=52 + B)
    Wd, bd, ed = _dev(W, bias, emb)
    ref = emb.double() @ W.double().t()
    errs = []
    for with_bias in (True, False):
        mod = Out(B, N)
        L.call("aid_modulation", L.ModulationParams(ed.data_ptr(), Wd.data_ptr(), bd.data_ptr() if with_bias else None, mod.ptr(), B, E, N))
        got = mod.cpu()
        assert bool(torch.isfinite(got).all())
        errs.append(rel_l2(got, ref + bias.double() if with_bias else ref))
    print(f"modulation B={B} E={E} N={N}: rel-L2 with bias {errs[0]:.2e}, bias = NULL {errs[1]:.2e}")
    assert max(errs) < 1e-5


# ---------------------------------------------------------------------------------------------------------
# aid_axpby
@pytest.mark.parametrize("form", ["device", "host", "y_null", "y_is_x"])
@pytest.mark.parametrize("Ls", LS_GRID)
def test_axpby(L, Ls, form):
    x, y = _rand(B3, Ls, seed=60), _rand(B3, Ls, seed=61)
    a, b = torch.tensor([0.7, -1.3, 2.1]), torch.tensor([-0.4, 0.9, 1.6])
    xd, yd, ad, bd = _dev(x, y, a, b)
    out = Out(B3, Ls)
    if form == "device":
        p = L.AxpbyParams(xd.data_ptr(), yd.data_ptr(), out.ptr(), ad.data_ptr(), bd.data_ptr(), B3, Ls)
        ref = a.double()[:, None] * x.double() + b.double()[:, None] * y.double()
    elif form == "host":
        p = L.AxpbyParams(xd.data_ptr(), yd.data_ptr(), out.ptr(), None, None, B3, Ls, 0.7, -1.3)
        ref = f32(0.7) * x.double() + f32(-1.3) * y.double()
    elif form == "y_null":                           # network.py: a per-item scalar times x
        p = L.AxpbyParams(xd.data_ptr(), None, out.ptr(), ad.data_ptr(), None, B3, Ls)
        ref = a.double()[:, None] * x.double()
    else:                                            # sampler.py: score = (-1 / t) d, y = x with b_host = 0
        p = L.AxpbyParams(xd.data_ptr(), xd.data_ptr(), out.ptr(), None, None, B3, Ls, -1.0 / 0.37, 0.0)
        ref = f32(-1.0 / 0.37) * x.double()
    L.call("aid_axpby", p)
    got = out.cpu()
    e = rel_l2(got, ref)
    print(f"axpby {form} L={Ls}: rel-L2 {e:.2e}")
    assert bool(torch.isfinite(got).all()) and e < 2e-6


# ---------------------------------------------------------------------------------------------------------
# aid_score_step
def _score_ref(x, xh, y, m, t, h, mode, x0, d0):
    """(xh_out, d, xnext) in float64 and in float32 with the kernel's operand order (1 / t formed once, then multiplied)"""
    res = []
    for dt in (torch.float64, torch.float32):
        X, XH, T_, H = x.to(dt), xh.to(dt), t.to(dt)[:, None], h.to(dt)[:, None]
        if m is not None:
            XH = m.to(dt) * y.to(dt) + (1.0 - m.to(dt)) * XH
        d = (X - XH) / T_ if dt == torch.float64 else (X - XH) * (1.0 / T_)
        nxt = X + H * d if mode == 0 else x0.to(dt) + H * (0.5 * d0.to(dt) + 0.5 * d)
        res.append((XH, d, nxt))
    return res


SCORE_FORMS = ["device", "host", "no_mask", "broadcast_mask", "no_dout_xh", "heun"]


@pytest.mark.parametrize("form", SCORE_FORMS)
def test_score_step(L, form):
    pairs = []
    for Ls in LS_GRID:
        x, xh, y, x0, d0 = (_rand(B3, Ls, seed=70 + k) for k in range(5))
        per_item = torch.rand(B3, Ls, generator=torch.Generator().manual_seed(76))
        host = form == "host"
        t = torch.full((B3,), 0.7) if host else torch.tensor([0.5, 0.7, 0.9])
        h = torch.full((B3,), -0.2) if host else torch.tensor([-0.1, -0.2, -0.3])
        m = None if form == "no_mask" else (per_item[:1] if form == "broadcast_mask" else per_item)
        mode = 1 if form == "heun" else 0
        outs = form != "no_dout_xh"
        (xh64, d64, n64), (xh32, d32, n32) = _score_ref(x, xh, y, m, t, h, mode, x0, d0)
        xd, xhd, yd, md, x0d, d0d, td, hd = _dev(x, xh, y, m, x0, d0, t, h)

        def run(host_scalars, want):
            xn, dd, xo = Out(B3, Ls), Out(B3, Ls), Out(B3, Ls)
            p = L.ScoreStepParams(xd.data_ptr(), xhd.data_ptr(), None if m is None else yd.data_ptr(), L.ptr(md), 0 if m is None or m.shape[0] == 1 else Ls,
                                  x0d.data_ptr() if mode else None, d0d.data_ptr() if mode else None,
                                  None if host_scalars else td.data_ptr(), None if host_scalars else hd.data_ptr(),
                                  xn.ptr(), dd.ptr() if want else None, xo.ptr() if want else None, B3, Ls, mode, 0.7, -0.2)
            L.call("aid_score_step", p)
            return xn.cpu(), dd.cpu(), xo.cpu()
        xn, dd, xo = run(host, outs)
        pairs.append((f"L={Ls} xnext", *_abs_errs(xn, n64, n32)))
        if outs:
            pairs.append((f"L={Ls} xh", *_abs_errs(xo, xh64, xh32)))
            assert rel_l2(xo, xh64) < 2e-6
        else:
            assert bool(torch.isnan(xo).all()) and bool(torch.isnan(dd).all())          # NULL outputs: nothing written there
        if mode == 0 and outs:
            pairs.append((f"L={Ls} d", *_abs_errs(dd, d64, d32)))
            assert rel_l2(dd, d64) < 2e-6
        elif outs:
            assert bool(torch.isnan(dd).all())                                          # the Heun combine writes no direction
        assert rel_l2(xn, n64) < 2e-6
        if host:                                                                        # host scalars against the same values on the device: the same bits
            assert all(torch.equal(u, v) for u, v in zip(run(False, outs), (xn, dd, xo)) if not bool(torch.isnan(u).all()))
        if form == "no_dout_xh":
            assert torch.equal(run(False, True)[0], xn)
    _hold(f"score_step {form}", pairs)


def test_score_step_refusals(L):
    Ls = 257
    xd, xhd, md = _dev(_rand(B3, Ls, seed=77), _rand(B3, Ls, seed=78), torch.ones(B3, Ls))
    for mode, mask in ((1, None), (0, md)):                                             # the Heun combine without x0 / d0; a mask without observations
        xn = Out(B3, Ls, fill=SENT)
        p = L.ScoreStepParams(xd.data_ptr(), xhd.data_ptr(), None, L.ptr(mask), Ls, None, None, None, None, xn.ptr(), None, None, B3, Ls, mode, 0.7, -0.2)
        with pytest.raises(L.AidError):
            L.call("aid_score_step", p)
        assert bool((xn.cpu() == SENT).all())


# ---------------------------------------------------------------------------------------------------------
# aid_row_norm, aid_guidance_step
def test_row_norm(L):
    errs = []
    for Ls in LS_ITEM:
        x = _rand(B3, Ls, seed=80)
        x[1] = 0.0
        out = Out(B3)
        L.call("aid_row_norm", L.RowNormParams(_dev(x)[0].data_ptr(), out.ptr(), B3, Ls))
        got = out.cpu()
        errs.append(rel_l2(got, x.double().norm(dim=1)))
        assert bool(torch.isfinite(got).all()) and float(got[1]) == 0.0
    print("row_norm rel-L2 " + " ".join(f"L={l} {e:.2e}" for l, e in zip(LS_ITEM, errs)))
    assert max(errs) < 1e-5


@pytest.mark.parametrize("extra", [True, False], ids=["step_s_out", "null_outs"])
def test_guidance_step(L, extra):
    coef, eps = f32(0.37), f32(1e-6)
    pairs, s_errs = [], []
    for Ls in LS_ITEM:
        inv = f32(1.0 / math.sqrt(Ls))
        xhat, g = _rand(B3, Ls, seed=85), _rand(B3, Ls, seed=86, scale=3.0)
        g[1] = 0.0
        nrm = g.double().norm(dim=1)
        s64 = coef / (nrm * inv + eps)
        s32 = torch.tensor(coef) / (nrm.float() * inv + eps)                            # (the kernel sums in float64 and rounds the norm once)
        ref, cpu = xhat.double() - s64[:, None] * g.double(), xhat - s32[:, None] * g
        xd, gd = _dev(xhat, g)
        out, step, s = Out(B3, Ls), Out(B3, Ls), Out(B3)
        p = L.GuidanceStepParams(xd.data_ptr(), gd.data_ptr(), out.ptr(), step.ptr() if extra else None, s.ptr() if extra else None, B3, Ls, coef, inv, eps)
        L.call("aid_guidance_step", p)
        got, st, sg = out.cpu(), step.cpu(), s.cpu()
        pairs.append((f"L={Ls} out", *_abs_errs(got, ref, cpu)))
        assert torch.equal(got[1], xhat[1])                                             # the all-zero item: out == xhat exactly
        if extra:
            pairs.append((f"L={Ls} step", *_abs_errs(st, s64[:, None] * g.double(), s32[:, None] * g)))
            s_errs.append(rel_l2(sg, s64))
            assert float(sg[1]) == float(np.float32(coef) / np.float32(eps)) and bool((st[1] == 0).all())
        else:
            assert bool(torch.isnan(st).all()) and bool(torch.isnan(sg).all())
    if extra:
        print("guidance_step s_out rel-L2 " + " ".join(f"L={l} {e:.2e}" for l, e in zip(LS_ITEM, s_errs)))
        assert max(s_errs) < 1e-5
    _hold(f"guidance_step extra={int(extra)}", pairs)


# ---------------------------------------------------------------------------------------------------------
# aid_guidance_seed
@pytest.mark.parametrize("mask_kind", ["none", "per_item", "broadcast"])
@pytest.mark.parametrize("norm_type", [2, 1, 3])
def test_guidance_seed(L, norm_type, mask_kind):
    """r = y - mask xhat with binary masks (the products are exact whether or not they are contracted into the subtraction), exact zeros in r, for
    the smooth-L1 norm values on both sides of beta, and item 1 with y == mask xhat"""
    beta = f32(0.5)
    figs = []
    for Ls in [1, 1000, 1025, 50000]:
        xhat, y = _rand(B3, Ls, seed=90), _rand(B3, Ls, seed=91)
        m = None if mask_kind == "none" else (torch.rand(B3 if mask_kind == "per_item" else 1, Ls, generator=torch.Generator().manual_seed(92)) < 0.7).float()
        mx = xhat if m is None else m * xhat
        y[:, ::5] = mx[:, ::5]
        y[1] = mx[1]
        r = y.double() - mx.double()
        assert bool((r == 0).any()) and (Ls < 1000 or norm_type != 3 or (bool((r.abs() < beta).any()) and bool((r.abs() > beta).any())))
        mm = torch.ones(1, Ls, dtype=torch.float64) if m is None else m.double()
        if norm_type == 2:
            nref = r.norm(dim=1)
            d = torch.where(nref[:, None] > 0, r / nref[:, None], torch.zeros_like(r))
        elif norm_type == 1:
            nref, d = r.abs().sum(1), torch.sign(r)
        else:
            ar = r.abs()
            nref = torch.where(ar < beta, 0.5 * r * r / beta, ar - 0.5 * beta).sum(1)
            d = torch.where(ar < beta, r / beta, torch.sign(r))
        gref = -mm * d
        xd, yd, md = _dev(xhat, y, m)
        g, nrm = Out(B3, Ls), Out(B3)
        p = L.GuidanceSeedParams(xd.data_ptr(), yd.data_ptr(), L.ptr(md), Ls if mask_kind == "per_item" else 0, g.ptr(), nrm.ptr(), B3, Ls, norm_type, beta)
        L.call("aid_guidance_seed", p)
        gg, gn = g.cpu(), nrm.cpu()
        assert bool(torch.isfinite(gg).all()) and bool(torch.isfinite(gn).all())
        assert float(gn[1]) == 0.0 and bool((gg[1] == 0).all())                         # residual exactly zero: norm 0, gradient finite and zero
        if norm_type == 1:
            assert torch.equal(gg.double(), gref + 0.0)                                 # signs times the mask: exact
        figs.append((Ls, rel_l2(gn, nref), rel_l2(gg, gref)))                           # (L = 1: every residual is zero, and so must g be)
    print(f"guidance_seed norm_type={norm_type} mask={mask_kind}: " + " ".join(f"L={l} norm {a:.2e} g {b:.2e}" for l, a, b in figs))
    assert max(a for _, a, _ in figs) < 1e-5
    assert max(b for _, _, b in figs) < (1e-5 if norm_type == 2 else 2e-6)              # type 2 divides by the reduced norm; types 1 and 3 are element-wise


def test_guidance_seed_refusals(L):
    Ls = 100
    xd, yd = _dev(_rand(B3, Ls, seed=95), _rand(B3, Ls, seed=96))
    for norm_type, beta in ((4, 1.0), (3, 0.0)):
        g, nrm = Out(B3, Ls, fill=SENT), Out(B3, fill=SENT)
        with pytest.raises(L.AidError):
            L.call("aid_guidance_seed", L.GuidanceSeedParams(xd.data_ptr(), yd.data_ptr(), None, 0, g.ptr(), nrm.ptr(), B3, Ls, norm_type, beta))
        assert bool((g.cpu() == SENT).all()) and bool((nrm.cpu() == SENT).all())


# ---------------------------------------------------------------------------------------------------------
# aid_set_rows
@pytest.mark.parametrize("B", [1, 64, 65])           # one lane; a full wave; one value into the second trip of the 64-thread loop
@pytest.mark.parametrize("n", [1, 8])
def test_set_rows(L, n, B):
    ld = B + 3
    vals = [f32(0.1 * (i + 1) - 0.35) for i in range(n)]
    out = Out(n + 1, ld, fill=SENT)                  # row n and the padding of every row are sentinels too
    L.call("aid_set_rows", L.SetRowsParams(out.ptr(), ld, B, n, (ctypes.c_float * 8)(*vals, *([7.0] * (8 - n)))))
    got = out.cpu()
    assert all(bool((got[i, :B] == vals[i]).all()) for i in range(n))
    assert bool((got[:n, B:] == SENT).all()) and bool((got[n] == SENT).all())


@pytest.mark.parametrize("n,B,ld", [(0, 4, 7), (9, 4, 7), (2, 8, 7)])
def test_set_rows_refusals(L, n, B, ld):
    out = Out(10, 16, fill=SENT)
    with pytest.raises(L.AidError):
        L.call("aid_set_rows", L.SetRowsParams(out.ptr(), ld, B, n, (ctypes.c_float * 8)(*([1.0] * 8))))
    assert bool((out.cpu() == SENT).all())
