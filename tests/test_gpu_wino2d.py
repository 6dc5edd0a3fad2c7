"""GPU parity of the non-fused 2-D Winograd path F(4,5) x F(4,3) of the dilated 5x3 convolution (csrc/aid_wino2d.hip), through the C ABI:
aid_scale_act(wino=3) -> aid_conv2d(x_wino=3) = aid_wino2d_gemm + output pass, against the torch-CPU form of the plain convolution
(reference: Conv2d.forward / ResnetBlock.forward, networks/unet_cqt_oct_with_projattention_adaLN_2.py:79-88, :472-482).

fp32 error budget of the form: 1e-5 rel-L2 per layer (tools/wino2d_fm5_error.py: 2.2e-6 ... 4.3e-6).
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def L():
    from audio_inpainting_diffusion_amd import _lib
    _lib.lib()
    return _lib


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@pytest.mark.parametrize("shape", [(128, 128, 256), (64, 128, 1000), (256, 256, 2052), (32, 128, 4), (96, 96, 1000), (64, 192, 260)])
def test_wino2d_gemm_vs_torch(L, shape):
    """M[xi] = U[xi]^T V[xi] for 48 planes; ragged last column tile, K of 2 .. 16 chunks"""
    cin, cout, N = shape
    cip, cop = L.pack_dims(cin, cout)
    U = torch.zeros(48, cip, cop)
    U[:, :cin, :cout] = _rand(48, cin, cout, seed=1, scale=1 / math.sqrt(cin))
    V = _rand(48, cin, N, seed=2)
    Ud, Vd = U.to(DEV), V.to(DEV)
    M = torch.full((48, cout, N + 8), 7.0, device=DEV)[:, :, :N].contiguous()
    tail = torch.full((64,), 7.0, device=DEV)
    p = L.Wino2dGemmParams(Ud.data_ptr(), Vd.data_ptr(), M.data_ptr(), 48, cin, cout, cip, cop, N, 0)
    L.call("aid_wino2d_gemm", p)
    torch.cuda.synchronize()
    ref = torch.bmm(U[:, :cin, :cout].transpose(1, 2).double(), V.double())
    assert rel_l2(M.cpu(), ref) < 2e-6
    assert float(tail.min()) == 7.0
    # the labelled split-precision variant (three bf16 pieces per fp32 operand, six products on the bf16 matrix pipe, fp32 accumulation): the pieces are an
    # exact decomposition; the dropped cross terms p1 q2 + p2 q1 are ~2^-24 of a product each (measured max 2^-21.3, median 2^-25.2: tools/bf16split_error.py
    # --per-product) -- the order of one fp32 rounding, NOT below 2^-32 -- and the bf16 MFMA sums 16 products per instruction, so over a K-long sum the
    # variant measures at least as close to the fp64 product as the fp32-MFMA kernel (an empirical bar, asserted below, not an exactness claim)
    e32 = rel_l2(M.cpu(), ref)
    if cout % 128 == 0:
        for variant in (100, 101):
            M.fill_(7.0)
            p.variant = variant
            L.call("aid_wino2d_gemm", p)
            torch.cuda.synchronize()
            assert "w2d_gemm_s6" in L.lib().aid_last_kernel().decode()
            es = rel_l2(M.cpu(), ref)
            print(f"GEMM {shape}: fp32 MFMA {e32:.2e}, bf16 x 6 split (variant {variant}) {es:.2e}")
            assert es < 2e-6 and es < 1.5 * e32 + 1e-8 and float(tail.min()) == 7.0


def _conv_ref(x, w, dil, in_scale, act, out_scale, res, res_scale, alpha):
    h = x * in_scale[:, :, None, None]
    if act:
        h = F.gelu(h)
    y = F.conv2d(h, w, padding="same", dilation=(dil, 1))
    if out_scale is not None:
        y = y * out_scale[:, :, None, None]
    if res is not None:
        y = y + res_scale * res
    return alpha * y


W2D_CASES = [
    # B, C, F, T, dil
    (2, 128, 16, 32, 1),         # R = 16: 4 row tiles
    (1, 128, 24, 64, 2),         # R = 12, two residue classes
    (2, 128, 20, 16, 4),         # R = 5: ragged (second tile holds one real row), T = 16
    (1, 128, 28, 32, 1),         # R = 28
    (2, 128, 24, 32, 8),         # R = 3: a single ragged tile per class
    (1, 256, 12, 48, 2),         # two Cout tiles, T = 48 (TG = 12)
    (3, 128, 8, 528, 1),         # TG = 132 > 64 lanes: neighbour samples across wave boundaries
    (2, 96, 24, 64, 2),          # the 96-channel levels: 96 x 128 GEMM tiles (three interleaved row fragments per lane), K = 6 chunks
    (1, 192, 16, 32, 1),         # two 96-row tiles
    (1, 128, 12, 512, 2),        # T = 512: the input pass works in two T segments of 256 samples with a float4 of halo on either side
]


def _input_ref(h, dil, tf=4):
    """V[xf*NTP+xt][c][b*NB + (j*dil + r)*TG + g] from its definition, float64 on the CPU (tf = 4: F(4,3) along T, 6 planes; tf = 8: F(8,3), 10 planes)"""
    from audio_inpainting_diffusion_amd._lib import wino45_matrices, wino8_matrices
    BF = torch.from_numpy(wino45_matrices()[2])
    BT = torch.from_numpy(wino45_matrices()[5] if tf == 4 else wino8_matrices()[2])
    ntp = tf + 2
    B, C, Fd, T = h.shape
    R, TG = Fd // dil, T // tf
    J = (R + 3) // 4
    hs = h.double().reshape(B, C, R, dil, T)                              # row f = jj * dil + r
    hp = F.pad(hs, (1, tf, 0, 0, 2, 4 * J + 4 - R))                          # jj: 2 before, up to 4J+5 after; t: 1 before, tf after
    pt = hp.unfold(-1, ntp, tf)[..., :TG, :]                                # [B, C, JJ, dil, TG, ntp]
    pf = pt.unfold(2, 8, 4)[:, :, :J]                                       # [B, C, J, dil, TG, ntp, 8]
    V = torch.einsum("xi,yk,bcjrgki->xybjrgc", BF, BT, pf)                  # [8, ntp, B, J, dil, TG, C]
    return V.reshape(8 * ntp, B * J * dil * TG, C).permute(0, 2, 1).contiguous()  # [nxi, C, N]


W2D8_CASES = [
    # the F(8,3)-along-T variant (x_wino = 4): T % 32 == 0
    (2, 128, 16, 32, 1),         # TG = 4
    (1, 128, 24, 64, 2),         # two residue classes
    (2, 128, 20, 32, 4),         # R = 5: ragged row tiles
    (2, 128, 24, 32, 8),         # R = 3: a single ragged tile per class
    (1, 256, 12, 96, 2),         # two Cout tiles, TG = 12
    (3, 128, 8, 544, 1),         # TG = 68 > 64 lanes: neighbour samples across wave boundaries
    (2, 96, 24, 64, 2),          # 96-channel level
    (1, 96, 8, 1024, 4),         # T = 1024: four T segments in the input pass, four residue classes
    (2, 128, 20, 512, 1),        # T = 512, ragged row tiles
]


def _check_fin_forward(L, p, y, sws, nst, gamma, sc2, st2, gemm_name):
    """fin_mode = 1 on the forward launch p (whose plain run gave y, and whose partials aid_group_stats(ws_n = nst) folded into sc2 / st2): the LAST block of each
    sample's output pass folds the partials itself -- the same bits as aid_group_stats(ws_n = nst), counters back to zero; through aid_conv2d and through the two
    separate entry points (GEMM, then output pass), where the GEMM that ran is asserted by name.  Returns the counters for the reverse sweep."""
    B, C = p.B, p.Cout
    y2 = torch.empty_like(y)
    p.y = L.view4(y2)
    cnt = torch.zeros(B + 2, device=DEV, dtype=torch.int32)
    cnt[B:] = 7
    for rep in range(2):
        scf, stf = torch.full((B, C), float("nan"), device=DEV), torch.full((B, 8, 2), float("nan"), device=DEV)
        sws.fill_(float("nan"))
        y2.fill_(float("nan"))
        p.fin_mode, p.fin_count, p.fin_gamma, p.fin_eps, p.fin_scale, p.fin_stats = 1, cnt.data_ptr(), gamma.data_ptr(), 1e-7, scf.data_ptr(), stf.data_ptr()
        if rep == 0:
            L.call("aid_conv2d", p)
        else:
            L.call("aid_conv2d_wino2d_gemm", p)
            assert gemm_name in L.lib().aid_last_kernel().decode(), L.lib().aid_last_kernel().decode()
            L.call("aid_conv2d_wino2d_output", p)
            assert L.lib().aid_last_kernel().decode() == "w2d_output_kernel"
        torch.cuda.synchronize()
        assert torch.equal(y2, y) and int(cnt[:B].abs().sum()) == 0 and int(cnt[B]) == 7
        assert torch.equal(scf, sc2) and torch.equal(stf, st2)
    p.fin_mode = 0
    return cnt


def _check_reverse(L, lay, XW, tol, stats, cnt, gemm_name, ref_dtype=torch.float32, slice_bar=None):
    """The reverse sweep of the layer y = alpha * conv(gelu(x in_scale), w) * out_scale: the transposed operator (Cout -> Cin) on the gated gradient (no activation),
    dGELU epilogue (epi = 1 with aux = x), <y, aux> partials in dot_ws, against torch.autograd.grad of the layer in ref_dtype on the CPU; then fin_mode = 2 -- the last
    block also writes the coefficients aid_norm_bwd's first kernel would compute from the partials (with the statistics `stats` [B, 8, 2] of x) -- the same bits.
    The GEMM of the transposed launch is asserted by name.  `lay` holds the layer: x, w, in_scale, out_scale, their device copies xd, wd, isd, osd, alpha and dil
    (a _FoldedLayer, or a namespace of the same names).  Returns the transposed packs."""
    x, w, in_scale, out_scale, xd, wd, isd, osd, alpha, dil = lay.x, lay.w, lay.in_scale, lay.out_scale, lay.xd, lay.wd, lay.isd, lay.osd, lay.alpha, lay.dil
    B, Ci, Fd, T = x.shape
    Co = w.shape[0]
    NXI = 48 if XW == 3 else 80
    tf = 4 if XW == 3 else 8
    N = int(L.lib().aid_conv2d_wino2d_positions(B, Fd, T, dil)) * 4 // tf
    pack2d = L.pack_conv_weight_wino2d if XW == 3 else L.pack_conv_weight_wino2d8
    nst = int(L.lib().aid_conv2d_dot_partials(B, Co, Ci, Fd, T, dil, XW))
    assert nst > 0
    gy = _rand(B, Co, Fd, T, seed=46)
    gyd = gy.to(DEV)
    V = torch.empty(NXI * Co * N, device=DEV)
    ws = torch.empty(NXI * Ci * N, device=DEV)
    sp = L.ScaleActParams(L.view4(gyd), L.View(V.data_ptr(), 0, 0, 0), osd.data_ptr(), osd.stride(0), B, Co, Fd, T, 0, XW, dil)
    L.call("aid_scale_act", sp)
    wpT, wpwT = L.pack_conv_weight(wd, transpose=True), pack2d(wd, transpose=True)
    gd = torch.full((B, Ci, Fd, T), float("nan"), device=DEV)
    dws = torch.zeros(B * 8 * nst, device=DEV, dtype=torch.float64)
    q = L.Conv2dParams()
    q.x, q.y, q.res, q.aux = L.View(V.data_ptr(), 0, 0, 0), L.view4(gd), L.view4(None), L.view4(xd)
    q.wp, q.wp_wino, q.wino_taps, q.x_wino = wpT.data_ptr(), wpwT.data_ptr(), NXI, XW
    q.out_scale, q.out_scale_ld = isd.data_ptr(), isd.stride(0)
    q.aux_scale, q.aux_scale_ld = isd.data_ptr(), isd.stride(0)
    q.B, q.Cin, q.Cout, q.F, q.T = B, Co, Ci, Fd, T
    q.Cin_pad, q.Cout_pad = wpT.shape[1], wpT.shape[2]
    q.KH, q.KW, q.dilF, q.act, q.epi = 5, 3, dil, 0, 1
    q.alpha, q.res_scale = alpha, 1.0
    q.ws, q.ws_bytes = ws.data_ptr(), NXI * Ci * N * 4
    q.dot_ws, q.dot_n = dws.data_ptr(), nst
    L.call("aid_conv2d", q)
    torch.cuda.synchronize()
    assert gemm_name in L.lib().aid_last_kernel().decode(), L.lib().aid_last_kernel().decode()
    xr = x.to(ref_dtype, copy=True).requires_grad_(True)
    hr = F.gelu(xr * in_scale.to(ref_dtype)[:, :, None, None])
    yr = alpha * F.conv2d(hr, w.to(ref_dtype), padding="same", dilation=(dil, 1)) * out_scale.to(ref_dtype)[:, :, None, None]
    gref, = torch.autograd.grad(yr, xr, gy.to(ref_dtype))                # = alpha * in_scale * gelu'(x in_scale) * conv^T(gy * out_scale)
    err = rel_l2(gd.cpu(), gref)
    if slice_bar is not None:
        e_row, e_tail = _slice_errs(gd.cpu(), gref)
        print(f"reverse {tuple(x.shape)} -> Cout {Co} d{dil}: rel-L2 vs autograd = {err:.2e}, worst (b, f) row {e_row:.2e}, worst (b, c) tail {e_tail:.2e}")
        assert e_row < slice_bar and e_tail < slice_bar, (e_row, e_tail)
    assert err < tol, err
    dref = (gd.cpu().double() * x.double()).reshape(B, 8, -1).sum(-1)
    assert rel_l2(dws.cpu().reshape(B, 8, nst).sum(-1), dref) < 1e-5
    # fin_mode = 2: the last block also writes the coefficients aid_norm_bwd's first kernel would compute from the partials -- same bits
    dwsf = torch.full((B * 8 * (nst + 1),), float("nan"), device=DEV, dtype=torch.float64)
    dwsf[:B * 8 * nst] = dws
    out = torch.empty_like(gd)
    npar = L.NormBwdParams(L.view4(gd), L.view4(xd), L.view4(None), L.view4(out), B, Ci, Fd, T, 8, stats.data_ptr(), dwsf.data_ptr(), 1e-7, 1.0, 0, nst)
    L.call("aid_norm_bwd", npar)
    torch.cuda.synchronize()
    coef_ref, out_ref = dwsf[B * 8 * nst:].view(torch.float32)[:B * 8].clone(), out.clone()
    assert bool(torch.isfinite(coef_ref).all()) and float(coef_ref.abs().max()) > 0
    gd2 = torch.empty_like(gd)
    q.y = L.view4(gd2)
    for _ in range(2):
        dwsf.fill_(float("nan"))
        q.dot_ws = dwsf.data_ptr()
        q.fin_mode, q.fin_count, q.fin_eps, q.fin_stats, q.fin_scale = 2, cnt.data_ptr(), 1e-7, stats.data_ptr(), dwsf.data_ptr() + 8 * B * 8 * nst
        L.call("aid_conv2d", q)
        npar.coef_ready = 1
        out.fill_(float("nan"))
        L.call("aid_norm_bwd", npar)
        torch.cuda.synchronize()
        assert torch.equal(gd2, gd) and torch.equal(dwsf[B * 8 * nst:].view(torch.float32)[:B * 8], coef_ref) and torch.equal(out, out_ref) and int(cnt[:B].abs().sum()) == 0
    return wpT, wpwT


@pytest.mark.parametrize("case", [c + (4,) for c in W2D_CASES] + [c + (8,) for c in W2D8_CASES])
def test_conv2d_wino2d(L, case):
    """tf = 4: F(4,5) x F(4,3) (x_wino = 3, 48 planes); tf = 8: F(4,5) x F(8,3) (x_wino = 4, 80 planes over groups of eight samples; fp32 error budget
    of that form 2e-5 per layer: tools/wino2d_fm5_error.py measures 1.0e-5 at Cin = 128, 1.3e-5 at Cin = 256)"""
    B, C, Fd, T, dil, tf = case
    XW, NXI = (3, 48) if tf == 4 else (4, 80)
    tol = 1e-5 if tf == 4 else 2.5e-5
    assert L.lib().aid_conv2d_wino2d_supported(C, C, Fd, T, dil)
    N = int(L.lib().aid_conv2d_wino2d_positions(B, Fd, T, dil))
    R = Fd // dil
    assert N == B * ((R + 3) // 4) * dil * (T // 4)
    N = N * 4 // tf
    pack2d = L.pack_conv_weight_wino2d if tf == 4 else L.pack_conv_weight_wino2d8
    x = _rand(B, C, Fd, T, seed=40)
    w = _rand(C, C, 5, 3, seed=41, scale=1.0 / math.sqrt(C * 15))
    in_scale = 1.0 + 0.5 * _rand(B, C, seed=42)
    out_scale = _rand(B, C, seed=43)
    res = _rand(B, C, Fd, T, seed=44)
    alpha, res_scale = 1 / math.sqrt(2), 1.5
    xd, wd, isd, osd, resd = x.to(DEV), w.to(DEV), in_scale.to(DEV), out_scale.to(DEV), res.to(DEV)
    # (1) the input transform against its definition (GELU prologue)
    V = torch.full((NXI * C * N + 16,), 7.0, device=DEV)
    sp = L.ScaleActParams(L.view4(xd), L.View(V.data_ptr(), 0, 0, 0), isd.data_ptr(), isd.stride(0), B, C, Fd, T, 1, XW, dil)
    L.call("aid_scale_act", sp)
    torch.cuda.synchronize()
    assert float(V[NXI * C * N:].min()) == 7.0
    Vref = _input_ref(F.gelu(x * in_scale[:, :, None, None]), dil, tf)
    assert rel_l2(V[:NXI * C * N].cpu().reshape(NXI, C, N), Vref) < 1e-6
    # (2) forward: the convolution on it, gate + residual epilogue, (sum, sum of squares) partials
    wp, wpw = L.pack_conv_weight(wd), pack2d(wd)
    y = torch.full((B, C, Fd, T), float("nan"), device=DEV)
    ws = torch.full((NXI * C * N + 16,), 7.0, device=DEV)
    nst = int(L.lib().aid_conv2d_stat_partials(B, C, C, Fd, T, dil, XW))
    assert nst > 0 and nst == int(L.lib().aid_conv2d_dot_partials(B, C, C, Fd, T, dil, XW))
    assert L.lib().aid_conv2d_fin_supported(B, C, C, Fd, T, dil, XW) == 1
    sws = torch.zeros(B * 8 * nst * 2, device=DEV, dtype=torch.float64)
    p = L.Conv2dParams()
    p.x, p.y, p.res, p.aux = L.View(V.data_ptr(), 0, 0, 0), L.view4(y), L.view4(resd), L.view4(None)
    p.wp, p.wp_wino, p.wino_taps, p.x_wino = wp.data_ptr(), wpw.data_ptr(), NXI, XW
    p.out_scale, p.out_scale_ld = osd.data_ptr(), osd.stride(0)
    p.B, p.Cin, p.Cout, p.F, p.T = B, C, C, Fd, T
    p.Cin_pad, p.Cout_pad = wp.shape[1], wp.shape[2]
    p.KH, p.KW, p.dilF, p.act, p.epi = 5, 3, dil, 0, 0
    p.alpha, p.res_scale = alpha, res_scale
    p.ws, p.ws_bytes = ws.data_ptr(), NXI * C * N * 4
    p.stat_ws, p.stat_n = sws.data_ptr(), nst
    L.call("aid_conv2d", p)
    torch.cuda.synchronize()
    assert "w2d_gemm" in L.lib().aid_last_kernel().decode()
    ref = _conv_ref(x, w, dil, in_scale, 1, out_scale, res, res_scale, alpha)
    err = rel_l2(y.cpu(), ref)
    assert err < tol, err
    assert float(ws[NXI * C * N:].min()) == 7.0
    part = sws.cpu().reshape(B, 8, nst, 2).sum(2)
    yg = y.cpu().double().reshape(B, 8, -1)
    assert rel_l2(part[..., 0], yg.sum(-1)) < 1e-5 and rel_l2(part[..., 1], (yg * yg).sum(-1)) < 1e-6
    # aid_group_stats folds these partials like those of the fused kernels
    gamma = (1.0 + 0.3 * _rand(C, seed=45)).to(DEV)
    sc1, sc2 = torch.empty(B, C, device=DEV), torch.empty(B, C, device=DEV)
    st1, st2 = torch.empty(B, 8, 2, device=DEV), torch.empty(B, 8, 2, device=DEV)
    gws = torch.empty(B * 8 * L.AID_STATS_SPLIT * 2, device=DEV, dtype=torch.float64)
    L.call("aid_group_stats", L.GroupStatsParams(L.view4(y), B, C, Fd, T, 8, gamma.data_ptr(), None, 0, 1e-7, sc1.data_ptr(), st1.data_ptr(), gws.data_ptr(), 0))
    L.call("aid_group_stats", L.GroupStatsParams(L.view4(y), B, C, Fd, T, 8, gamma.data_ptr(), None, 0, 1e-7, sc2.data_ptr(), st2.data_ptr(), sws.data_ptr(), nst))
    assert rel_l2(sc2.cpu(), sc1.cpu()) < 1e-6 and rel_l2(st2.cpu(), st1.cpu()) < 1e-5
    # three runs bit-identical
    y2 = torch.empty_like(y)
    p.y = L.view4(y2)
    L.call("aid_conv2d", p)
    torch.cuda.synchronize()
    assert torch.equal(y, y2)
    cnt = _check_fin_forward(L, p, y, sws, nst, gamma, sc2, st2, "w2d_gemm")
    # (3) reverse sweep: the transposed operator on the gated gradient (no activation), dGELU epilogue, <y, aux> partials, fin_mode = 2
    lay = SimpleNamespace(x=x, w=w, in_scale=in_scale, out_scale=out_scale, xd=xd, wd=wd, isd=isd, osd=osd, alpha=alpha, dil=dil)
    wpT, wpwT = _check_reverse(L, lay, XW, tol, st2, cnt, "w2d_gemm")
    # (4) the pack kernel writes the same 2-D packs as the torch helper
    outs = [torch.empty_like(wp), torch.empty_like(wpT), torch.empty_like(wpw), torch.empty_like(wpwT)]
    pk = (outs[2].data_ptr(), outs[3].data_ptr(), None, None) if tf == 4 else (None, None, outs[2].data_ptr(), outs[3].data_ptr())
    pp = L.PackConvWeightParams(wd.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), None, None, C, C, 5, 3, wp.shape[1], wp.shape[2],
                                wpT.shape[1], wpT.shape[2], None, None, *pk)
    L.call("aid_pack_conv_weight", pp)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], wp) and torch.equal(outs[1], wpT)
    assert rel_l2(outs[2].cpu(), wpw.cpu()) < 1e-7 and rel_l2(outs[3].cpu(), wpwT.cpu()) < 1e-7


def _slice_errs(y, ref):
    """Largest rel-L2 error over thin slices of a [B, C, F, T] result against its fp64 reference: per (b, f) row over all channels and samples (a fault confined to
    one row of one residue class -- the last ragged row tile -- is the whole of such a slice), and per (b, c) over the last eight samples of every row (the last
    group of eight of a row: the last columns of a sample's positions, the ones a ragged GEMM column tile holds)."""
    d = y.double() - ref
    d2, r2 = d * d, ref * ref
    e_row = (d2.sum((1, 3)) / r2.sum((1, 3))).sqrt().max()
    e_tail = (d2[..., -8:].sum((2, 3)) / r2[..., -8:].sum((2, 3))).sqrt().max()
    return float(e_row), float(e_tail)


# The bar of the sliced check on the folded path.  Measured on an MI355X on the six aligned cases of test_conv2d_wino2d_folded_gemm_on_large_launches (whole column
# tiles, whole row tiles, one M tile), with the library of the commit before these tests (they change no kernel): the worst (b, f) row is 5.39e-6, the worst
# (b, co) tail 8.65e-6, beside 3.4e-6 .. 3.9e-6 on the whole tensor (profiles/r11_w2d_fold_edges.txt).  The bar is 4 x the larger = 3.46e-5 (the error of F(4,5)
# depends on the position within a tile, and out_scale[b, co] sets how much of a (b, co) slice is the convolution and how much the exactly-added residual); the
# ceiling of 1e-3 is not reached.  A structural fault in a slice measures 0.1 .. 1.  The edge cases measure at most 5.30e-6 / 9.44e-6.
W2D_FOLD_SLICE_BAR = 4 * 8.65e-6
assert W2D_FOLD_SLICE_BAR <= 1e-3


class _FoldedLayer:
    """One layer on the 80-plane form, large enough for the folded GEMM: inputs (seeded), the input pass's V, the packs, and the launch parameters of
    y = alpha * (res_scale * res + conv(gelu(x in_scale), w) * out_scale)."""

    def __init__(self, L, case):
        self.L = L
        B, Ci, C, Fd, T, dil, self.inst = case
        self.dims, self.dil = (B, Ci, C, Fd, T, dil), dil
        self.N = N = int(L.lib().aid_conv2d_wino2d_positions(B, Fd, T, dil)) // 2
        self.wgs = 10 * ((N + 63) // 64) * ((C + 127) // 128)
        assert self.wgs >= 768
        self.x = _rand(B, Ci, Fd, T, seed=70)
        self.w = _rand(C, Ci, 5, 3, seed=71, scale=1.0 / math.sqrt(Ci * 15))
        self.in_scale, self.out_scale, self.res = 1.0 + 0.5 * _rand(B, Ci, seed=72), _rand(B, C, seed=73), _rand(B, C, Fd, T, seed=74)
        self.alpha, self.res_scale = 1 / math.sqrt(2), 1.5
        self.xd, self.wd, self.isd, self.osd, self.resd = self.x.to(DEV), self.w.to(DEV), self.in_scale.to(DEV), self.out_scale.to(DEV), self.res.to(DEV)
        self.V = torch.empty(80 * Ci * N, device=DEV)
        L.call("aid_scale_act", L.ScaleActParams(L.view4(self.xd), L.View(self.V.data_ptr(), 0, 0, 0), self.isd.data_ptr(), self.isd.stride(0), B, Ci, Fd, T, 1, 4, dil))
        self.wp, self.wpw = L.pack_conv_weight(self.wd), L.pack_conv_weight_wino2d8(self.wd)
        self.ws = torch.full((80 * C * N + 16,), 7.0, device=DEV)
        self.nst = int(L.lib().aid_conv2d_stat_partials(B, Ci, C, Fd, T, dil, 4))
        self.sws = torch.zeros(B * 8 * self.nst * 2, device=DEV, dtype=torch.float64)

    def params(self, y, stats=True):
        L = self.L
        B, Ci, C, Fd, T, dil = self.dims
        p = L.Conv2dParams()
        p.x, p.y, p.res, p.aux = L.View(self.V.data_ptr(), 0, 0, 0), L.view4(y), L.view4(self.resd), L.view4(None)
        p.wp, p.wp_wino, p.wino_taps, p.x_wino = self.wp.data_ptr(), self.wpw.data_ptr(), 80, 4
        p.out_scale, p.out_scale_ld = self.osd.data_ptr(), self.osd.stride(0)
        p.B, p.Cin, p.Cout, p.F, p.T = B, Ci, C, Fd, T
        p.Cin_pad, p.Cout_pad = self.wp.shape[1], self.wp.shape[2]
        p.KH, p.KW, p.dilF, p.act, p.epi = 5, 3, dil, 0, 0
        p.alpha, p.res_scale = self.alpha, self.res_scale
        p.ws, p.ws_bytes = self.ws.data_ptr(), 80 * C * self.N * 4
        if stats:
            p.stat_ws, p.stat_n = self.sws.data_ptr(), self.nst
        return p


def _check_folded_forward(L, case):
    """Forward of a folded launch with gate + residual and the (sum, sum of squares) partials, through aid_conv2d and through the two separate entry points (the same
    bits; the GEMM that ran asserted by name), against the fp64 convolution on the CPU: whole tensor at the budget of the form (2.5e-5) and slice by slice
    (_slice_errs) at W2D_FOLD_SLICE_BAR; the sentinel after ws."""
    s = _FoldedLayer(L, case)
    B, Ci, C, Fd, T, dil = s.dims
    ys = []
    for split_calls in (False, True):
        y = torch.full((B, C, Fd, T), float("nan"), device=DEV)
        p = s.params(y)
        if split_calls:
            L.call("aid_conv2d_wino2d_gemm", p)
            assert s.inst in L.lib().aid_last_kernel().decode(), L.lib().aid_last_kernel().decode()
            L.call("aid_conv2d_wino2d_output", p)
        else:
            L.call("aid_conv2d", p)
        torch.cuda.synchronize()
        ys.append(y)
    assert torch.equal(ys[0], ys[1]) and float(s.ws[80 * C * s.N:].min()) == 7.0
    ref = _conv_ref(s.x.double(), s.w.double(), dil, s.in_scale.double(), 1, s.out_scale.double(), s.res.double(), s.res_scale, s.alpha)
    yc = ys[0].cpu()
    err = rel_l2(yc, ref)
    e_row, e_tail = _slice_errs(yc, ref)
    print(f"folded GEMM {case}: N = {s.N}, {s.wgs} workgroups, rel-L2 vs the fp64 convolution = {err:.2e}, worst (b, f) row {e_row:.2e}, worst (b, co) tail {e_tail:.2e}")
    assert err < 2.5e-5, err
    assert e_row < W2D_FOLD_SLICE_BAR and e_tail < W2D_FOLD_SLICE_BAR, (e_row, e_tail)
    part = s.sws.cpu().reshape(B, 8, s.nst, 2).sum(2)
    yg = yc.double().reshape(B, 8, -1)
    assert rel_l2(part[..., 0], yg.sum(-1)) < 1e-5 and rel_l2(part[..., 1], (yg * yg).sum(-1)) < 1e-6


@pytest.mark.parametrize("case", [(4, 128, 128, 80, 512, 1, "<128x64,foldM,kc32"), (4, 96, 96, 96, 512, 2, "<96x64,foldM,kc24"),
                                  (4, 112, 128, 80, 512, 1, "<128x64,foldM,kc16"), (4, 96, 128, 80, 512, 1, "<128x64,foldM,kc32"),
                                  (4, 112, 96, 96, 512, 2, "<128x64(96),foldM,kc16"), (4, 128, 96, 96, 512, 1, "<128x64(96),foldM,kc32")])
def test_conv2d_wino2d_folded_gemm_on_large_launches(L, case):
    """Launches with >= 768 folded workgroups and Cin <= 128 on the 80-plane form take w2d_gemm_fold_kernel (the row-axis output transform folded into the GEMM: M has
    40 planes) and the FOLD output pass -- the per-shape cases above are too small for it.  Forward with gate + residual and the (sum, sum of squares) partials, through
    aid_conv2d and through the two separate entry points, against the fp64 convolution on the CPU; the kernel that ran is asserted by name: 128-channel panels on
    the four-wave instance with K chunks of 32 (16 where Cin is no multiple of 32), 96-channel panels on the three-wave instance with chunks of 24 or, for other Cin,
    on the four-wave instance with clamped weight columns.  These are the ALIGNED shapes (N a multiple of the 64-column tile, whole row tiles, one M tile): their
    per-slice errors are what W2D_FOLD_SLICE_BAR was measured on."""
    _check_folded_forward(L, case)


W2D_FOLD_EDGE_CASES = [
    # B, Cin, Cout, F, T, dil, instance                               N (N % 64)   workgroups
    (3, 128, 128, 78, 672, 1, "<128x64,foldM,kc32"),              # 5040 (48)    790   ragged column tile, ragged last row tile (R = 78), T > 512 and no multiple of 512
    (3, 128, 128, 80, 544, 8, "<128x64,foldM,kc32"),              # 4896 (32)    770   R = 10, J = 3 in eight residue classes (padding 1.2, the largest the dispatcher takes)
    (3, 96, 96, 100, 544, 2, "<96x64,foldM,kc24"),                # 5304 (56)    830   three-wave instance, ragged both ways (R = 50)
    (2, 128, 256, 38, 992, 1, "<128x64,foldM,kc32"),              # 2480 (48)    780   two M tiles, R = 38
    (2, 128, 192, 38, 992, 1, "<128x64(96),foldM,kc32"),          # 2480 (48)    780   clamped weight columns in the second M tile
    (2, 96, 192, 38, 992, 1, "<96x64,foldM,kc24"),                # 2480 (48)    780   two exact 96-row tiles
    (3, 64, 128, 78, 672, 1, "<128x64,foldM,kc32"),               # 5040 (48)    790   two K chunks per plane: the prologue already holds all of plane 0
    (3, 80, 128, 78, 672, 1, "<128x64,foldM,kc16"),               # 5040 (48)    790   five K chunks per plane
]


def _assert_fold_edges(L, case):
    """What every row of W2D_FOLD_EDGE_CASES claims: enough workgroups to fold, a ragged last column tile, ragged row tiles"""
    B, Ci, C, Fd, T, dil, inst = case
    N = int(L.lib().aid_conv2d_wino2d_positions(B, Fd, T, dil)) // 2
    assert N == B * ((Fd // dil + 3) // 4) * dil * (T // 8)
    assert 10 * ((N + 63) // 64) * ((C + 127) // 128) >= 768
    assert N % 64 != 0
    assert Fd % dil == 0 and (Fd // dil) % 4 != 0
    assert "foldM" in inst
    return N


@pytest.mark.parametrize("case", W2D_FOLD_EDGE_CASES)
def test_conv2d_wino2d_folded_forward_at_the_edges(L, case):
    """The folded GEMM and the FOLD output pass where the aligned cases above do not reach: a ragged last column tile (N % 64 != 0: clamped DMA columns, lanes that
    store nothing), ragged row tiles in the output pass (F / dil no multiple of 4), two M tiles (Cout = 256; Cout = 192 on both 96-panel instances, the four-wave one
    with clamped weight columns and skipped rows), and 2 and 5 K chunks per plane.  The same forward checks at the same budget as the aligned cases, and the sliced
    check: rel-L2 against the fp64 convolution per (b, f) row and per (b, co) over the last eight samples of every row, at W2D_FOLD_SLICE_BAR."""
    _assert_fold_edges(L, case)
    _check_folded_forward(L, case)


@pytest.mark.parametrize("case", [W2D_FOLD_EDGE_CASES[0], W2D_FOLD_EDGE_CASES[2], W2D_FOLD_EDGE_CASES[4]])
def test_conv2d_wino2d_folded_gemm_planes(L, case):
    """What the folded GEMM writes into ws, on its own: exactly the 40 planes M'[j * 10 + xt] = sum_xf AF^T[j][xf] M[xf * 10 + xt] (AF^T of aid_wino45.h), the other
    40 planes of ws and its tail untouched.  Reference: the 80 products U[xi]^T V[xi] in fp64 on the CPU, folded in fp64.  Bar: aid_wino2d_gemm's fp32 M of the same
    U, V folded in fp32 with torch measures E against that reference; the folded kernel does the same arithmetic in another order (plane after plane into four
    accumulators, in registers) and must stay within 2 E -- on the whole tensor, on the columns of the ragged last column tile and on the rows of the last M tile.
    Measured on an MI355X (profiles/r11_w2d_fold_edges.txt), folded kernel / fp32 fold / ratio, whole tensor: case (3, 128, 128, 78, 672, 1) 8.87e-7 / 8.87e-7 / 1.00,
    (3, 96, 96, 100, 544, 2) 7.94e-7 / 7.94e-7 / 1.00, (2, 128, 192, 38, 992, 1) 8.91e-7 / 8.91e-7 / 1.00; the last column tile (8.83e-7, 7.89e-7, 8.79e-7) and the last M
    tile (8.87e-7, 7.94e-7, 8.93e-7) measure the same on both sides, ratio 1.00 throughout."""
    N = _assert_fold_edges(L, case)
    s = _FoldedLayer(L, case)
    B, Ci, C, Fd, T, dil = s.dims
    y = torch.full((B, C, Fd, T), float("nan"), device=DEV)
    p = s.params(y, stats=False)
    L.call("aid_conv2d_wino2d_gemm", p)
    torch.cuda.synchronize()
    assert s.inst in L.lib().aid_last_kernel().decode(), L.lib().aid_last_kernel().decode()
    rest = s.ws[40 * C * N:]
    assert float(rest.min()) == 7.0 and float(rest.max()) == 7.0
    Mf = s.ws[:40 * C * N].reshape(4, 10, C, N)
    M = torch.full((80 * C * N + 16,), 7.0, device=DEV)
    L.call("aid_wino2d_gemm", L.Wino2dGemmParams(s.wpw.data_ptr(), s.V.data_ptr(), M.data_ptr(), 80, Ci, C, s.wp.shape[1], s.wp.shape[2], N, 0))
    torch.cuda.synchronize()
    assert float(M[80 * C * N:].min()) == 7.0
    Mu = M[:80 * C * N].reshape(8, 10, C, N)
    AFT = L.wino45_matrices()[0]                                          # [4, 8]
    assert AFT.shape == (4, 8)
    fold32 = torch.stack([sum(float(AFT[j, xf]) * Mu[xf] for xf in range(8) if AFT[j, xf] != 0) for j in range(4)])      # fp32, plane by plane
    U, V = s.wpw.cpu()[:, :Ci, :C].double().reshape(8, 10, Ci, C), s.V.cpu().double().reshape(8, 10, Ci, N)
    AFTd = torch.from_numpy(AFT)
    ref = torch.stack([torch.einsum("jf,fcn->jcn", AFTd, torch.bmm(U[:, xt].transpose(1, 2), V[:, xt])) for xt in range(10)], dim=1)      # [4, 10, C, N]
    Mf, fold32 = Mf.cpu(), fold32.cpu()
    n_tail, m_tail = N - N % 64, (C - 1) // 128 * 128 if "128x64" in s.inst else (C - 1) // 96 * 96
    for name, sl in (("whole", (Ellipsis,)), ("last column tile", (Ellipsis, slice(n_tail, N))), ("last M tile", (Ellipsis, slice(m_tail, C), slice(None)))):
        e_k, e_t = rel_l2(Mf[sl], ref[sl]), rel_l2(fold32[sl], ref[sl])
        print(f"folded GEMM planes {case} {name}: folded kernel {e_k:.2e}, fp32 fold of the 80-plane M {e_t:.2e} (ratio {e_k / e_t:.2f})")
        assert e_k <= 2 * e_t, (name, e_k, e_t)


W2D_FOLD_REVERSE_CASES = [
    # the forward case, the instance of its transposed launch (Cout -> Cin)
    (W2D_FOLD_EDGE_CASES[0], "<128x64,foldM,kc32"),                                   # 128 -> 128
    (W2D_FOLD_EDGE_CASES[2], "<96x64,foldM,kc24"),                                    # 96 -> 96
    ((4, 128, 96, 96, 512, 1, "<128x64(96),foldM,kc32"), "<128x64,foldM,kc32"),       # aligned, Cin != Cout: 96 -> 128 on another instance than forward
]


@pytest.mark.parametrize("case,inst_rev", W2D_FOLD_REVERSE_CASES)
def test_conv2d_wino2d_folded_reverse_and_fin(L, case, inst_rev):
    """Blocks (2) fin and (3) of test_conv2d_wino2d on folded launches: fin_mode = 1 forward (the same bits as aid_group_stats(ws_n = nst), counters back to zero: its
    fin_total and nblk come from the folded launch's geometry), the transposed operator with epi = 1, aux and the dot_ws partials against torch.autograd.grad of the
    fp64 layer, fin_mode = 2 (the same bits as aid_norm_bwd).  The reverse launch is asserted to fold too: 128 -> 128 and 96 -> 96 for the two ragged cases; the third
    case has Cin != Cout, its transpose 96 -> 128 takes another instance than its forward launch.  The gradient is also checked slice by slice (_slice_errs) at
    W2D_FOLD_SLICE_BAR, the bar measured on the forward launches of the same kernels.  Measured (profiles/r11_w2d_fold_edges.txt): whole tensor 8.7e-6 .. 1.0e-5,
    worst (b, f) row 1.62e-5, worst (b, c) tail 1.42e-5 -- larger than forward because the gradient has no exactly-added residual in its norm."""
    if case in W2D_FOLD_EDGE_CASES:
        _assert_fold_edges(L, case)
    s = _FoldedLayer(L, case)
    B, Ci, C, Fd, T, dil = s.dims
    assert "foldM" in inst_rev and (Ci == C) == (inst_rev == s.inst)
    assert L.lib().aid_conv2d_fin_supported(B, Ci, C, Fd, T, dil, 4) == 1
    y = torch.full((B, C, Fd, T), float("nan"), device=DEV)
    p = s.params(y)
    L.call("aid_conv2d", p)
    torch.cuda.synchronize()
    assert s.inst in L.lib().aid_last_kernel().decode(), L.lib().aid_last_kernel().decode()
    assert bool(torch.isfinite(y).all())
    gamma = (1.0 + 0.3 * _rand(C, seed=45)).to(DEV)
    sc2, st2 = torch.empty(B, C, device=DEV), torch.empty(B, 8, 2, device=DEV)
    L.call("aid_group_stats", L.GroupStatsParams(L.view4(y), B, C, Fd, T, 8, gamma.data_ptr(), None, 0, 1e-7, sc2.data_ptr(), st2.data_ptr(), s.sws.data_ptr(), s.nst))
    cnt = _check_fin_forward(L, p, y, s.sws, s.nst, gamma, sc2, st2, s.inst)
    # the statistics of x for aid_norm_bwd (fin_mode = 2 folds with the same ones)
    gx = torch.ones(Ci, device=DEV)
    scx, stx = torch.empty(B, Ci, device=DEV), torch.empty(B, 8, 2, device=DEV)
    gws = torch.empty(B * 8 * L.AID_STATS_SPLIT * 2, device=DEV, dtype=torch.float64)
    L.call("aid_group_stats", L.GroupStatsParams(L.view4(s.xd), B, Ci, Fd, T, 8, gx.data_ptr(), None, 0, 1e-7, scx.data_ptr(), stx.data_ptr(), gws.data_ptr(), 0))
    _check_reverse(L, s, 4, 2.5e-5, stx, cnt, inst_rev, ref_dtype=torch.float64, slice_bar=W2D_FOLD_SLICE_BAR)


@pytest.mark.parametrize("case", [(1, 64, 8, 2016, 1, 4), (1, 64, 8, 2032, 2, 3)])
def test_w2d_input_pass_at_the_lds_limit(L, case):
    """Rows longer than 512 samples that are no multiple of 512 are not cut into T segments: one workgroup of the input pass holds whole rows, 4 JB + 4 = 8 of them
    at JB = 1 -- 64 512 bytes of LDS at T = 2016 (F(8,3) along T) and 65 024 at T = 2032 (F(4,3)), the two longest rows aid_conv2d_wino2d_supported accepts short
    of 2048, right under the 64-KiB ceiling.  Against the definition (_input_ref) at the bar of the other shapes, with the sentinel after V."""
    B, C, Fd, T, dil, XW = case
    tf, NXI = (4, 48) if XW == 3 else (8, 80)
    assert L.lib().aid_conv2d_wino2d_supported(C, 128, Fd, T, dil) and T % (4 * tf) == 0      # (the pass's channels are the layer's Cin; it never sees Cout: any the form takes)
    assert T > 512 and T % 512 != 0
    assert 63 * 1024 <= 8 * T * 4 <= 64 * 1024
    N = int(L.lib().aid_conv2d_wino2d_positions(B, Fd, T, dil)) * 4 // tf
    x = _rand(B, C, Fd, T, seed=80)
    in_scale = 1.0 + 0.5 * _rand(B, C, seed=81)
    xd, isd = x.to(DEV), in_scale.to(DEV)
    V = torch.full((NXI * C * N + 16,), 7.0, device=DEV)
    L.call("aid_scale_act", L.ScaleActParams(L.view4(xd), L.View(V.data_ptr(), 0, 0, 0), isd.data_ptr(), isd.stride(0), B, C, Fd, T, 1, XW, dil))
    torch.cuda.synchronize()
    assert float(V[NXI * C * N:].min()) == 7.0 and float(V[NXI * C * N:].max()) == 7.0
    Vref = _input_ref(F.gelu(x * in_scale[:, :, None, None]), dil, tf)
    err = rel_l2(V[:NXI * C * N].cpu().reshape(NXI, C, N), Vref)
    print(f"input pass {case}: slab {8 * T * 4} bytes, rel-L2 vs the definition = {err:.2e}")
    assert err < 1e-6, err
