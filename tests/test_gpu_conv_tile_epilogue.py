"""The tile frame and the two epilogues the position-tiled conv kernels share (csrc/aid_conv_tile.h), kernel by kernel.

A deterministic grid: each of the four 5x3 kernels that run the shared scalar or F(4,3) epilogue, times the epilogue options, on the smallest
shapes at which the frame can still go wrong -- T not a power of two (zero-page columns), B * F not a multiple of the rows of a tile (rows with
b = -1 in the last tile), at least two Cout tiles, Cout below its padded width (masked rows), y a channel slice of a sentinel-filled buffer.
Every case asserts through aid_last_kernel that the intended kernel took the launch.  Reference and bounds as test_conv2d_dispatch_fuzz:
fp64 conv2d on the CPU, rel-L2 below 2e-5, dot partials within 1e-5 of the absolute-product sum, sentinel untouched.

The dot partials are defined only where a tile stays inside one sample (F a multiple of the rows of a tile) and Cout / 8 is a multiple of 4,
so those cases have F = 16 and an unpadded Cout; the others keep the ragged last tile and the masked rows.
"""
import functools
import math

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


# kernel id -> (noted name, how the launch is steered to it)
#   mfma   : in_scale given, so neither direct-to-LDS 5x3 kernel is eligible
#   dma    : no prologue, no Winograd pack
#   wino4  : 30-tap pack, plain input (x_wino = 0)
#   wino4v : 30-tap pack, Winograd-domain input (x_wino = 1) on geometries the row-shared kernel declines (T = 48 has no row-shared tile; nor has T = 32 with 96 channels)
RAGGED = {
    # B, Cin, Cout, F, T, dil: T = 12 -> TT = 16, 16 rows per 256-position tile, B * F = 27 rows; Cout 100 -> two 64-wide tiles, 136 -> five 32-wide ones
    ("mfma", "conv_mfma_kernel(5x3)"): (3, 40, 136, 9, 12, 2),
    ("dma", "conv53_dma_kernel"): (3, 64, 100, 9, 12, 2),
    ("wino4", "conv53_wino4_kernel(64x256)"): (3, 64, 100, 9, 12, 2),
    # T = 48 -> TT = 64: 8 rows per 512-position tile (96-wide, Cout 72 of 96), 4 rows per 256-position tile (64-wide, Cout 100 of 128)
    ("wino4", "conv53_wino4_kernel(96)"): (3, 64, 72, 9, 48, 2),
    ("wino4v", "conv53_wino4v_kernel(64x256)"): (3, 64, 100, 9, 48, 1),
    ("wino4v", "conv53_wino4v_kernel(96)"): (3, 64, 72, 9, 48, 2),
}
DOT = {
    ("wino4", "conv53_wino4_kernel(64x256)"): [(3, 64, 128, 16, 12, 2)],
    ("wino4", "conv53_wino4_kernel(96)"): [(2, 64, 96, 16, 48, 2)],
    ("wino4v", "conv53_wino4v_kernel(64x256)"): [(3, 64, 128, 16, 48, 1)],
    ("wino4v", "conv53_wino4v_kernel(96)"): [(2, 64, 96, 16, 48, 2), (2, 64, 96, 16, 32, 2)],
}
CASES = [(k, g, opt) for k, g in RAGGED.items() for opt in ("plain", "alias", "dgelu")] + [(k, g, "dot") for k, gs in DOT.items() for g in gs]


@functools.lru_cache(maxsize=None)
def _inputs(geo, scaled):
    """seeded inputs of a geometry and the fp64 convolution of them (computed once, shared by the options; never modified)"""
    B, Cin, Cout, Fd, T, dil = geo
    g = torch.Generator().manual_seed(20261021 + sum(v * 131 ** i for i, v in enumerate(geo)) % 100003)
    x = torch.randn(B, Cin, Fd, T, generator=g)
    w = torch.randn(Cout, Cin, 5, 3, generator=g) / math.sqrt(Cin * 15)
    in_scale = (1.0 + 0.5 * torch.randn(B, Cin, generator=g)) if scaled else None
    out_scale = torch.randn(B, Cout, generator=g)
    res = torch.randn(B, Cout, Fd, T, generator=g)
    aux = torch.randn(B, Cout, Fd, T, generator=g)
    asc = 1.0 + 0.3 * torch.randn(B, Cout, generator=g)
    h = x.double() * (in_scale.double()[:, :, None, None] if scaled else 1.0)
    conv = F.conv2d(h, w.double(), padding="same", dilation=(dil, 1))
    return x, w, in_scale, out_scale, res, aux, asc, conv


def launch_case(L, kern, geo, opt):
    """one launch of the grid: (noted kernel, y, the sentinel buffer y is a slice of, dot partials or None, P, fp64 reference, aux)"""
    (kind, noted), (B, Cin, Cout, Fd, T, dil) = kern, geo
    x, w, in_scale, out_scale, res, aux, asc, conv = _inputs(geo, kind == "mfma")
    epi = opt in ("dgelu", "dot")
    use_out = opt in ("alias", "dgelu", "dot")
    alpha, res_scale = {"plain": (1.0, 1.0), "alias": (0.7071, 1.5), "dgelu": (0.7071, 1.0), "dot": (0.7, 1.0)}[opt]
    ref = conv
    if use_out:
        ref = ref * out_scale.double()[:, :, None, None]
    if epi:
        u = aux.double() * asc.double()[:, :, None, None]
        ref = ref * (0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi))
    if opt == "alias":
        ref = ref + res_scale * res.double()
    ref = alpha * ref

    xd, wd = x.to(DEV), w.to(DEV)
    wp = L.pack_conv_weight(wd)
    if opt != "dot":
        assert Cout < wp.shape[2], "the ragged geometries are meant to mask rows m >= Cout"
        assert (B * Fd) % 2 == 1 and T <= 64, "... and to leave rows with b = -1 in the last tile (an odd row count, tiles of 4 ... 16 rows)"
    ybig = torch.full((B, Cout + 8, Fd, T), 7.0, device=DEV)
    y = ybig[:, 4:4 + Cout]                                  # channel slice of the sentinel-filled buffer (16-byte aligned offset)
    resd = None
    if opt == "alias":                                       # the residual IS the output buffer
        y.copy_(res.to(DEV))
        resd = y
    keep = [t.to(DEV) if use else None for t, use in ((in_scale, kind == "mfma"), (out_scale, use_out), (aux, epi), (asc, epi))]
    xin = xd
    if kind == "wino4v":
        assert L.lib().aid_conv2d_wino_input_ok(B, Cin, Cout, Fd, T, dil)
        xin = torch.empty(B, Cin, Fd, 6 * (T // 4), device=DEV)
        L.call("aid_scale_act", L.ScaleActParams(L.view4(xd), L.view4(xin), None, 0, B, Cin, Fd, T, 0, 1))
    p = L.Conv2dParams()
    p.x, p.y, p.res, p.aux = L.view4(xin), L.view4(y), L.view4(resd), L.view4(keep[2])
    p.wp = wp.data_ptr()
    p.in_scale, p.in_scale_ld = L.ptr(keep[0]), (0 if keep[0] is None else keep[0].stride(0))
    p.out_scale, p.out_scale_ld = L.ptr(keep[1]), (0 if keep[1] is None else keep[1].stride(0))
    p.aux_scale, p.aux_scale_ld = L.ptr(keep[3]), (0 if keep[3] is None else keep[3].stride(0))
    p.B, p.Cin, p.Cout, p.F, p.T = B, Cin, Cout, Fd, T
    p.Cin_pad, p.Cout_pad = wp.shape[1], wp.shape[2]
    p.KH, p.KW, p.dilF, p.act, p.epi = 5, 3, dil, 0, int(epi)
    p.alpha, p.res_scale = alpha, res_scale
    p.x_wino = int(kind == "wino4v")
    wpw = None
    if kind in ("wino4", "wino4v"):
        wpw = L.pack_conv_weight_wino(wd)
        p.wp_wino, p.wino_taps = wpw.data_ptr(), 30
    P, dws = 0, None
    if opt == "dot":
        P = int(L.lib().aid_conv2d_dot_partials(B, Cin, Cout, Fd, T, dil, p.x_wino))
        assert P > 0
        dws = torch.full((B * 8 * (P + 1),), float("nan"), device=DEV, dtype=torch.float64)
        p.dot_ws, p.dot_n = dws.data_ptr(), P
    L.call("aid_conv2d", p)
    torch.cuda.synchronize()
    return L.lib().aid_last_kernel().decode(), y, ybig, dws, P, ref, aux


@pytest.mark.parametrize("kern,geo,opt", CASES, ids=[f"{k[1]}-{'x'.join(map(str, g))}-{o}" for k, g, o in CASES])
def test_shared_conv_epilogues(L, kern, geo, opt):
    B, Cin, Cout, Fd, T, dil = geo
    noted, y, ybig, dws, P, ref, aux = launch_case(L, kern, geo, opt)
    assert noted == kern[1]
    yc = y.cpu().double()
    e = rel_l2(yc, ref)
    print(f"{noted} {geo} {opt}: rel-L2 {e:.2e}")
    assert e < 2e-5, f"rel-L2 {e:.2e}"
    assert float(ybig[:, :4].min()) == 7.0 and float(ybig[:, :4].max()) == 7.0, "wrote below its channel slice"
    assert float(ybig[:, 4 + Cout:].min()) == 7.0 and float(ybig[:, 4 + Cout:].max()) == 7.0, "wrote above its channel slice"
    if P:
        assert bool(torch.isnan(dws[B * 8 * P:]).all()), "wrote past the partial slots"
        got = dws[:B * 8 * P].cpu().reshape(B, 8, P).sum(-1)
        want = (yc * aux.double()).reshape(B, 8, Cout // 8, Fd, T).sum((2, 3, 4))
        scale = float((yc.abs() * aux.double().abs()).reshape(B, 8, -1).sum(-1).max())
        assert bool(torch.isfinite(got).all()) and float((got - want).abs().max()) < 1e-5 * scale, "dot partials"
