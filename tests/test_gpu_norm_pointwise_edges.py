"""The normalisation and pointwise kernels of csrc/aid_norm.hip and aid_add2 (csrc/aid_sampler.hip), each directly against a float64 reference of
the same operation on the same float32 inputs: aid_group_stats, aid_group_dot, aid_norm_bwd (plain, F(4,3) and F(8,3) Winograd-domain copy),
aid_scale_act (plain, F(4,3), F(8,3)) and aid_add2 at the edges of their shared thread-to-sample mapping (lpr = pow2ceil(T/4) capped at 256,
rpb = 256 / lpr rows per block, tiles = cdiv(T/4, lpr)): one lane per row, dead lanes inside a row, a ragged last tile with lpr = 256, a row count
that is no multiple of rpb, neighbour samples across a wave and across a block boundary, group counts other than 8, channel slices of padded
parents (a sentinel around and between the rows, exact), NaN pre-fills, hand-made fp64 partials, a constant group and the refusals.

Bounds: 1e-5 rel-L2 for the reductions (header of test_gpu_kernels.py), 1e-6 where the issue of this file sets it (cancellation, hand-made
partials).  Elementwise results are held to a max-abs error of FOUR times that of the same formula evaluated in float32 on the CPU (torch, same
operand order) against the float64 reference, on the case's own inputs; Winograd-domain outputs plane by plane, relative to the plane's
max |reference| -- one wrong edge sample per row would vanish in a whole-tensor rel-L2.  Every case prints its figures
(profiles/r32_norm_pointwise_sampler_edges.txt)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
SENT = 123.0          # around and between the rows of an output: must survive
BIG = 3.0e4           # around and between the rows of an input: would wreck every result if read
FLAT = (0, 0, 0)


@pytest.fixture(scope="module")
def L():
    from audio_inpainting_diffusion_amd import _lib
    _lib.lib()
    return _lib


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def f32(v):
    """a host scalar as the float the parameter block carries"""
    return float(np.float32(v))


EPS = f32(1e-7)


class Par:
    """a [B, C, F, T] view at [:, off:off+C, :F, :T] of a parent padded by ``pad`` = (channels, rows, samples; samples % 4 == 0) and filled with ``fill``"""

    def __init__(self, shape, pad=(5, 1, 4), off=3, fill=SENT, data=None):
        B, C, Fd, T = shape
        off = min(off, pad[0])
        self.fill, self.sl = fill, (slice(None), slice(off, off + C), slice(0, Fd), slice(0, T))
        self.buf = torch.full((B, C + pad[0], Fd + pad[1], T + pad[2]), fill, device=DEV)
        self.v = self.buf[self.sl]
        if data is not None:
            self.v.copy_(data)

    def untouched(self):
        t = self.buf.clone()
        t[self.sl] = self.fill
        return bool((t == self.fill).all())


class WRows:
    """Winograd-domain rows [B, C, F, n, G] with row stride n * G + 4 inside a parent padded by two channels and one row, all SENT; planes NaN"""

    def __init__(self, B, C, Fd, n, G):
        self.nG, self.shape = n * G, (B, C, Fd, n, G)
        self.buf = torch.full((B, C + 2, Fd + 1, n * G + 4), SENT, device=DEV)
        self.v = self.buf[:, 1:1 + C, :Fd, :]
        self.v[..., :self.nG] = NAN

    def planes(self):
        return self.v[..., :self.nG].reshape(self.shape).cpu()

    def untouched(self):
        t = self.buf.clone()
        t[:, 1:1 + self.shape[1], :self.shape[2], :self.nG] = SENT
        return bool((t == SENT).all())


def _guarded(n, fill, dtype=torch.float32):
    """n values pre-filled with ``fill`` between two SENT values: (whole buffer, the n values)"""
    buf = torch.full((n + 2,), SENT, device=DEV, dtype=dtype)
    buf[1:-1] = fill
    return buf, buf[1:-1]


def _guards_ok(buf):
    return float(buf[0]) == SENT and float(buf[-1]) == SENT


def _check_abs(tag, got, ref, cpu32, per_plane_dim=None):
    """max-abs error of the kernel against four times that of the float32 CPU evaluation (module docstring); with ``per_plane_dim`` plane by plane,
    relative to the plane's max |reference|"""
    got, cpu32 = got.double(), cpu32.double()
    assert bool(torch.isfinite(got).all()), tag
    if per_plane_dim is None:
        e_gpu, e_cpu = float((got - ref).abs().max()), float((cpu32 - ref).abs().max())
        print(f"{tag}: max |err| kernel {e_gpu:.2e} fp32-cpu {e_cpu:.2e} bound {4 * e_cpu:.2e}")
        assert e_gpu <= 4 * e_cpu, tag
        return
    dims = [d for d in range(ref.dim()) if d != per_plane_dim]
    den = ref.abs().amax(dims)
    e_gpu, e_cpu = (got - ref).abs().amax(dims) / den, (cpu32 - ref).abs().amax(dims) / den
    print(f"{tag}: per plane max |err| / max |ref|: kernel " + " ".join(f"{float(e):.1e}" for e in e_gpu) + " | fp32-cpu "
          + " ".join(f"{float(e):.1e}" for e in e_cpu) + " (bound: 4 x)")
    assert bool((e_gpu <= 4 * e_cpu).all()), tag


# ---------------------------------------------------------------------------------------------------------
# float64 references
def _group_ref(x, gamma, mod, groups):
    """(mean [B, G], inv [B, G], scale [B, C]): n = cg F T, inv = 1 / (unbiased std + eps), scale = gamma (1 + mod) inv"""
    B, C = x.shape[:2]
    xg = x.double().reshape(B, groups, -1)
    mean, inv = xg.mean(-1), 1.0 / (xg.std(-1) + EPS)
    m = 1.0 if mod is None else 1.0 + mod.double()
    return mean, inv, gamma.double()[None] * m * inv.repeat_interleave(C // groups, dim=1)


def _gelu64(h):
    return 0.5 * h * (1.0 + torch.erf(h / np.sqrt(2.0)))


def _gelu32(h):
    return 0.5 * h * (1.0 + torch.erf(h * 0.70710678118654752440))


# B^T of F(4,3) over {0, +-1, +-2, inf} as the fused 1-D kernels use it
BT4 = torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]],
                   dtype=torch.float64)


def _bt(m):
    if m == 4:
        return BT4
    from audio_inpainting_diffusion_amd import winograd
    return torch.from_numpy(winograd.cook_toom(winograd.W8_POINTS, 8, 3)[2])


def _groups_of(h, m):
    """[..., T] -> [..., T/m, m + 2]: samples m g - 1 .. m g + m of every group, zero outside [0, T)"""
    return F.pad(h, (1, 1)).unfold(-1, m + 2, m)


def _wino64(h, m):
    """float64 input transform along T: [..., T] -> [..., m + 2, T/m]"""
    return torch.einsum("xk,...gk->...xg", _bt(m), _groups_of(h.double(), m))


def _wino32(h, m):
    """the same in float32 in the kernels' operand order: F(4,3) as the six expressions of aid_kernels.h, F(8,3) as aid_wino8_input -- per row the
    even-sample terms left to right, the odd-sample terms left to right, then their sum"""
    d = _groups_of(h.float(), m)
    e = [d[..., k] for k in range(m + 2)]
    if m == 4:
        s12, m12, m42, m31 = e[1] + e[2], e[1] - e[2], e[4] - e[2], e[3] - e[1]
        V = [4 * e[0] - 5 * e[2] + e[4], (e[3] + e[4]) - 4 * s12, (e[4] - e[3]) + 4 * m12, m42 + 2 * m31, m42 - 2 * m31, 4 * e[1] - 5 * e[3] + e[5]]
        return torch.stack(V, dim=-2)
    bt = _bt(8).float()
    V = []
    for r in range(10):
        parts = []
        for cols in (range(0, 10, 2), range(1, 10, 2)):
            acc = None
            for c in cols:
                if float(bt[r, c]) != 0.0:
                    acc = bt[r, c] * e[c] if acc is None else acc + bt[r, c] * e[c]
            if acc is not None:
                parts.append(acc)
        V.append(parts[0] if len(parts) == 1 else parts[0] + parts[1])
    return torch.stack(V, dim=-2)


# ---------------------------------------------------------------------------------------------------------
# aid_group_stats, aid_group_dot
def _stats_run(L, xv, shape, groups, gamma, mod=None, mod_ld=0, want_stats=True, ws=None, ws_n=0):
    B, C, Fd, T = shape
    sbuf, scale = _guarded(B * C, NAN)
    tbuf, stats = _guarded(B * groups * 2, NAN)
    if ws is None:
        ws = torch.full((B * groups * L.AID_STATS_SPLIT * 2,), NAN, device=DEV, dtype=torch.float64)
    p = L.GroupStatsParams(L.view4(xv), B, C, Fd, T, groups, gamma.data_ptr(), L.ptr(mod), mod_ld, EPS, scale.data_ptr(),
                           stats.data_ptr() if want_stats else None, ws.data_ptr(), ws_n)
    L.call("aid_group_stats", p)
    torch.cuda.synchronize()
    assert _guards_ok(sbuf) and _guards_ok(tbuf)
    return scale.reshape(B, C).cpu(), stats.reshape(B, groups, 2).cpu()


def _dot_run(L, uv, vv, shape, groups, tail=0):
    """aid_group_dot into [B groups][SPLIT] doubles (NaN pre-filled, ``tail`` more doubles behind them for aid_norm_bwd's coefficients)"""
    B, C, Fd, T = shape
    n = B * groups * L.AID_STATS_SPLIT
    ws = torch.full((n + tail + 1,), NAN, device=DEV, dtype=torch.float64)
    ws[-1] = SENT
    L.call("aid_group_dot", L.GroupDotParams(L.view4(uv), L.view4(vv), B, C, Fd, T, groups, ws.data_ptr()))
    torch.cuda.synchronize()
    assert float(ws[-1]) == SENT and (tail == 0 or bool(torch.isnan(ws[n:-1]).all()))
    return ws


STATS_CASES = [((2, 8, 3, 4), 8),          # lpr = 1, 64 rows per pass; nrows = 3 < AID_STATS_SPLIT: most splits are empty
               ((2, 16, 5, 12), 1),        # one group of everything; three of four lanes live
               ((1, 64, 2, 48), 64),       # cg = 1; 16 group trips per wave in the final kernel
               ((1, 8, 3, 1040), 4),       # lpr = 256, the second trip along a row is ragged (260 float4)
               ((1, 264, 2, 16), 8)]       # C > 256: second trip of the per-channel loop of the final kernel


@pytest.mark.parametrize("shape,groups", STATS_CASES)
def test_group_stats_and_dot(L, shape, groups):
    B, C, Fd, T = shape
    x = _rand(*shape, seed=11, scale=3.0) + 0.5
    u = _rand(*shape, seed=12)
    v = u + 0.5 * _rand(*shape, seed=13)                            # <u, v> ~ |u|^2: far from zero against |u| |v|
    gamma = 1.0 + 0.3 * _rand(C, seed=14)
    mod = 0.5 * _rand(B, C, seed=15)
    gd_ = gamma.to(DEV)
    modw = torch.full((B, C + 7), BIG, device=DEV)
    modw[:, 2:2 + C] = mod.to(DEV)
    xc, xs = x.to(DEV), Par(shape, fill=BIG, data=x)
    mean, inv, scale_nomod = _group_ref(x, gamma, None, groups)
    scale_mod = _group_ref(x, gamma, mod, groups)[2]
    # contiguous, mod = NULL
    sc, st = _stats_run(L, xc, shape, groups, gd_)
    errs = [rel_l2(sc, scale_nomod), rel_l2(st[..., 0], mean), rel_l2(st[..., 1], inv)]
    # channel slice of a padded parent, mod with mod_ld > C
    sc2, st2 = _stats_run(L, xs.v, shape, groups, gd_, modw[:, 2:], modw.stride(0))
    errs += [rel_l2(sc2, scale_mod), rel_l2(st2[..., 0], mean), rel_l2(st2[..., 1], inv)]
    assert torch.equal(st, st2)                                     # same values through other strides: the same bits (fixed reduction order)
    # stats = NULL: the same scale, nothing else written (the guards around `stats` hold, its NaN pre-fill stays)
    sc3, st3 = _stats_run(L, xs.v, shape, groups, gd_, modw[:, 2:], modw.stride(0), want_stats=False)
    assert torch.equal(sc3, sc2) and bool(torch.isnan(st3).all())
    print(f"group_stats {shape} g={groups}: scale {errs[0]:.2e} mean {errs[1]:.2e} inv {errs[2]:.2e} | strided + mod: scale {errs[3]:.2e} "
          f"mean {errs[4]:.2e} inv {errs[5]:.2e}", end="")
    assert all(bool(torch.isfinite(t).all()) for t in (sc, st, sc2)) and max(errs) < 1e-5
    # aid_group_dot: the SPLIT partials per (b, g) summed on the host in float64
    ref = (u.double() * v.double()).reshape(B, groups, -1).sum(-1)
    us, vs = Par(shape, fill=BIG, data=u), Par(shape, pad=(2, 3, 8), off=1, fill=BIG, data=v)
    e = []
    for uv, vv in ((u.to(DEV), v.to(DEV)), (us.v, vs.v)):
        ws = _dot_run(L, uv, vv, shape, groups)
        got = ws[:-1].reshape(B, groups, L.AID_STATS_SPLIT).sum(-1).cpu()
        assert bool(torch.isfinite(got).all())
        e.append(rel_l2(got, ref))
    print(f" | group_dot contiguous {e[0]:.2e} strided {e[1]:.2e}")
    assert max(e) < 1e-5


def test_group_stats_cancellation(L):
    """mean 100, std 1e-2: E[x^2] - E[x]^2 loses eight digits.  In fp64 that leaves 5e-9 (CPU emulation of the two-moment form on this input); fp32
    accumulation would be off by order 1.  Bound: 1e-6."""
    shape, groups = (2, 16, 5, 64), 8
    x = 100.0 + 1e-2 * _rand(*shape, seed=21)
    gamma = 1.0 + 0.3 * _rand(16, seed=22)
    mean, inv, scale = _group_ref(x, gamma, None, groups)
    n = 2 * 5 * 64
    s, ss = x.double().reshape(2, groups, -1).sum(-1), (x.double() ** 2).reshape(2, groups, -1).sum(-1)
    emu = 1.0 / (((ss - n * (s / n) ** 2) / (n - 1)).clamp_min(0).sqrt() + EPS)
    sc, st = _stats_run(L, x.to(DEV), shape, groups, gamma.to(DEV))
    e = [rel_l2(st[..., 1], inv), rel_l2(sc, scale), rel_l2(st[..., 0], mean)]
    print(f"group_stats cancellation: fp64 two-moment emulation {rel_l2(emu, inv):.2e}; kernel inv {e[0]:.2e} scale {e[1]:.2e} mean {e[2]:.2e}")
    assert bool(torch.isfinite(sc).all()) and max(e) < 1e-6


def _partials(total, k, seed):
    """[...] float64 -> [..., k] float64 partials of mixed sign and size that sum (in float64) to ``total``"""
    w = _rand(*total.shape, k, seed=seed).double()
    w[..., -1] = 1.0 - w[..., :-1].sum(-1)
    return total[..., None] * w


# ---------------------------------------------------------------------------------------------------------
# aid_norm_bwd
def _nb_case(L, shape, groups, seed, const_group=None, a=0.75):
    """inputs, the forward statistics as the DEVICE wrote them (float32, so that the reference coefficient is about aid_norm_bwd alone) and the
    float64 / float32-CPU evaluations of  out = gd - coef (x - mean) + a gy (+ old),  coef = <gd, x>_g inv / ((n - 1) std),  std = 1 / inv - eps"""
    B, C, Fd, T = shape
    cg = C // groups
    x = _rand(*shape, seed=seed, scale=2.0) + 0.5
    if const_group is not None:
        x[:, const_group * cg:(const_group + 1) * cg] = 0.75       # (n * 0.75 and n * 0.5625 are exact in fp64: the variance is exactly 0)
    gd, gy = _rand(*shape, seed=seed + 1), _rand(*shape, seed=seed + 2)
    gamma = torch.ones(C, device=DEV)
    scale, stats = _stats_run(L, x.to(DEV), shape, groups, gamma)
    n = cg * Fd * T
    mean, inv = stats[..., 0].double(), stats[..., 1].double()
    sd = 1.0 / inv - EPS
    dot = (gd.double() * x.double()).reshape(B, groups, -1).sum(-1)
    coef = torch.where(sd > 0, dot * inv / ((n - 1.0) * sd), torch.zeros_like(dot))
    ex = lambda t: t.repeat_interleave(cg, dim=1)[:, :, None, None]

    def ref(with_gy, old=0.0):
        r64 = gd.double() - ex(coef) * (x.double() - ex(mean))
        r32 = gd - ex(coef.float()) * (x - ex(stats[..., 0]))
        if with_gy:
            r64, r32 = r64 + a * gy.double(), r32 + a * gy
        return r64 + old, r32 + old
    return dict(shape=shape, groups=groups, x=x, gd=gd, gy=gy, a=a, stats=stats, stats_dev=stats.to(DEV).contiguous(), ref=ref, dot=dot, scale=scale)


def _nb_run(L, c, gdv, xv, gyv, outv, accumulate=0, ws=None, ws_n=0, wout=None, wscale=None, wscale_ld=0, wform=0):
    B, C, Fd, T = c["shape"]
    g = c["groups"]
    if ws is None:
        ws = _dot_run(L, c["gd"].to(DEV), c["x"].to(DEV), c["shape"], g, tail=B * g)
    p = L.NormBwdParams(L.view4(gdv), L.view4(xv), L.view4(gyv), L.view4(outv), B, C, Fd, T, g, c["stats_dev"].data_ptr(), ws.data_ptr(), EPS, c["a"],
                        accumulate, ws_n, L.view4(wout), L.ptr(wscale), wscale_ld, wform, 0, 1)
    L.call("aid_norm_bwd", p)
    torch.cuda.synchronize()
    return ws


PADS = [((5, 1, 4), 3), ((2, 3, 8), 1), ((1, 0, 12), 1), ((7, 2, 4), 4)]       # gd, x, gy, out: four different parents


@pytest.mark.parametrize("shape,groups", [((2, 8, 3, 4), 2), ((2, 16, 5, 12), 16), ((1, 8, 2, 48), 8), ((1, 8, 1, 1040), 4)])
def test_norm_bwd_plain(L, shape, groups):
    c = _nb_case(L, shape, groups, seed=31)
    dev = {k: c[k].to(DEV) for k in ("gd", "x", "gy")}
    for with_gy in (False, True):
        for accumulate in (0, 1):
            old = 0.25 if accumulate else 0.0
            r64, r32 = c["ref"](with_gy, old)
            out = Par(shape, pad=FLAT)
            out.v.fill_(0.25 if accumulate else NAN)
            _nb_run(L, c, dev["gd"], dev["x"], dev["gy"] if with_gy else None, out.v, accumulate)
            _check_abs(f"norm_bwd {shape} g={groups} gy={int(with_gy)} acc={accumulate}", out.v.cpu(), r64, r32)
    # every operand a slice of its own padded parent
    ins = [Par(shape, pad=pd, off=o, fill=BIG, data=c[k]) for k, (pd, o) in zip(("gd", "x", "gy"), PADS)]
    for accumulate in (0, 1):
        r64, r32 = c["ref"](True, 0.25 if accumulate else 0.0)
        out = Par(shape, pad=PADS[3][0], off=PADS[3][1])
        out.v.fill_(0.25 if accumulate else NAN)
        _nb_run(L, c, ins[0].v, ins[1].v, ins[2].v, out.v, accumulate)
        assert out.untouched()
        _check_abs(f"norm_bwd {shape} g={groups} strided acc={accumulate}", out.v.cpu(), r64, r32)


def test_norm_bwd_constant_group(L):
    """one group of x is constant: std = 0, inv = 1 / eps, scale and stats finite; aid_norm_bwd then writes exactly gd + a gy there (x - mean is
    exactly 0 and the coefficient finite, or 0 where 1 / inv - eps <= 0), and no NaN or Inf anywhere.  a = 0.5: a gy is exact, so the sum has one
    rounding whether or not the compiler contracts it into an fma."""
    shape, groups = (2, 16, 5, 64), 8
    c = _nb_case(L, shape, groups, seed=41, const_group=3, a=0.5)
    st = c["stats"]
    assert bool(torch.isfinite(st).all()) and bool(torch.isfinite(c["scale"]).all())
    assert bool((st[:, 3, 0] == 0.75).all()) and bool((st[:, 3, 1] == np.float32(1.0 / EPS)).all())
    assert bool((c["scale"][:, 6:8] == np.float32(1.0 / EPS)).all())                                  # gamma = 1, mod = NULL
    out = Par(shape)
    out.v.fill_(NAN)
    ws = _nb_run(L, c, c["gd"].to(DEV), c["x"].to(DEV), c["gy"].to(DEV), out.v)
    coef = ws[2 * groups * L.AID_STATS_SPLIT:-1].view(torch.float32)[:2 * groups].cpu().reshape(2, groups)
    got = out.v.cpu()
    print(f"norm_bwd constant group: inv = {float(st[0, 3, 1]):.6e}, coefficients there {coef[:, 3].tolist()}")
    assert out.untouched() and bool(torch.isfinite(got).all()) and bool(torch.isfinite(coef).all())
    assert torch.equal(got[:, 6:8], c["gd"][:, 6:8] + c["a"] * c["gy"][:, 6:8])
    r64, r32 = c["ref"](True)
    keep = [ch for ch in range(16) if ch not in (6, 7)]
    _check_abs("norm_bwd constant group, the other groups", got[:, keep], r64[:, keep], r32[:, keep])


@pytest.mark.parametrize("ws_n", [1, 65, 130])       # one partial; one full trip of the 64 lanes + 1; two trips + 2
def test_hand_made_partials(L, ws_n):
    """ws_n > 0 with partials the test wrote (fp64, mixed signs, summing to the true moments / dots): the lane loops of group_stats_final and
    norm_bwd_coef without a convolution; results equal those of ws_n = 0 to 1e-6"""
    shape, groups = (2, 16, 3, 48), 8
    B, C, Fd, T = shape
    c = _nb_case(L, shape, groups, seed=51)
    gamma = (1.0 + 0.3 * _rand(C, seed=52)).to(DEV)
    xd = c["x"].to(DEV)
    sc0, st0 = _stats_run(L, xd, shape, groups, gamma)
    xg = c["x"].double().reshape(B, groups, -1)
    mom = torch.stack([_partials(xg.sum(-1), ws_n, 53), _partials((xg * xg).sum(-1), ws_n, 54)], dim=-1)          # [B, G, ws_n, 2]
    ws = torch.full((B * groups * max(ws_n, L.AID_STATS_SPLIT) * 2,), NAN, device=DEV, dtype=torch.float64)
    ws[:mom.numel()] = mom.reshape(-1).to(DEV)
    sc1, st1 = _stats_run(L, xd, shape, groups, gamma, ws=ws, ws_n=ws_n)
    e = [rel_l2(sc1, sc0), rel_l2(st1[..., 0], st0[..., 0]), rel_l2(st1[..., 1], st0[..., 1])]
    dev = {k: c[k].to(DEV) for k in ("gd", "x", "gy")}
    out0, out1 = Par(shape, pad=FLAT), Par(shape, pad=FLAT)
    out0.v.fill_(NAN), out1.v.fill_(NAN)
    _nb_run(L, c, dev["gd"], dev["x"], dev["gy"], out0.v)
    wsd = torch.full((B * groups * ws_n + B * groups + 1,), NAN, device=DEV, dtype=torch.float64)
    wsd[-1] = SENT
    wsd[:B * groups * ws_n] = _partials(c["dot"], ws_n, 55).reshape(-1).to(DEV)
    _nb_run(L, c, dev["gd"], dev["x"], dev["gy"], out1.v, ws=wsd, ws_n=ws_n)
    assert float(wsd[-1]) == SENT
    e.append(rel_l2(out1.v.cpu(), out0.v.cpu()))
    r64, r32 = c["ref"](True)
    print(f"hand-made partials ws_n={ws_n}: scale {e[0]:.2e} mean {e[1]:.2e} inv {e[2]:.2e} norm_bwd out {e[3]:.2e} (against ws_n = 0)")
    assert bool(torch.isfinite(sc1).all()) and bool(torch.isfinite(out1.v).all()) and max(e) < 1e-6
    _check_abs(f"hand-made partials ws_n={ws_n}: norm_bwd against float64", out1.v.cpu(), r64, r32)


WINO_NB_SHAPES = [(1, 8, 2, 16),        # four lanes per row
                  (1, 8, 2, 48),        # 12 of 16 lanes live; the last group takes e5 / e9 = 0 from the o + 4 >= T branch
                  (1, 8, 2, 256),       # one wave per row
                  (1, 8, 2, 512),       # neighbour across a wave boundary
                  (1, 8, 2, 1040),      # neighbour across a block boundary, ragged second tile
                  (1, 8, 3, 48),        # 24 rows, 16 per block: ragged last block
                  (2, 8, 5, 16)]        # 80 rows, 64 per block


@pytest.mark.parametrize("shape", WINO_NB_SHAPES)
@pytest.mark.parametrize("wform", [1, 2])
def test_norm_bwd_wino(L, wform, shape):
    """out and its Winograd-domain copy (F(4,3) rows [6][T/4], F(8,3) rows [10][T/8], row stride 4 floats more) against the float64 transform of
    out * wscale[b, c]; wscale = NULL and with wscale_ld > C; contiguous operands and four differently padded parents"""
    B, C, Fd, T = shape
    m = 4 if wform == 1 else 8
    c = _nb_case(L, shape, 4, seed=61)
    wsc = 0.5 + torch.rand(B, C, generator=torch.Generator().manual_seed(62))
    wscw = torch.full((B, C + 3), BIG, device=DEV)
    wscw[:, 1:1 + C] = wsc.to(DEV)
    for with_scale, strided in ((False, False), (True, True)):
        r64, r32 = c["ref"](True)
        if strided:
            ins = [Par(shape, pad=pd, off=o, fill=BIG, data=c[k]) for k, (pd, o) in zip(("gd", "x", "gy"), PADS)]
            out = Par(shape, pad=PADS[3][0], off=PADS[3][1])
        else:
            ins = [Par(shape, pad=FLAT, data=c[k]) for k in ("gd", "x", "gy")]
            out = Par(shape, pad=FLAT)
        out.v.fill_(NAN)
        w = WRows(B, C, Fd, m + 2, T // m)
        _nb_run(L, c, ins[0].v, ins[1].v, ins[2].v, out.v, wout=w.v, wscale=wscw[:, 1:] if with_scale else None,
                wscale_ld=wscw.stride(0) if with_scale else 0, wform=wform)
        tag = f"norm_bwd wform={wform} {shape} wscale={int(with_scale)} strided={int(strided)}"
        assert out.untouched() and w.untouched(), tag
        _check_abs(tag + " out", out.v.cpu(), r64, r32)
        s = wsc[:, :, None, None] if with_scale else torch.ones(B, C, 1, 1)
        _check_abs(tag + " wout", w.planes(), _wino64(r64 * s.double(), m), _wino32(r32 * s, m), per_plane_dim=3)


def test_norm_bwd_refusals(L):
    c = _nb_case(L, (1, 8, 2, 16), 4, seed=71)
    c24 = _nb_case(L, (1, 8, 2, 24), 4, seed=72)
    for wform, n, m in ((1, 6, 4), (2, 10, 8)):
        for what in ("accumulate", "T=24", "sF"):
            cc = c24 if what == "T=24" else c
            B, C, Fd, T = cc["shape"]
            ins = [cc[k].to(DEV) for k in ("gd", "x", "gy")]
            out = Par(cc["shape"], pad=FLAT)
            w = torch.full((B, C, Fd, n * (T // m) + 4), SENT, device=DEV)
            wv = w[..., :n * (T // m) - 4] if what == "sF" else w          # (a view whose row stride is 4 floats short of [n][T/m])
            if what == "sF":
                wv = wv.as_strided(wv.shape, (w.stride(0), w.stride(1), n * (T // m) - 4, 1))
            with pytest.raises(L.AidError):
                _nb_run(L, cc, ins[0], ins[1], ins[2], out.v, accumulate=int(what == "accumulate"), wout=wv, wform=wform)
            assert bool((w == SENT).all()) and bool((out.buf == SENT).all()), (wform, what)


# ---------------------------------------------------------------------------------------------------------
# aid_scale_act
def _sa_inputs(shape, seed):
    """x with exact zeros and values that reach |x scale| = 6 (the GELU tails) on both sides; scale [B, C] in [0.5, 1.5]"""
    B, C, Fd, T = shape
    x = _rand(*shape, seed=seed, scale=1.5)
    scale = 0.5 + torch.rand(B, C, generator=torch.Generator().manual_seed(seed + 1))
    flat = x.reshape(-1)
    idx = torch.arange(flat.numel())
    tail = (6.0 / scale)[:, :, None, None].expand(shape).reshape(-1)
    flat[idx % 11 == 3] = tail[idx % 11 == 3] * torch.where(idx[idx % 11 == 3] % 2 == 0, 1.0, -1.0)
    flat[idx % 7 == 0] = 0.0
    x[:, :, ::2, 0] = 0.0                                           # every second row starts at an exact zero, the others end in one
    x[:, :, 1::2, -1] = 0.0
    assert float((x * scale[:, :, None, None]).abs().max()) > 5.9 and float(_gelu32(torch.tensor(0.0))) == 0.0
    return x, scale


def _sa_ref(x, scale, mul, act):
    """float64 and float32-CPU h = act(x scale[b, c] mul) (scale None -> 1, mul 0 -> 1)"""
    s64 = torch.ones(x.shape[:2], dtype=torch.float64) if scale is None else scale.double()
    s32 = torch.ones(x.shape[:2]) if scale is None else scale
    mu = mul if mul != 0.0 else 1.0
    h64, h32 = x.double() * (s64 * mu)[:, :, None, None], x * (s32 * mu)[:, :, None, None]
    return (_gelu64(h64), _gelu32(h32)) if act else (h64, h32)


def _sa_run(L, xv, yv, shape, scale, scale_ld, act, wino, mul):
    B, C, Fd, T = shape
    L.call("aid_scale_act", L.ScaleActParams(L.view4(xv), L.view4(yv), L.ptr(scale), scale_ld, B, C, Fd, T, act, wino, 1, mul))
    torch.cuda.synchronize()


def _scale_wide(scale):
    B, C = scale.shape
    w = torch.full((B, C + 3), BIG, device=DEV)
    w[:, 2:2 + C] = scale.to(DEV)
    return w


@pytest.mark.parametrize("shape", [(2, 8, 3, 4), (2, 16, 5, 12), (1, 8, 2, 48), (1, 8, 1, 1040)])
def test_scale_act_plain(L, shape):
    x, scale = _sa_inputs(shape, seed=81)
    sw = _scale_wide(scale)
    xs = Par(shape, pad=(2, 3, 8), off=1, fill=BIG, data=x)
    for act in (0, 1):
        for with_scale, mul in ((True, 0.0), (True, 0.5), (False, 0.5), (False, 0.0)):
            r64, r32 = _sa_ref(x, scale if with_scale else None, mul, act)
            y = Par(shape)
            y.v.fill_(NAN)
            _sa_run(L, xs.v, y.v, shape, sw[:, 2:] if with_scale else None, sw.stride(0) if with_scale else 0, act, 0, mul)
            assert y.untouched()
            _check_abs(f"scale_act {shape} act={act} scale={int(with_scale)} mul={mul}", y.v.cpu(), r64, r32)
            if act == 0 and not with_scale and mul == 0.0:
                assert torch.equal(y.v.cpu(), x)                     # a plain copy


WINO4_SA = [(1, 8, 1, 16), (1, 8, 3, 48), (1, 8, 1, 128),
            (1, 8, 1, 4112)]            # T / 16 = 257: lpr = 256, two tiles, the second with one live lane
WINO8_SA = [(1, 8, 1, 16), (1, 8, 3, 32), (1, 8, 3, 64),        # T = 32 / 64: the LDS-staged store; 24 rows < rpb
            (2, 8, 9, 32),              # 144 rows, 128 per block: ragged second block of the staged store
            (1, 8, 1, 128), (1, 8, 1, 4112)]


@pytest.mark.parametrize("wino,shape", [(1, s) for s in WINO4_SA] + [(2, s) for s in WINO8_SA])
def test_scale_act_wino(L, wino, shape):
    B, C, Fd, T = shape
    m = 4 if wino == 1 else 8
    x, scale = _sa_inputs(shape, seed=91)
    sw = _scale_wide(scale)
    xs = Par(shape, fill=BIG, data=x)
    for act, with_scale, mul in ((1, True, 0.0), (0, False, 0.5)):
        r64, r32 = _sa_ref(x, scale if with_scale else None, mul, act)
        w = WRows(B, C, Fd, m + 2, T // m)
        _sa_run(L, xs.v, w.v, shape, sw[:, 2:] if with_scale else None, sw.stride(0) if with_scale else 0, act, wino, mul)
        tag = f"scale_act wino={wino} {shape} act={act} scale={int(with_scale)}"
        assert w.untouched(), tag
        _check_abs(tag, w.planes(), _wino64(r64, m), _wino32(r32, m), per_plane_dim=3)


def test_scale_act_refusals(L):
    for wino, T, n, m in ((2, 48, 10, 8), (1, 24, 6, 4), (5, 16, 6, 4)):
        shape = (1, 8, 2, T)
        x = _rand(*shape, seed=95).to(DEV)
        y = torch.full((1, 8, 2, n * T), SENT, device=DEV)
        with pytest.raises(L.AidError):
            _sa_run(L, x, y, shape, None, 0, 0, wino, 0.0)
        torch.cuda.synchronize()
        assert bool((y == SENT).all())


# ---------------------------------------------------------------------------------------------------------
# aid_add2
@pytest.mark.parametrize("T", [4, 12, 1040])
def test_add2(L, T):
    shape = (2, 8, 3, T)
    u, v = _rand(*shape, seed=101), _rand(*shape, seed=102)
    a, b = f32(0.7), f32(-1.3)
    us, vs = Par(shape, fill=BIG, data=u), Par(shape, pad=(2, 3, 8), off=1, fill=BIG, data=v)
    for with_v in (True, False):
        y = Par(shape, pad=(1, 2, 12), off=1)
        y.v.fill_(NAN)
        L.call("aid_add2", L.Add2Params(L.view4(us.v), L.view4(vs.v if with_v else None), L.view4(y.v), *shape, a, b))
        torch.cuda.synchronize()
        assert y.untouched()
        r64 = a * u.double() + (b * v.double() if with_v else 0.0)
        r32 = a * u + b * v if with_v else a * u
        _check_abs(f"add2 T={T} v={int(with_v)}", y.v.cpu(), r64, r32)
        assert rel_l2(y.v.cpu(), r64) < 2e-6


# ---------------------------------------------------------------------------------------------------------
# views that are not float4-addressable are refused before any launch
def _misaligned(L, shape, kind):
    """(keep-alive buffer, aid_view): a flat buffer sliced at a one-float offset, or a parent whose channel stride is odd"""
    B, C, Fd, T = shape
    if kind == "offset":
        buf = torch.full((B * C * Fd * T + 4,), SENT, device=DEV)
        return buf, L.View(buf.data_ptr() + 4, C * Fd * T, Fd * T, T)
    buf = torch.full((B * C * (Fd * T + 1),), SENT, device=DEV)
    return buf, L.View(buf.data_ptr(), C * (Fd * T + 1), Fd * T + 1, T)


@pytest.mark.parametrize("kind", ["offset", "odd_sC"])
def test_misaligned_views_are_refused(L, kind):
    shape = (2, 8, 3, 16)
    B, C, Fd, T = shape
    good = [torch.full(shape, SENT, device=DEV) for _ in range(4)]
    gv = [L.view4(t) for t in good]
    none = L.view4(None)
    gamma = torch.ones(C, device=DEV)
    scale, stats = torch.full((B, C), SENT, device=DEV), torch.full((B, 4, 2), 1.0, device=DEV)
    ws = torch.full((B * 4 * L.AID_STATS_SPLIT * 2 + B * 4,), SENT, device=DEV, dtype=torch.float64)
    bad_buf, bad = _misaligned(L, shape, kind)

    def slots(k, n):
        v = list(gv[:n])
        v[k] = bad
        return v
    calls = [("aid_group_stats", L.GroupStatsParams(bad, B, C, Fd, T, 4, gamma.data_ptr(), None, 0, EPS, scale.data_ptr(), None, ws.data_ptr(), 0))]
    calls += [("aid_group_dot", L.GroupDotParams(*slots(k, 2), B, C, Fd, T, 4, ws.data_ptr())) for k in range(2)]
    calls += [("aid_norm_bwd", L.NormBwdParams(*slots(k, 4), B, C, Fd, T, 4, stats.data_ptr(), ws.data_ptr(), EPS, 0.5, 0, 0, none, None, 0, 0, 0, 1))
              for k in range(4)]
    calls += [("aid_scale_act", L.ScaleActParams(*slots(k, 2), None, 0, B, C, Fd, T, 0, 0, 1, 0.0)) for k in range(2)]
    wy = torch.full((B, C, Fd, 10 * T), SENT, device=DEV)
    calls += [("aid_scale_act", L.ScaleActParams(bad, L.view4(wy), None, 0, B, C, Fd, T, 0, wino, 1, 0.0)) for wino in (1, 2)]
    calls += [("aid_add2", L.Add2Params(*slots(k, 3), B, C, Fd, T, 1.0, 1.0)) for k in range(3)]
    for name, p in calls:
        with pytest.raises(L.AidError):
            L.call(name, p)
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in good + [bad_buf, scale, ws, wy])
