"""aid_time_attention / aid_time_attention_bwd (csrc/aid_attn.hip) at their edges: ragged key and query tiles, the scalar branch of att_ld4 / att_st4
(T % 4 != 0 or a pointer off the 16-byte grid), the three attn_bwd_fr_kernel<NCOL> instances from both sides of T = 32 | 33 and 63 | 65, the
relative-position bias, probs = NULL, accumulate_gv = 0 | 1, logits beyond expf's range, batch invariance and the refusals.

References are plain torch on the CPU in float64 (einsum / softmax / autograd, bias added before the scale as oracle/unet.py:88-90 does).

Bounds.  Whole tensor: the project's 1e-5 (forward) and 2e-5 (VJP).  Per query column -- probs per (b, h, n) row, out / gv per (b, h, t) over f, gqk per
(b, h, q | k, t) over f, dS per (b, h, n) row (against the magnitude of the row's evaluation, see _col_err) -- and in the sigma = 6 cases the bound is
made in the test from the reference side alone: the same torch expression evaluated in float32 on the CPU, its error against float64 on the same
inputs and the same partition (for the columns: its worst column); the kernel's (worst column's) error may be at most 8 x that, with an absolute floor
of 1e-6.  Kernel and float32 torch both accumulate in float32; the MFMA chain sums over f in k-steps of 2 where torch's sums are blocked, an ordering
factor of a few units, while a structurally wrong column is off by O(1) on that column.  Every case prints its kernel error, reference error and ratio (profiles/r22_attention_train_edges.txt)."""
import functools

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64              # floats of sentinel band on each side of an output (256 bytes: the interior stays 16-byte aligned)
SENT = 123.0
NAN = float("nan")
FACTOR, FLOOR = 8.0, 1e-6

# (B, H, F, T) -- what each shape is for
SHAPES = [
    (1, 2, 9, 1),         # T = 1: one key, one query (softmax of a single logit; dS = 0); F < 16: first trip of the score loop already has fr >= F
    (2, 3, 17, 5),        # T < 8: one partly filled 4-column group per half-wave; F = 17: second 16-row trip of the score loop with fr < F on one row only
    (2, 2, 33, 31),       # T = 31: fr<1> from below its boundary, last key / query of the tile missing; F = 33: second 32-row O tile with a single row
    (1, 3, 129, 32),      # T = 32: fr<1> at its boundary, float4 branch everywhere; F = 129: 5 row tiles over the forward's 4 waves, RT * 32 = 128 -> 2 row blocks
    (1, 3, 16, 33),       # T = 33: fr<2> from the ragged side; wave 1 holds ONE key (m0 < T, 31 of 32 masked), second query tile holds one query; F = 16: exactly one trip
    (1, 2, 40, 48),       # T = 48: T % 4 == 0 (float4 branch) with a half-filled second tile; F = 40 on fr<2>: RT * 32 = 64, second row tile ragged
    (2, 2, 129, 63),      # T = 63: fr<2> from below its boundary; F = 129: 3 row blocks of 64, the last with an idle wave pair (f0 >= F)
    (1, 3, 1, 65),        # T = 65: fr<4> from the ragged side, wave 2 holds one key, third query tile one query; F = 1
    (1, 2, 33, 97),       # T = 97: wave 3 holds one key, fourth query tile one query; fr<4>: RT = 1, F = 33 -> 2 row blocks
    (2, 3, 17, 100),      # T = 100: T % 4 == 0 with a ragged fourth tile (4 of 32 keys): float4 loads next to the T edge
    (1, 2, 40, 128),      # T = 128: every tile full
    (1, 2, 320, 127),     # the shipped regime (F = 320) with a ragged T: scalar branch on every row
]
BIG_LOGIT_SHAPES = [(1, 3, 16, 33), (1, 2, 33, 97), (1, 2, 40, 128)]
MISALIGNED_SHAPES = [(1, 3, 129, 32), (2, 3, 17, 100)]      # T % 4 == 0: only the pointer decides between the float4 and the scalar branch


@pytest.fixture(scope="module")
def L():
    from audio_inpainting_diffusion_amd import _lib
    _lib.lib()
    return _lib


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _reference(qk, v, go, bias, dtype):
    """probs, out and the gradients of <out, go> w.r.t. qk, v and a per-sample copy of the bias (= dS of every sample), all computed in ``dtype``"""
    B, H, Fd, T = v.shape
    qk_, v_ = qk.to(dtype).requires_grad_(), v.to(dtype).requires_grad_()
    bb = (torch.zeros(H, T, T) if bias is None else bias).to(dtype)[None].repeat(B, 1, 1, 1).requires_grad_()
    q4 = qk_.reshape(B, H, 2 * Fd, T).permute(0, 1, 3, 2)
    sim = (torch.einsum("bhnd,bhmd->bhnm", q4[..., :Fd], q4[..., Fd:]) + bb) * (float(Fd) ** -0.5)
    probs = sim.softmax(-1)
    out = torch.einsum("bhnm,bhmd->bhnd", probs, v_.permute(0, 1, 3, 2)).permute(0, 1, 3, 2)
    gqk, gv, gb = torch.autograd.grad((out * go.to(dtype)).sum(), (qk_, v_, bb))
    # dS[n, :] = scale * P[n, :] o (dP[n, :] - d_n), d_n = <P[n, :], dP[n, :]>: the magnitude of what a row's evaluation adds up, see _col_err
    P, dP = probs.detach(), torch.einsum("bhfn,bhfm->bhnm", go.to(dtype), v.to(dtype))
    mag = (float(Fd) ** -0.5) * (P * (dP.abs() + (P * dP).sum(-1, keepdim=True).abs())).norm(dim=-1)
    return {"probs": P, "out": out.detach().contiguous(), "gqk": gqk, "gv": gv, "dS": gb, "sim": sim.detach(), "dS_mag": mag}


@functools.lru_cache(maxsize=None)
def _case(shape, with_bias, sigma=2.0):
    """inputs, the float64 reference and the float32 CPU evaluation of one case (computed once, shared, never modified)"""
    B, H, Fd, T = shape
    s0 = 100 * T + Fd
    qk = _rand(B, H * 2 * Fd, T, seed=s0 + 1, scale=sigma)
    v, go = _rand(B, H, Fd, T, seed=s0 + 2), _rand(B, H, Fd, T, seed=s0 + 3)
    bias = _rand(H, T, T, seed=s0 + 4, scale=2.0) if with_bias else None
    return {"shape": shape, "qk": qk, "v": v, "go": go, "bias": bias, "r64": _reference(qk, v, go, bias, torch.float64),
            "r32": _reference(qk, v, go, bias, torch.float32)}


def big_logit_precheck(c):
    """CPU only: the sigma = 6 inputs really leave expf's range (fp32 expf overflows at 88.7) and the rows are dominated by one key"""
    sim, top = c["r64"]["sim"], c["r64"]["probs"].max(-1).values
    assert float(sim.abs().max()) > 100.0, float(sim.abs().max())
    assert float(top.median()) >= 0.9 and float((top >= 0.4).double().mean()) >= 0.95, (float(top.median()), float(top.min()))


_DIMS = {"probs": -1, "out": 2, "gv": 2, "dS": -1, "gqk": 3}


def _col_err(name, got, ref, H, mag=None):
    """rel-L2 of every column.  dS rows are measured against ``mag``, the magnitude of the row's evaluation, not against the row's own norm: where one
    key takes p -> 1, dP - d cancels and the row's norm falls to (1 - p) of the terms that form it, so that the error relative to the row's norm is
    u / (1 - p) for the float32 CPU evaluation and the kernel alike, one realisation of a rounding each (measured: 1e-4 .. 8e-4 on single rows against a
    median of 5e-7, on either side, at rows with p = 0.99 .. 0.9996 and never at an edge row).  Against ``mag`` both stay at a few u on every row, and
    the worst rows can be compared; a row that is structurally wrong is off by O(row norm) >= (1 - p) mag."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    if mag is not None:
        return (got - ref).norm(dim=-1) / mag.clamp_min(1e-300)
    if name == "gqk":                                     # [B, H*2F, T] -> [B, H, q | k, F, T]
        B, R, T = ref.shape
        got, ref = got.reshape(B, H, 2, R // (2 * H), T), ref.reshape(B, H, 2, R // (2 * H), T)
    d = _DIMS[name]
    return (got - ref).norm(dim=d) / ref.norm(dim=d).clamp_min(1e-300)


def _check(tag, name, got, c, whole_tol):
    """whole tensor against ``whole_tol`` (None: 8 x the float32 CPU evaluation's own error) and the worst column against 8 x the float32 evaluation's worst"""
    H = c["shape"][1]
    r64, r32 = c["r64"][name], c["r32"][name]
    assert bool(torch.isfinite(got).all()), f"{tag} {name}: not finite (an element was not written, or overflowed)"
    e, e32 = rel_l2(got.cpu(), r64), rel_l2(r32, r64)
    mag = c["r64"]["dS_mag"] if name == "dS" else None
    col, col32 = float(_col_err(name, got, r64, H, mag).max()), float(_col_err(name, r32, r64, H, mag).max())
    tol = max(FACTOR * e32, FLOOR) if whole_tol is None else whole_tol
    ctol = max(FACTOR * col32, FLOOR)
    print(f"attn-edges {tag} {name}: whole kernel {e:.2e} fp32-cpu {e32:.2e} ratio {e / max(e32, 1e-300):.2f} (bound {tol:.1e}) | "
          f"worst column kernel {col:.2e} fp32-cpu {col32:.2e} ratio {col / max(col32, 1e-300):.2f} (bound {ctol:.1e})")
    assert e < tol, f"{tag} {name}: whole-tensor rel-L2 {e:.3e} >= {tol:.3e}"
    assert col <= ctol, f"{tag} {name}: worst column {col:.3e} > {ctol:.3e} (fp32 CPU evaluation: {col32:.3e})"


def _banded(n, fill, off=0):
    """n floats filled with ``fill`` between two sentinel bands; off = 1 puts the interior one float off the 16-byte grid"""
    buf = torch.full((2 * PAD + n + off,), SENT, device=DEV)
    view = buf[PAD + off:PAD + off + n]
    view.fill_(fill)
    assert view.data_ptr() % 16 == 4 * off
    return buf, view


def _bands_intact(buf, n, off=0):
    return bool((buf[:PAD + off] == SENT).all()) and bool((buf[PAD + off + n:] == SENT).all())


def _shifted(t, off):
    """a device copy of ``t`` whose first element sits ``off`` floats past a 16-byte boundary"""
    if t is None:
        return None
    buf = torch.empty(t.numel() + 4, device=DEV)
    view = buf[off:off + t.numel()]
    view.copy_(t.reshape(-1))
    assert view.data_ptr() % 16 == 4 * off
    return view


def _forward(L, c, with_probs=True, off=()):
    """one aid_time_attention call on NaN-filled, sentinel-banded outputs; ``off`` names the pointers moved one float off the 16-byte grid"""
    B, H, Fd, T = c["shape"]
    qk, v, bias = c["qk"].to(DEV), _shifted(c["v"], int("v" in off)), _shifted(c["bias"], int("bias" in off))
    obuf, out = _banded(B * H * Fd * T, NAN)
    pbuf, probs = _banded(B * H * T * T, NAN, int("probs" in off))
    L.call("aid_time_attention", L.AttentionParams(qk.data_ptr(), v.data_ptr(), out.data_ptr(), probs.data_ptr() if with_probs else None, B, H, Fd, T,
                                                   float(Fd) ** -0.5, L.ptr(bias)))
    torch.cuda.synchronize()
    assert _bands_intact(obuf, out.numel()) and _bands_intact(pbuf, probs.numel(), int("probs" in off)), "aid_time_attention wrote outside out / probs"
    if not with_probs:
        assert bool(torch.isnan(probs).all())
    return out.reshape(B, H, Fd, T), probs.reshape(B, H, T, T)


def _backward(L, c, probs, accumulate, off=()):
    """one aid_time_attention_bwd call: gqk and ws NaN-filled, gv 0.5 (accumulate) or NaN, all between sentinel bands"""
    B, H, Fd, T = c["shape"]
    qk, v, go = _shifted(c["qk"], int("qk" in off)), c["v"].to(DEV), _shifted(c["go"], int("gout" in off))
    pr = _shifted(probs, int("probs" in off))
    qbuf, gqk = _banded(B * H * 2 * Fd * T, NAN)
    vbuf, gv = _banded(B * H * Fd * T, 0.5 if accumulate else NAN)
    wbuf, ws = _banded(B * H * T * T, NAN, int("ws" in off))
    L.call("aid_time_attention_bwd", L.AttentionBwdParams(qk.data_ptr(), v.data_ptr(), pr.data_ptr(), go.data_ptr(), gqk.data_ptr(), gv.data_ptr(),
                                                          B, H, Fd, T, float(Fd) ** -0.5, int(accumulate), ws.data_ptr()))
    torch.cuda.synchronize()
    assert _bands_intact(qbuf, gqk.numel()) and _bands_intact(vbuf, gv.numel()) and _bands_intact(wbuf, ws.numel(), int("ws" in off)), \
        "aid_time_attention_bwd wrote outside gqk / gv / ws"
    return gqk.reshape(B, H * 2 * Fd, T), gv.reshape(B, H, Fd, T), ws.reshape(B, H, T, T)


def _check_forward(L, c, tag, whole_tol):
    out, probs = _forward(L, c)
    out_np, _ = _forward(L, c, with_probs=False)                       # probs = NULL: the same out, bit for bit
    assert torch.equal(out, out_np), f"{tag}: out differs between probs given and probs = NULL"
    _check(tag, "probs", probs, c, whole_tol)
    _check(tag, "out", out, c, whole_tol)
    rows = probs.double().sum(-1)
    print(f"attn-edges {tag} probs row sums: max |sum - 1| = {float((rows - 1).abs().max()):.2e}")
    assert float((rows - 1).abs().max()) <= 1e-6
    return probs


def _check_backward(L, c, tag, whole_tol, columns=True):
    _, probs = _forward(L, c)
    probs = probs.contiguous()
    gqk, gv, ws = _backward(L, c, probs, accumulate=0)
    gqk1, gv1, ws1 = _backward(L, c, probs, accumulate=1)
    # accumulate_gv = 1 adds the same product onto what is there: one float32 addition more, everything else the same bits
    assert torch.equal(gv1, gv + 0.5) and torch.equal(gqk1, gqk) and torch.equal(ws1, ws), f"{tag}: accumulate_gv = 1 is not 0.5 + the accumulate_gv = 0 result"
    assert rel_l2(gv1.cpu().double() - 0.5, c["r64"]["gv"]) < 2e-5
    for name, got in (("gqk", gqk), ("gv", gv), ("dS", ws)):            # ws = dS = the gradient w.r.t. (q k^T + bias) of every sample
        if columns:
            _check(tag, name, got, c, whole_tol)
        else:
            H = c["shape"][1]
            e, e32 = rel_l2(got.cpu(), c["r64"][name]), rel_l2(c["r32"][name], c["r64"][name])
            col, col32 = float(_col_err(name, got, c["r64"][name], H).max()), float(_col_err(name, c["r32"][name], c["r64"][name], H).max())
            tol = max(FACTOR * e32, FLOOR)
            print(f"attn-edges {tag} {name}: whole kernel {e:.2e} fp32-cpu {e32:.2e} ratio {e / max(e32, 1e-300):.2f} (bound {tol:.1e}) | "
                  f"worst column kernel {col:.2e} fp32-cpu {col32:.2e} (printed only)")
            assert bool(torch.isfinite(got).all()) and e < tol, f"{tag} {name}: whole-tensor rel-L2 {e:.3e} >= {tol:.3e}"
    # the gradient w.r.t. the shared bias table is dS summed over the samples
    gb, gb_ref = ws.double().sum(0).cpu(), c["r64"]["dS"].sum(0)
    gb_tol = 2e-5 if whole_tol is not None else max(FACTOR * rel_l2(c["r32"]["dS"].double().sum(0), gb_ref), FLOOR)
    assert rel_l2(gb, gb_ref) < gb_tol


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_edges(L, shape, with_bias):
    c = _case(shape, with_bias)
    _check_forward(L, c, f"fwd {shape} bias={int(with_bias)}", 1e-5)


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_edges(L, shape, with_bias):
    c = _case(shape, with_bias)
    _check_backward(L, c, f"bwd {shape} bias={int(with_bias)}", 2e-5)


@pytest.mark.parametrize("shape", BIG_LOGIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_large_logits(L, shape):
    """qk at sigma = 6: |logit| beyond 100, rows dominated by one key.  A softmax without the max subtraction overflows here (fp32 expf: 88.7).
    The backward runs too (P close to one-hot); its columns are printed, not asserted: where P is one-hot to float32, dS of that row is pure cancellation
    in the reference's float32 evaluation as well."""
    c = _case(shape, True, 6.0)
    big_logit_precheck(c)
    _check_forward(L, c, f"fwd-sigma6 {shape}", None)
    _check_backward(L, c, f"bwd-sigma6 {shape}", None, columns=False)


@pytest.mark.parametrize("which", ["v", "probs", "bias"])
@pytest.mark.parametrize("shape", MISALIGNED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_misaligned_pointer(L, shape, which):
    """one pointer one float off the 16-byte grid: att_ld4 / att_st4 take their scalar branch, load and store the same values, the MFMA order is unchanged"""
    c = _case(shape, True)
    out, probs = _forward(L, c)
    out_m, probs_m = _forward(L, c, off=(which,))
    assert torch.equal(out_m, out) and torch.equal(probs_m, probs)


@pytest.mark.parametrize("which", ["qk", "gout", "probs", "ws"])
@pytest.mark.parametrize("shape", MISALIGNED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_misaligned_pointer(L, shape, which):
    c = _case(shape, True)
    _, probs = _forward(L, c)
    probs = probs.contiguous()
    for acc in (0, 1):
        ref = _backward(L, c, probs, acc)
        got = _backward(L, c, probs, acc, off=(which,))
        for a, b in zip(got, ref):
            assert torch.equal(a, b)


def test_batch_invariance(L):
    """sample 0 of a B = 3 call is the B = 1 call on that sample, bit for bit"""
    c3 = _case((3, 2, 33, 97), True)
    c1 = {"shape": (1, 2, 33, 97), "qk": c3["qk"][:1], "v": c3["v"][:1], "go": c3["go"][:1], "bias": c3["bias"]}
    out3, probs3 = _forward(L, c3)
    out1, probs1 = _forward(L, c1)
    assert torch.equal(out3[:1], out1) and torch.equal(probs3[:1], probs1)
    for acc in (0, 1):
        g3 = _backward(L, c3, probs3.contiguous(), acc)
        g1 = _backward(L, c1, probs1.contiguous(), acc)
        for a, b in zip(g3, g1):
            assert torch.equal(a[:1], b)


@pytest.mark.parametrize("T", [0, 129])
def test_refusals(L, T):
    """T outside [1, 128] is refused by both entry points before anything is launched: the outputs keep their sentinel"""
    B, H, Fd, n = 1, 2, 8, 129
    qk, v, go = torch.zeros(B * H * 2 * Fd * n, device=DEV), torch.zeros(B * H * Fd * n, device=DEV), torch.zeros(B * H * Fd * n, device=DEV)
    probs = torch.full((B * H * n * n,), SENT, device=DEV)
    out, gqk, gv, ws = (torch.full((m,), SENT, device=DEV) for m in (B * H * Fd * n, B * H * 2 * Fd * n, B * H * Fd * n, B * H * n * n))
    with pytest.raises(L.AidError):
        L.call("aid_time_attention", L.AttentionParams(qk.data_ptr(), v.data_ptr(), out.data_ptr(), probs.data_ptr(), B, H, Fd, T, float(Fd) ** -0.5, None))
    with pytest.raises(L.AidError):
        L.call("aid_time_attention_bwd", L.AttentionBwdParams(qk.data_ptr(), v.data_ptr(), probs.data_ptr(), go.data_ptr(), gqk.data_ptr(), gv.data_ptr(),
                                                              B, H, Fd, T, float(Fd) ** -0.5, 0, ws.data_ptr()))
    torch.cuda.synchronize()
    for t in (out, probs, gqk, gv, ws):
        assert bool((t == SENT).all())
