"""aid_time_attention_long / aid_time_attention_long_bwd (csrc/aid_attn_long.hip) alone, 1 <= T <= 1024: several key tiles per wave, key chunks of 128
that are full, half full or hold one key, ragged query tiles, the scalar branch of the 16-byte loads and stores (T % 4 != 0 or a pointer off the
16-byte grid), more than one column group in the backward's dV / dQ / dK kernel, the relative-position bias, probs = NULL, accumulate_gv = 0 | 1,
logits beyond expf's range, batch invariance, determinism and the refusals.

Inputs, references and bounds are those of tests/test_gpu_attention_edges.py (``_case``, ``_check``): float64 torch on the CPU; whole tensor within the
project's 1e-5 (forward) and 2e-5 (VJP) at sigma = 2; per query column, and everywhere at sigma = 6, at most 8 x the error of the same torch expression
evaluated in float32 on the CPU, with a floor of 1e-6.  Every case prints its kernel error, reference error and ratio."""
import pytest
import torch

from conftest import rel_l2
from test_gpu_attention_edges import (DEV, FACTOR, FLOOR, NAN, SENT, _banded, _bands_intact, _case, _check, _col_err, _shifted, big_logit_precheck)

pytestmark = pytest.mark.gpu
FWD, BWD = "aid_time_attention_long", "aid_time_attention_long_bwd"

# (B, H, F, T) -- what each shape is for
SHAPES = [
    (1, 2, 16, 129),      # the second key tile of wave 0 holds ONE key (second chunk: one key), the fifth query tile one query; scalar branch
    (2, 2, 33, 160),      # T % 4 == 0 (float4 branch), a quarter-filled second chunk; F = 33: second 32-row O tile with a single row
    (1, 2, 40, 256),      # the shipped T: every tile full, two key chunks, two column groups in the backward
    (1, 1, 16, 257),      # a third chunk (NT = 4 instance) with one key
    (1, 2, 9, 383),       # T odd, the last tile short by one; F < 16: the first trip of the score loop already has rows >= F
    (1, 2, 17, 516),      # T % 4 == 0 with four keys in the last tile (NT = 8 instance, fifth chunk); five column groups in the backward
    (1, 1, 8, 512),       # NT = 4, every tile full
    (1, 1, 8, 1024),      # the largest instance, every tile of every wave full
    (1, 1, 320, 255),     # the shipped F with a ragged T: scalar branch on every row
    (2, 3, 17, 100),      # T <= 128 through the long entries (NT = 1), ragged fourth tile
    (1, 2, 40, 128),      # T = 128 through the long entries, every tile full
]
BIG_LOGIT_SHAPES = [(1, 2, 16, 129), (1, 2, 40, 256), (1, 2, 17, 516), (1, 1, 8, 512)]
MISALIGNED_SHAPES = [(2, 2, 33, 160), (1, 2, 17, 516)]      # T % 4 == 0: only the pointer decides between the float4 and the scalar branch
_ids = dict(ids=lambda s: "x".join(map(str, s)))


@pytest.fixture(scope="module")
def L():
    from audio_inpainting_diffusion_amd import _lib
    _lib.lib()
    return _lib


def _forward(L, c, with_probs=True, off=()):
    """one forward call on NaN-filled, sentinel-banded outputs; ``off`` names the pointers moved one float off the 16-byte grid"""
    B, H, Fd, T = c["shape"]
    qk, v, bias = c["qk"].to(DEV), _shifted(c["v"], int("v" in off)), _shifted(c["bias"], int("bias" in off))
    obuf, out = _banded(B * H * Fd * T, NAN)
    pbuf, probs = _banded(B * H * T * T, NAN, int("probs" in off))
    L.call(FWD, L.AttentionParams(qk.data_ptr(), v.data_ptr(), out.data_ptr(), probs.data_ptr() if with_probs else None, B, H, Fd, T,
                                  float(Fd) ** -0.5, L.ptr(bias)))
    torch.cuda.synchronize()
    assert _bands_intact(obuf, out.numel()) and _bands_intact(pbuf, probs.numel(), int("probs" in off)), f"{FWD} wrote outside out / probs"
    if not with_probs:
        assert bool(torch.isnan(probs).all())
    return out.reshape(B, H, Fd, T), probs.reshape(B, H, T, T)


def _backward(L, c, probs, accumulate, off=()):
    """one backward call: gqk and ws NaN-filled, gv 0.5 (accumulate) or NaN, all between sentinel bands"""
    B, H, Fd, T = c["shape"]
    qk, v, go = _shifted(c["qk"], int("qk" in off)), c["v"].to(DEV), _shifted(c["go"], int("gout" in off))
    pr = _shifted(probs, int("probs" in off))
    qbuf, gqk = _banded(B * H * 2 * Fd * T, NAN)
    vbuf, gv = _banded(B * H * Fd * T, 0.5 if accumulate else NAN)
    wbuf, ws = _banded(B * H * T * T, NAN, int("ws" in off))
    L.call(BWD, L.AttentionBwdParams(qk.data_ptr(), v.data_ptr(), pr.data_ptr(), go.data_ptr(), gqk.data_ptr(), gv.data_ptr(),
                                     B, H, Fd, T, float(Fd) ** -0.5, int(accumulate), ws.data_ptr()))
    torch.cuda.synchronize()
    assert _bands_intact(qbuf, gqk.numel()) and _bands_intact(vbuf, gv.numel()) and _bands_intact(wbuf, ws.numel(), int("ws" in off)), \
        f"{BWD} wrote outside gqk / gv / ws"
    return gqk.reshape(B, H * 2 * Fd, T), gv.reshape(B, H, Fd, T), ws.reshape(B, H, T, T)


def _check_forward(L, c, tag, whole_tol):
    out, probs = _forward(L, c)
    out2, probs2 = _forward(L, c)                                      # a second call: the same bits
    assert torch.equal(out, out2) and torch.equal(probs, probs2), f"{tag}: a second call differs"
    out_np, _ = _forward(L, c, with_probs=False)                       # probs = NULL: the same out, bit for bit
    assert torch.equal(out, out_np), f"{tag}: out differs between probs given and probs = NULL"
    _check(tag, "probs", probs, c, whole_tol)
    _check(tag, "out", out, c, whole_tol)
    rows = probs.double().sum(-1)
    print(f"attn-long {tag} probs row sums: max |sum - 1| = {float((rows - 1).abs().max()):.2e}")
    assert float((rows - 1).abs().max()) <= 1e-6
    return probs


def _check_backward(L, c, tag, whole_tol, columns=True):
    _, probs = _forward(L, c)
    probs = probs.contiguous()
    gqk, gv, ws = _backward(L, c, probs, accumulate=0)
    for a, b in zip(_backward(L, c, probs, accumulate=0), (gqk, gv, ws)):
        assert torch.equal(a, b), f"{tag}: a second call differs"
    gqk1, gv1, ws1 = _backward(L, c, probs, accumulate=1)
    # accumulate_gv = 1 adds the same product onto what is there: one float32 addition more, everything else the same bits
    assert torch.equal(gv1, gv + 0.5) and torch.equal(gqk1, gqk) and torch.equal(ws1, ws), f"{tag}: accumulate_gv = 1 is not 0.5 + the accumulate_gv = 0 result"
    assert rel_l2(gv1.cpu().double() - 0.5, c["r64"]["gv"]) < 2e-5
    for name, got in (("gqk", gqk), ("gv", gv), ("dS", ws)):            # ws = dS = the gradient w.r.t. (q k^T + bias) of every sample
        if columns:
            _check(tag, name, got, c, whole_tol)
        else:            # (sigma = 6: where P is one-hot to float32, dS of that row is pure cancellation in the float32 CPU evaluation as well -- printed)
            H = c["shape"][1]
            e, e32 = rel_l2(got.cpu(), c["r64"][name]), rel_l2(c["r32"][name], c["r64"][name])
            col, col32 = float(_col_err(name, got, c["r64"][name], H).max()), float(_col_err(name, c["r32"][name], c["r64"][name], H).max())
            tol = max(FACTOR * e32, FLOOR)
            print(f"attn-long {tag} {name}: whole kernel {e:.2e} fp32-cpu {e32:.2e} ratio {e / max(e32, 1e-300):.2f} (bound {tol:.1e}) | "
                  f"worst column kernel {col:.2e} fp32-cpu {col32:.2e} (printed only)")
            assert bool(torch.isfinite(got).all()) and e < tol, f"{tag} {name}: whole-tensor rel-L2 {e:.3e} >= {tol:.3e}"
    # the gradient w.r.t. the shared bias table is dS summed over the samples
    gb, gb_ref = ws.double().sum(0).cpu(), c["r64"]["dS"].sum(0)
    gb_tol = 2e-5 if whole_tol is not None else max(FACTOR * rel_l2(c["r32"]["dS"].double().sum(0), gb_ref), FLOOR)
    assert rel_l2(gb, gb_ref) < gb_tol


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_forward(L, shape, with_bias):
    _check_forward(L, _case(shape, with_bias), f"fwd {shape} bias={int(with_bias)}", 1e-5)


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_backward(L, shape, with_bias):
    _check_backward(L, _case(shape, with_bias), f"bwd {shape} bias={int(with_bias)}", 2e-5)


@pytest.mark.parametrize("shape", BIG_LOGIT_SHAPES, **_ids)
def test_large_logits(L, shape):
    """qk at sigma = 6: |logit| beyond 100, rows dominated by one key; a softmax without the max over ALL of a lane's tiles overflows here"""
    c = _case(shape, True, 6.0)
    big_logit_precheck(c)
    _check_forward(L, c, f"fwd-sigma6 {shape}", None)
    _check_backward(L, c, f"bwd-sigma6 {shape}", None, columns=False)


@pytest.mark.parametrize("which", ["v", "probs", "bias"])
@pytest.mark.parametrize("shape", MISALIGNED_SHAPES, **_ids)
def test_forward_misaligned_pointer(L, shape, which):
    """one pointer one float off the 16-byte grid: the scalar branch loads and stores the same values, the MFMA order is unchanged"""
    c = _case(shape, True)
    out, probs = _forward(L, c)
    out_m, probs_m = _forward(L, c, off=(which,))
    assert torch.equal(out_m, out) and torch.equal(probs_m, probs)


@pytest.mark.parametrize("which", ["qk", "gout", "probs", "ws"])
@pytest.mark.parametrize("shape", MISALIGNED_SHAPES, **_ids)
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
    c3 = _case((3, 2, 33, 257), True)
    c1 = {"shape": (1, 2, 33, 257), "qk": c3["qk"][:1], "v": c3["v"][:1], "go": c3["go"][:1], "bias": c3["bias"]}
    out3, probs3 = _forward(L, c3)
    out1, probs1 = _forward(L, c1)
    assert torch.equal(out3[:1], out1) and torch.equal(probs3[:1], probs1)
    for acc in (0, 1):
        g3 = _backward(L, c3, probs3.contiguous(), acc)
        g1 = _backward(L, c1, probs1.contiguous(), acc)
        for a, b in zip(g3, g1):
            assert torch.equal(a[:1], b)


@pytest.mark.parametrize("T", [0, 1025])
def test_refusals(L, T):
    """T outside [1, 1024] is refused by both entry points before anything is launched: the outputs keep their sentinel"""
    B, H, Fd, n = 1, 2, 8, 1025
    assert L.AID_ATTN_LONG_MAX_T == 1024
    qk, v, go = torch.zeros(B * H * 2 * Fd * n, device=DEV), torch.zeros(B * H * Fd * n, device=DEV), torch.zeros(B * H * Fd * n, device=DEV)
    probs = torch.full((B * H * n * n,), SENT, device=DEV)
    out, gqk, gv, ws = (torch.full((m,), SENT, device=DEV) for m in (B * H * Fd * n, B * H * 2 * Fd * n, B * H * Fd * n, B * H * n * n))
    with pytest.raises(L.AidError):
        L.call(FWD, L.AttentionParams(qk.data_ptr(), v.data_ptr(), out.data_ptr(), probs.data_ptr(), B, H, Fd, T, float(Fd) ** -0.5, None))
    with pytest.raises(L.AidError):
        L.call(BWD, L.AttentionBwdParams(qk.data_ptr(), v.data_ptr(), probs.data_ptr(), go.data_ptr(), gqk.data_ptr(), gv.data_ptr(),
                                         B, H, Fd, T, float(Fd) ** -0.5, 0, ws.data_ptr()))
    torch.cuda.synchronize()
    for t in (out, probs, gqk, gv, ws):
        assert bool((t == SENT).all())
