"""The small training-only backward kernels of csrc/aid_train.hip, each directly against a float64 reference: aid_relpos_bwd, aid_scale_bwd,
aid_modulation_bwd and aid_embed_bwd at sizes where every 256-stride loop takes a second, ragged trip, grids have more than one workgroup, far
relative-position buckets are populated (and some are empty), with accumulate = 0 on a NaN pre-fill and accumulate = 1 on a 0.25 pre-fill, the
scale == 0 guard, and leading dimensions wider than the row.  Every case prints its errors (profiles/r22_attention_train_edges.txt)."""
import functools
import math

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
SENT = 123.0


@pytest.fixture(scope="module")
def L():
    from audio_inpainting_diffusion_amd import _lib
    _lib.lib()
    return _lib


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _filled(shape, value):
    return torch.full(shape, value, device=DEV)


# ---------------------------------------------------------------------------------------------------------
# aid_relpos_bwd
NUM_BUCKETS, MAX_DISTANCE, HEADS = 32, 64, 3


def _buckets(T, table):
    """``net``: the network's own T5-style table (_RelPos.buckets: at T = 5 only 9 of the 32 buckets occur, at T = 128 the logarithmic far ones too);
    ``one``: a synthetic table in which bucket 7 holds every position and every other bucket is empty"""
    if table == "one":
        return torch.full((T, T), 7, dtype=torch.long)
    from audio_inpainting_diffusion_amd.network import _RelPos
    return _RelPos(NUM_BUCKETS, MAX_DISTANCE, HEADS).buckets(T)


def _relpos_run(L, dS, bucket, accumulate):
    B, H, T, _ = dS.shape
    dW = _filled((NUM_BUCKETS + 2, H), SENT)                       # rows 0 and NUM_BUCKETS + 1 are sentinels
    dW[1:-1] = 0.25 if accumulate else NAN
    L.call("aid_relpos_bwd", L.RelposBwdParams(dS.data_ptr(), bucket.data_ptr(), dW[1:].data_ptr(), B, H, T, NUM_BUCKETS, int(accumulate)))
    torch.cuda.synchronize()
    assert bool((dW[0] == SENT).all()) and bool((dW[-1] == SENT).all())
    return dW[1:-1].clone()


@pytest.mark.parametrize("table", ["net", "one"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [5, 33, 128])          # T^2 = 25 < 256; 1089 = 4 * 256 + 65 (ragged fifth trip of the i += 256 loop); 16384 >> 256
def test_relpos_bwd(L, T, B, table):
    H = HEADS
    dS = _rand(B, H, T, T, seed=700 + T + B)
    bucket = _buckets(T, table)
    idx = bucket.reshape(-1)
    flat = dS.double().sum(0).reshape(H, T * T)
    ref = torch.zeros(NUM_BUCKETS, H, dtype=torch.float64).index_add_(0, idx, flat.t().contiguous())
    mass = torch.zeros(NUM_BUCKETS, H, dtype=torch.float64).index_add_(0, idx, dS.double().abs().sum(0).reshape(H, T * T).t().contiguous())
    empty = torch.bincount(idx, minlength=NUM_BUCKETS) == 0
    assert bool(empty.any()) and (table == "net" or int((~empty).sum()) == 1)
    dSd, bd = dS.to(DEV), bucket.to(torch.int32).to(DEV)
    got = _relpos_run(L, dSd, bd, 0)
    acc = _relpos_run(L, dSd, bd, 1)
    # the device sums in float64 and rounds once: 2^-24 of the value; 1e-6 of the bucket's absolute mass is the issue's bound
    err = (got.cpu().double() - ref).abs()
    print(f"relpos_bwd T={T} B={B} {table}: {int((~empty).sum())} buckets filled, max |err| / mass = {float((err[~empty] / mass[~empty]).max()):.2e}")
    assert bool(torch.isfinite(got).all()) and bool((err <= 1e-6 * mass).all())
    assert bool((got[empty.to(DEV)] == 0).all()) and bool((acc[empty.to(DEV)] == 0.25).all())          # empty buckets: exactly 0 / exactly what was there
    assert torch.equal(acc, got + 0.25)                                                                 # accumulate: one float32 addition onto the old value


def test_relpos_bwd_chained_after_attention(L):
    """attention forward with bias = W[bucket] -> aid_time_attention_bwd -> aid_relpos_bwd against float64 autograd w.r.t. W, at T = 97 (relative
    distances up to 96: the logarithmic far buckets on both sides are populated)"""
    B, H, Fd, T = 2, HEADS, 17, 97
    bucket = _buckets(T, "net")
    assert int((torch.bincount(bucket.reshape(-1), minlength=NUM_BUCKETS) > 0).sum()) == NUM_BUCKETS - 1     # (bucket 0 never occurs: distance 0 counts as "ahead")
    W = _rand(NUM_BUCKETS, H, seed=720, scale=2.0)
    qk, v, go = _rand(B, H * 2 * Fd, T, seed=721, scale=2.0), _rand(B, H, Fd, T, seed=722), _rand(B, H, Fd, T, seed=723)
    Wr = W.double().requires_grad_()
    q4 = qk.double().reshape(B, H, 2 * Fd, T).permute(0, 1, 3, 2)
    sim = (torch.einsum("bhnd,bhmd->bhnm", q4[..., :Fd], q4[..., Fd:]) + Wr[bucket].permute(2, 0, 1)[None]) * (float(Fd) ** -0.5)
    out = torch.einsum("bhnm,bhmd->bhnd", sim.softmax(-1), v.double().permute(0, 1, 3, 2)).permute(0, 1, 3, 2)
    ref = torch.autograd.grad((out * go.double()).sum(), Wr)[0]
    qd, vd, god = qk.to(DEV), v.to(DEV), go.to(DEV)
    bias = W[bucket].permute(2, 0, 1).contiguous().to(DEV)
    o, probs = _filled((B, H, Fd, T), NAN), _filled((B, H, T, T), NAN)
    sc = float(Fd) ** -0.5
    L.call("aid_time_attention", L.AttentionParams(qd.data_ptr(), vd.data_ptr(), o.data_ptr(), probs.data_ptr(), B, H, Fd, T, sc, bias.data_ptr()))
    gq, gv, ws = _filled(tuple(qd.shape), NAN), _filled(tuple(vd.shape), NAN), _filled((B, H, T, T), NAN)
    L.call("aid_time_attention_bwd", L.AttentionBwdParams(qd.data_ptr(), vd.data_ptr(), probs.data_ptr(), god.data_ptr(), gq.data_ptr(), gv.data_ptr(),
                                                          B, H, Fd, T, sc, 0, ws.data_ptr()))
    got = _relpos_run(L, ws, bucket.to(torch.int32).to(DEV), 0)
    e = rel_l2(got.cpu(), ref)
    print(f"relpos_bwd chained after attention, T = 97: dW rel-L2 vs float64 autograd = {e:.2e}")
    assert bool(torch.isfinite(got).all()) and e < 2e-5


# ---------------------------------------------------------------------------------------------------------
# aid_scale_bwd
@pytest.mark.parametrize("with_dmod", [False, True], ids=["nodmod", "dmod"])
@pytest.mark.parametrize("with_mod", [False, True], ids=["nomod", "mod"])
@pytest.mark.parametrize("C", [40, 264])             # 264: two workgroups, the second with 8 live threads; 33 channels per group
def test_scale_bwd(L, C, with_mod, with_dmod):
    """d scale[b,c] = S[b,c] / scale[b,c] pulled back through scale = gamma_c (1 + a[b,c]) inv[b,g]: float64 autograd of that expression with the
    upstream S / scale (0 where scale is exactly 0).  S, scale, mod and dmod are column slices of wider buffers (leading dimension > C)."""
    B, G, WIDE, OFF = 3, 8, C + 24, 8
    gamma = 1 + 0.3 * _rand(C, seed=800)
    a = 0.4 * _rand(B, C, seed=801) if with_mod else None
    stats = torch.stack([_rand(B, G, seed=802), 0.5 + _rand(B, G, seed=803).abs()], -1).contiguous()       # (mean, inv) of the forward
    S = _rand(B, C, seed=804)
    g_, a_ = gamma.double().requires_grad_(), (torch.zeros(B, C) if a is None else a).double().requires_grad_()
    sc64 = g_[None] * (1 + a_) * stats[..., 1].double().repeat_interleave(C // G, dim=1)
    scale = sc64.detach().float()
    scale[1, C - 3] = 0.0                                                                                    # the sc == 0 guard
    up = torch.where(scale != 0, S.double() / scale.double(), torch.zeros(B, C, dtype=torch.float64))
    dgamma_ref, dmod_ref = torch.autograd.grad((sc64 * up).sum(), (g_, a_))

    def wide(t, fill=0.0):
        buf = _filled((B, WIDE), fill)
        if t is not None:
            buf[:, OFF:OFF + C] = t.to(DEV)
        return buf

    Sw, scw, mw = wide(S, 7.0), wide(scale, 0.0), wide(a, 7.0)
    gd, st = gamma.to(DEV), stats.to(DEV)
    res = []
    for accumulate in (0, 1):
        dmw = wide(torch.full((B, C), NAN), SENT)
        dg = _filled((C + 2,), SENT)
        dg[1:-1] = 0.25 if accumulate else NAN
        sl = lambda t: t[:, OFF:OFF + C]
        p = L.ScaleBwdParams(sl(Sw).data_ptr(), WIDE, sl(scw).data_ptr(), WIDE, gd.data_ptr(), sl(mw).data_ptr() if with_mod else None, WIDE if with_mod else 0,
                             st.data_ptr(), dg[1:].data_ptr(), sl(dmw).data_ptr() if with_dmod else None, WIDE if with_dmod else 0, B, C, G, accumulate)
        L.call("aid_scale_bwd", p)
        torch.cuda.synchronize()
        assert float(dg[0]) == SENT and float(dg[-1]) == SENT
        assert bool((dmw[:, :OFF] == SENT).all()) and bool((dmw[:, OFF + C:] == SENT).all())
        res.append((dg[1:-1].clone(), sl(dmw).clone()))
    (dg0, dm0), (dg1, dm1) = res
    assert torch.equal(dg1, dg0 + 0.25)                                                                     # accumulate: one float32 addition onto the old value
    e = rel_l2(dg0.cpu(), dgamma_ref)
    print(f"scale_bwd C={C} mod={int(with_mod)} dmod={int(with_dmod)}: dgamma rel-L2 {e:.2e}", end="")
    assert bool(torch.isfinite(dg0).all()) and e < 2e-6
    if with_dmod:
        e = rel_l2(dm0.cpu(), dmod_ref)
        print(f", dmod rel-L2 {e:.2e}", end="")
        assert bool(torch.isfinite(dm0).all()) and e < 2e-6 and torch.equal(dm0, dm1)                       # (dmod is written, never accumulated)
        assert float(dm0[1, C - 3]) == 0.0                                                                  # scale == 0: contributes exactly nothing
    else:
        assert bool(torch.isnan(dm0).all())                                                                 # dmod = NULL: nothing written there
    print()


# ---------------------------------------------------------------------------------------------------------
# aid_modulation_bwd
def _modulation_run(L, dmod, emb, W, accumulate):
    B, N = dmod.shape
    E = emb.shape[1]
    nfl = B * ((N + 127) // 128) * E
    part = _filled((nfl + 64,), SENT)
    part[:nfl] = NAN
    dW, dbias, demb = (_filled(s, 0.25 if accumulate else NAN) for s in ((N, E), (N,), (B, E)))
    demb.fill_(NAN)                                                 # (an intermediate gradient: written, never accumulated)
    p = L.ModulationBwdParams(dmod.data_ptr(), emb.data_ptr(), W.data_ptr(), dW.data_ptr(), dbias.data_ptr(), demb.data_ptr(), B, E, N, int(accumulate),
                              part.data_ptr(), nfl)
    try:
        L.call("aid_modulation_bwd", p)
    finally:
        torch.cuda.synchronize()
        assert bool((part[nfl:] == SENT).all()), "aid_modulation_bwd wrote behind B * ceil(N / 128) * E floats of `part`"
    return dW, dbias, demb


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("E", [48, 256, 300])        # 300: second, ragged trip of the e += 256 loop; fold grid of 2
@pytest.mark.parametrize("N", [1, 127, 128, 129, 1000])        # chunks of 128 rows: one ragged, one full, full + 1 row, 7 full + 104
def test_modulation_bwd(L, N, E, B):
    dmod, emb, W = _rand(B, N, seed=900 + N), _rand(B, E, seed=901 + E), _rand(N, E, seed=902 + B, scale=1 / math.sqrt(E))
    e_, W_, b_ = emb.double().requires_grad_(), W.double().requires_grad_(), torch.zeros(N, dtype=torch.float64).requires_grad_()
    refs = torch.autograd.grad(((e_ @ W_.t() + b_) * dmod.double()).sum(), (W_, b_, e_))
    dev = [t.to(DEV) for t in (dmod, emb, W)]
    got0 = _modulation_run(L, *dev, accumulate=0)
    got1 = _modulation_run(L, *dev, accumulate=1)
    assert torch.equal(got1[0], got0[0] + 0.25) and torch.equal(got1[1], got0[1] + 0.25) and torch.equal(got1[2], got0[2])
    errs = [rel_l2(g.cpu(), r) for g, r in zip(got0, refs)]
    print(f"modulation_bwd N={N} E={E} B={B}: dW {errs[0]:.2e} dbias {errs[1]:.2e} demb {errs[2]:.2e}")
    assert all(bool(torch.isfinite(g).all()) for g in got0) and max(errs) < 1e-5


def test_modulation_bwd_refuses_short_scratch(L):
    """one float fewer than B * ceil(N / 128) * E in part_floats: refused before the first launch, nothing is written"""
    B, N, E = 5, 129, 300
    dev = [t.to(DEV) for t in (_rand(B, N, seed=1), _rand(B, E, seed=2), _rand(N, E, seed=3))]
    _modulation_run(L, *dev, accumulate=1)                          # (the exact size is accepted)
    nfl = B * 2 * E
    part = _filled((nfl,), SENT)
    dW, dbias, demb = _filled((N, E), 0.25), _filled((N,), 0.25), _filled((B, E), SENT)
    p = L.ModulationBwdParams(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dW.data_ptr(), dbias.data_ptr(), demb.data_ptr(), B, E, N, 1,
                              part.data_ptr(), nfl - 1)
    with pytest.raises(L.AidError):
        L.call("aid_modulation_bwd", p)
    torch.cuda.synchronize()
    assert bool((part == SENT).all()) and bool((demb == SENT).all()) and bool((dW == 0.25).all()) and bool((dbias == 0.25).all())


# ---------------------------------------------------------------------------------------------------------
# aid_embed_bwd
EMBED_WIDTHS = {"net": (32, 128, 256, 48),           # the widths of the existing forward test: every loop runs once
                "wide": (160, 300, 260, 264)}        # every += 256 loop runs twice with a ragged tail (rff 160, 2 rff = 320, h0 300, h1 260, E 264)
EMBED_SEED = {"net": 41, "wide": 44}                 # seeds for which no ReLU pre-activation of the float64 reference lies within 1e-4 of 0 (checked below)
SIGMAS = [-2.1, -0.3, 0.4]


@functools.lru_cache(maxsize=None)
def _embed_case(widths, B):
    """parameters, the upstream gradient and the float64 reference: the RFF angle in float32 exactly as oracle.unet.embed forms it (2 pi sigma freq, the
    1e2-rad argument's rounding is part of the operation), everything from sin / cos onward in float64"""
    rff, h0, h1, E = EMBED_WIDTHS[widths]
    s0 = EMBED_SEED[widths]
    freq = 16 * _rand(1, rff, seed=s0)
    dims = [(h0, 2 * rff), (h1, h0), (E, h1)]
    Ws = [_rand(o, i, seed=s0 + 1 + k, scale=1 / math.sqrt(i)) for k, (o, i) in enumerate(dims)]
    bs = [0.1 * _rand(o, seed=s0 + 5 + k) for k, (o, i) in enumerate(dims)]
    sig = torch.tensor(SIGMAS[:B]).reshape(B, 1)
    demb = _rand(B, E, seed=s0 + 9)
    table = (2 * math.pi * sig * freq).double()                     # float32 product, as the reference forms it
    x = torch.cat([torch.sin(table), torch.cos(table)], dim=1)
    params = [t.double().requires_grad_() for pair in zip(Ws, bs) for t in pair]
    margin = float("inf")
    for k in range(3):
        z = x @ params[2 * k].t() + params[2 * k + 1]
        margin = min(margin, float(z.detach().abs().min()))
        x = torch.relu(z)
    grads = torch.autograd.grad((x * demb.double()).sum(), params)
    return {"freq": freq, "W": Ws, "b": bs, "sig": sig, "demb": demb, "emb": x.detach(), "grads": grads, "margin": margin}


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("widths", ["net", "wide"])
def test_embed_bwd(L, widths, B):
    rff, h0, h1, E = EMBED_WIDTHS[widths]
    c = _embed_case(widths, B)
    assert c["margin"] > 1e-4, c["margin"]                          # no ReLU gate on the edge (reference alone, before the GPU is touched)
    d = [t.to(DEV).contiguous() for t in (c["sig"].reshape(-1), c["freq"], c["W"][0], c["b"][0], c["W"][1], c["b"][1], c["W"][2], c["b"][2])]
    emb = _filled((B, E), NAN)
    fwd = L.EmbedParams(*[t.data_ptr() for t in d], emb.data_ptr(), B, rff, h0, h1, E)
    L.call("aid_embed", fwd)
    e_fwd = rel_l2(emb.cpu(), c["emb"])
    assert e_fwd < 2e-5
    dembd = c["demb"].to(DEV)
    res = []
    for accumulate in (0, 1):
        outs = [_filled((t.numel() + 2,), SENT) for pair in zip(c["W"], c["b"]) for t in pair]        # dw0 db0 dw1 db1 dw2 db2, a sentinel on each side
        for o in outs:
            o[1:-1] = 0.25 if accumulate else NAN
        L.call("aid_embed_bwd", L.EmbedBwdParams(fwd, dembd.data_ptr(), *[o[1:].data_ptr() for o in outs], accumulate))
        torch.cuda.synchronize()
        assert all(float(o[0]) == SENT and float(o[-1]) == SENT for o in outs)
        res.append([o[1:-1].clone() for o in outs])
    names = ("dw0", "db0", "dw1", "db1", "dw2", "db2")
    errs0 = [rel_l2(g.cpu(), r.reshape(-1)) for g, r in zip(res[0], c["grads"])]
    errs1 = [rel_l2(g.cpu().double() - 0.25, r.reshape(-1)) for g, r in zip(res[1], c["grads"])]
    print(f"embed_bwd {widths} B={B}: gate margin {c['margin']:.1e}, forward {e_fwd:.1e}; accumulate=0 " + " ".join(f"{n} {e:.1e}" for n, e in zip(names, errs0))
          + "; accumulate=1 " + " ".join(f"{n} {e:.1e}" for n, e in zip(names, errs1)))
    assert all(bool(torch.isfinite(g).all()) for g in res[0] + res[1])
    assert max(errs0) < 2e-5 and max(errs1) < 2e-5       # (old + g * a contracts into one fma: accumulate = 1 is not 0.25 + the accumulate = 0 bits)
