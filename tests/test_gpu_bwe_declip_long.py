"""GPU tests of bandwidth extension of whole recordings that are also clipped and have dropouts (csrc/aid_bwe_declip_long.hip,
bwe_declip_long.py, Sampler.predict_bwe_declip_long): the operator of the clipped filter against float64 torch expressions and bit for bit
against the two existing kernels it fuses, on concurrent streams and sliced; aid_gap_states bit-exact against Python indexing; the mode
without clipping and dropouts against predict_bwe_long; the reduced HIP network against the oracle, across batch compositions and pooled.
Toy and reduced-size models only."""
import math

import pytest
import torch

from conftest import rel_l2
from test_bwe_long_host import BWE_CASES
from test_gpu_bwe_long import SENT, _corr64, _lowpass, _on_device, _signals, _small_net, _strided

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- the operator against float64 ----------------------------------------------------------------------------------------------------------
def _levels(c64, k):
    """One level per item: the midpoint of the widest gap between neighbouring sorted |c64| of the item's state-0 samples in the 40-80 %
    quantile range (0.5 with fewer than two state-0 samples) -> (levels float32 [B], the smallest half gap relative to its level)"""
    levels, margin = [], math.inf
    for b in range(c64.shape[0]):
        a = c64[b][k[b] == 0].abs().sort().values
        n = a.numel()
        if n < 2:
            levels.append(0.5)
            continue
        lo = int(0.4 * n)
        cand = a[lo:max(int(0.8 * n), lo + 2)]
        if cand.numel() < 2:
            cand = a
        gaps = cand[1:] - cand[:-1]
        j = int(gaps.argmax())
        level = float(torch.tensor(float(cand[j] + cand[j + 1]) / 2, dtype=torch.float32))
        levels.append(level)
        margin = min(margin, min(level - float(cand[j]), float(cand[j + 1]) - level) / level)
    return torch.tensor(levels, dtype=torch.float32), margin


def _references(x, v, gy, h, state, clip):
    """apply (plane 0), the pre-clip plane, the adjoint at x, autograd's gradient of the apply, and the Jacobian at x applied to v -- float64
    torch expressions on the host"""
    k = state.expand_as(x)
    K = h.numel()
    P = (K - 1) // 2
    cb = clip.double()[:, None]
    g64 = gy.double()
    zero = torch.zeros_like(g64)

    def apply64(xx):
        c = _corr64(torch.where(k == -2, zero, xx), h, P)
        return torch.where(k == 1, xx, torch.where(k == 0, torch.maximum(torch.minimum(c, cb), -cb), zero)), c
    xr = x.double().clone().requires_grad_()
    obs, c = apply64(xr)
    (auto,) = torch.autograd.grad(obs, xr, g64)
    obs, c = obs.detach(), c.detach()
    gate = (k == 0) & (c >= -cb) & (c <= cb)
    a = _corr64(torch.where(gate, g64, zero), h.flip(0), K - 1 - P)
    adj = torch.where(k == -2, zero, torch.where(k == 1, a + g64, a))
    cv = _corr64(torch.where(k == -2, zero, v.double()), h, P)
    jv = torch.where(k == 1, v.double(), torch.where(gate, cv, zero))
    return obs, torch.where(k == 0, c, zero), adj, auto, jv, c


@pytest.mark.parametrize("B,L", [(1, 1000), (3, 4097), (2, 5)])
@pytest.mark.parametrize("K", [1, 8, 9, 33, 1025])
@pytest.mark.parametrize("shared", [False, True])
def test_fir_clip_observed_against_float64_on_strided_misaligned_rows(B, L, K, shared):
    """Apply and adjoint within rel-L2 1e-6 of the float64 expression (the bar FIRObserved is held to), the adjoint also against autograd of the
    float64 apply and by the dot product with the Jacobian; what the state selects is exact; plane 1 is FIRObserved's apply at state 0.
    Every item clips at its own level, placed in the widest gap of the sorted |c| so that float32 and float64 agree on which samples clip."""
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.bwe_declip_long import FIRClipObserved
    from audio_inpainting_diffusion_amd.bwe_long import FIRObserved
    x, v, gy, h, state = _signals(B, L, K, 7 + L + B + K)
    if shared:
        state = state[:1]
    k = state.expand(B, L)
    c64 = _corr64(torch.where(k == -2, torch.zeros_like(x), x), h, (K - 1) // 2)
    clip, margin = _levels(c64, k)
    print(f"FIRClipObserved B={B} L={L} K={K} shared={shared}: levels {[round(float(c), 4) for c in clip]}, smallest half gap / level = {margin:.2e}")
    assert margin >= 1e-4 and (L < 1000 or len(set(clip.tolist())) == B)     # (every item its own level)
    want0, want_pre, want1, auto, jv, c = _references(x, v, gy, h, state, clip)
    assert rel_l2(want1, auto) <= 1e-12
    if L >= 1000:      # both sides of the clipper are exercised
        clipped = ((k == 0) & (c.abs() > clip.double()[:, None])).sum(1)
        assert bool((clipped > 0).all()) and bool((clipped < (k == 0).sum(1)).all())
    table = torch.cat([h, clip]).to(DEV)
    (_, xd), (_, gd), (_, kd) = _on_device(x, 1), _on_device(gy, 0), _on_device(state, 2)
    fir_c = FIRObserved(h, kd).apply(xd).cpu()
    errs = {}
    for out_shift in (0, 1, 3):
        obuf = torch.full((2 * B, L + 3), SENT, device=DEV)
        od = obuf[:, out_shift:out_shift + L]
        guard = torch.full((2, B, L + 3), SENT, device=DEV)
        _lib.call("aid_fir_clip_observed", _lib.FirObservedParams(xd.data_ptr(), None, kd.data_ptr(), table.data_ptr(), od.data_ptr(),
                                                                  B, K, 0, L, L + 3, 0, 0 if shared else L + 3, L + 3))
        got0, pre = od[:B].cpu(), od[B:].cpu()
        abuf = torch.full((B, L + 3), SENT, device=DEV)
        ad = abuf[:, out_shift:out_shift + L]
        _lib.call("aid_fir_clip_observed", _lib.FirObservedParams(gd.data_ptr(), od[B:].data_ptr(), kd.data_ptr(), table.data_ptr(), ad.data_ptr(),
                                                                  B, K, 1, L, L + 3, L + 3, 0 if shared else L + 3, L + 3))
        got1 = ad.cpu()
        errs[(out_shift, 0)], errs[(out_shift, "pre")], errs[(out_shift, 1)] = rel_l2(got0, want0), rel_l2(pre, want_pre), rel_l2(got1, want1)
        pad = torch.ones(2 * B, L + 3, dtype=torch.bool)
        pad[:, out_shift:out_shift + L] = False
        assert bool((obuf.cpu()[pad] == SENT).all()) and bool((abuf.cpu()[pad[:B]] == SENT).all()) and bool((guard == SENT).all())
        # known outputs are x bit for bit; no observation: 0.0; a clipped sample is the level itself; plane 1 is FIRObserved's sum at state 0
        assert torch.equal(got0[k == 1], x[k == 1]) and bool((got0[k < 0] == 0).all()) and bool((pre[k != 0] == 0).all())
        assert torch.equal(pre[k == 0], fir_c[k == 0])
        sat = (k == 0) & (c.abs() > clip.double()[:, None])
        assert torch.equal(got0[sat].abs(), clip[:, None].expand(B, L)[sat]) and torch.equal(got0[(k == 0) & ~sat], pre[(k == 0) & ~sat])
        assert bool((got1[k == -2] == 0).all())
    print(f"FIRClipObserved B={B} L={L} K={K} shared={shared}: worst rel-L2 vs float64 = {max(errs.values()):.2e}")
    assert all(e <= 1e-6 for e in errs.values()), errs
    # the operator object (contiguous signals; the state keeps its row stride)
    op = FIRClipObserved(h, kd, clip)
    assert op.shared_mask is False and (op.K, op.B, op.L, op.items_held) == (K, B, L, B)
    ax, atg = op.apply(xd).cpu(), op.adjoint(gd).cpu()
    assert rel_l2(ax, want0) <= 1e-6 and rel_l2(op(xd).cpu(), want0) <= 1e-6
    assert rel_l2(atg, want1) <= 1e-6 and rel_l2(atg, auto) <= 1e-6
    lhs, rhs = float((jv * gy.double()).sum()), float((v.double() * atg.double()).sum())
    assert abs(lhs - rhs) <= 1e-6 * float(jv.norm() * gy.double().norm())
    with pytest.raises(AttributeError, match="no projection exists for the clipped filter"):
        op.project(xd, xd)
    # refusals of the launcher: checked on the host, nothing is launched
    o = torch.zeros(2 * B, L, device=DEV)
    for bad in (dict(mode=2), dict(mode=3), dict(mode=-1), dict(mode=1, y=None), dict(mode=1, y_ld=L - 1), dict(B=0), dict(K=0), dict(x_ld=L - 1),
                dict(out_ld=L - 1), dict(state_ld=L - 1)):
        kw = dict(mode=0, B=B, K=K, x_ld=L + 3, out_ld=L, state_ld=0 if shared else L + 3, y=gd.data_ptr(), y_ld=L + 3)
        kw.update(bad)
        with pytest.raises(_lib.AidError):
            _lib.call("aid_fir_clip_observed", _lib.FirObservedParams(xd.data_ptr(), kw["y"], kd.data_ptr(), table.data_ptr(), o.data_ptr(), kw["B"], kw["K"],
                                                                      kw["mode"], L, kw["x_ld"], kw["y_ld"], kw["state_ld"], kw["out_ld"]))
    assert bool((o == 0).all())
    # (one state row serves any number of levels; B > 1 state rows need B levels)
    for bad in ([[0.5] * (B + 1)] if kd.shape[0] > 1 else []) + [[0.0] * B, [-1.0] * B, [float("nan")] * B, []]:
        with pytest.raises(_lib.AidError):
            FIRClipObserved(h, kd, bad)
    with pytest.raises(_lib.AidError, match="matching apply"):
        FIRClipObserved(h, kd, clip).adjoint(gd)


# ---- bit for bit against the existing kernels ----------------------------------------------------------------------------------------------
def _clip_states(k):
    """the states of ClipObserved: 0 -> 0, 1 -> 1, < 0 -> -1"""
    return torch.where(k < 0, -torch.ones_like(k), k)


@pytest.mark.parametrize("K", [9, 1025])
@pytest.mark.parametrize("shared", [False, True])
def test_apply_and_adjoint_are_the_two_existing_kernels_composed_bit_for_bit(K, shared):
    from audio_inpainting_diffusion_amd.bwe_declip_long import FIRClipObserved
    from audio_inpainting_diffusion_amd.bwe_long import FIRObserved
    from audio_inpainting_diffusion_amd.declip_long import ClipObserved
    B, L = 3, 4097
    x, _, gy, h, state = _signals(B, L, K, 31 + K)
    kd = (state[:1] if shared else state).to(DEV)
    xd, gd = x.to(DEV), gy.to(DEV)
    clip = torch.tensor([0.4, 0.8, 1.3])                                     # (c ~ N(0, 1): every item clips some samples and passes others)
    op, fir, clp = FIRClipObserved(h, kd, clip), FIRObserved(h, kd), ClipObserved(_clip_states(kd), clip)
    c = fir.apply(xd)
    want = clp.apply(c)
    got = op.apply(xd)
    assert torch.equal(got, want) and not torch.equal(want, c)
    assert torch.equal(op.adjoint(gd), fir.adjoint(clp.adjoint(gd))) and not torch.equal(op.adjoint(gd), fir.adjoint(gd))
    # every level +inf: FIRObserved's bits
    inf = FIRClipObserved(h, kd, [math.inf] * B)
    assert torch.equal(inf.apply(xd), c) and torch.equal(inf.adjoint(gd), fir.adjoint(gd))
    assert torch.equal(FIRClipObserved(h, kd, torch.full((B,), math.inf, device=DEV)).apply(xd), c)


@pytest.mark.parametrize("shared", [False, True])
def test_with_one_unit_tap_apply_and_adjoint_are_clip_observed_bit_for_bit(shared):
    from audio_inpainting_diffusion_amd.bwe_declip_long import FIRClipObserved
    from audio_inpainting_diffusion_amd.declip_long import ClipObserved
    B, L = 3, 4097
    x, _, gy, _, state = _signals(B, L, 1, 5)
    kd = (state[:1] if shared else state).to(DEV)
    xd, gd = x.to(DEV), gy.to(DEV)
    clip = torch.tensor([0.4, 0.8, 1.3])
    op, clp = FIRClipObserved(torch.tensor([1.0]), kd, clip), ClipObserved(_clip_states(kd), clip)
    assert torch.equal(op.apply(xd), clp.apply(xd)) and torch.equal(op.adjoint(gd), clp.adjoint(gd))      # (torch.equal: -0.0 == 0.0)
    assert not torch.equal(op.apply(xd), xd)


# ---- concurrency and slicing ---------------------------------------------------------------------------------------------------------------
def test_apply_and_adjoint_pairs_on_two_concurrent_streams_do_not_mix_their_kept_planes():
    """One operator of four items, its halves used by two streams at once: both applies first, then both adjoints, so that each adjoint must
    find the pre-clip plane its own stream kept."""
    from audio_inpainting_diffusion_amd.bwe_declip_long import FIRClipObserved
    B, L, K = 4, 3000, 33
    x, _, gy, h, state = _signals(B, L, K, 9)
    op = FIRClipObserved(h, state.to(DEV), [0.3, 0.6, 0.9, 1.2])
    xd, gd = x.to(DEV), gy.to(DEV)
    halves = [op.rows(0, 2), op.rows(2, 4)]
    seq = [(halves[i].apply(xd[2 * i:2 * i + 2]), halves[i].adjoint(gd[2 * i:2 * i + 2])) for i in range(2)]
    assert not torch.equal(seq[0][0], seq[1][0])
    # ... and one operator used for two inputs on two streams keeps one plane per stream
    alt = op.rows(0, 2)
    x2 = (xd[0:2] * 3).contiguous()
    want = [(alt.apply(xd[0:2]), alt.adjoint(gd[0:2])), (alt.apply(x2), alt.adjoint(gd[0:2]))]
    assert not torch.equal(want[0][1], want[1][1])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs, outs2 = [None, None], [None, None]
    cur = torch.cuda.current_stream()
    for s in streams:
        s.wait_stream(cur)
    for i, s in enumerate(streams):
        with torch.cuda.stream(s):
            outs[i] = [halves[i].apply(xd[2 * i:2 * i + 2])]
            outs2[i] = [alt.apply(xd[0:2] if i == 0 else x2)]
    for i, s in enumerate(streams):
        with torch.cuda.stream(s):
            outs[i].append(halves[i].adjoint(gd[2 * i:2 * i + 2]))
            outs2[i].append(alt.adjoint(gd[0:2]))
    for s in streams:
        cur.wait_stream(s)
    torch.cuda.synchronize()
    assert all(torch.equal(outs[i][j], seq[i][j]) for i in range(2) for j in range(2))
    assert all(torch.equal(outs2[i][j], want[i][j]) for i in range(2) for j in range(2))


@pytest.mark.parametrize("shared", [False, True])
def test_rows_is_the_operator_of_the_sliced_inputs(shared):
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.bwe_declip_long import FIRClipObserved
    B, L, K = 3, 4097, 33
    x, _, gy, h, state = _signals(B, L, K, 21)
    state = (state[:1] if shared else state).to(DEV)
    xd, gd, hd = x.to(DEV), gy.to(DEV), h.to(DEV)
    clip = torch.tensor([0.4, 0.8, 1.3], device=DEV)
    full = FIRClipObserved(hd, state, clip)
    sub = full.rows(1, 3)
    ref = FIRClipObserved(h, state if shared else state[1:3].contiguous(), [0.8, 1.3])
    assert full.rows(1, 3) is sub and (sub.K, sub.B, sub.L, sub.shared_mask, sub.items_held) == (K, 2, L, False, 2) and sub.state.shape[0] == (1 if shared else 2)
    assert sub.taps.data_ptr() == hd.data_ptr() and (not shared or sub.state.data_ptr() == state.data_ptr())       # taps and a shared state row stay shared
    assert torch.equal(sub.apply(xd[1:3]), ref.apply(xd[1:3])) and torch.equal(sub.adjoint(gd[1:3]), ref.adjoint(gd[1:3]))
    whole = full.apply(xd)
    assert torch.equal(sub.apply(xd[1:3]), whole[1:3]) and torch.equal(sub.adjoint(gd[1:3]), full.adjoint(gd)[1:3])
    assert not torch.equal(sub.apply(xd[1:3]), full.rows(0, 2).apply(xd[1:3]))                                     # (the levels differ)
    for lo, hi in ((2, 2), (-1, 2), (1, 4)):
        with pytest.raises(_lib.AidError):
            full.rows(lo, hi)
    with pytest.raises(_lib.AidError):
        full.apply(xd[:2])                                                                                         # (one level per item: exactly B items)


# ---- aid_gap_states ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L,end,K", BWE_CASES)
@pytest.mark.parametrize("rows", ["per recording", "shared"])
def test_gap_states_is_bit_exact_against_python_indexing(N, L, end, K, rows):
    from test_bwe_declip_long_host import _mask
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.bwe_declip_long import bwe_declip_gather, gap_states, window_state
    from audio_inpainting_diffusion_amd.bwe_long import bwe_gather, bwe_plan
    from audio_inpainting_diffusion_amd.restore import job_table
    R = 3
    A, B = bwe_plan(R, N, L, end, K)
    _, rec = _strided(R, N, 1 + N, 0)
    _, out = _strided(R, N, 2 + N, 1)
    rec_d = torch.empty(R, N + 3, device=DEV)[:, :N].copy_(rec)
    out_d = torch.empty(R, N + 3, device=DEV)[:, 1:N + 1].copy_(out)
    mask = _mask(N, L, end, K, R if rows == "per recording" else 1, 3 + N)
    mask_d = torch.empty(mask.shape[0], N + 3, device=DEV)[:, 2:N + 2].copy_(mask)             # (rows strided and misaligned)
    levels = torch.tensor([0.25, 0.5, 2.0], device=DEV)
    i = torch.arange(L)
    changed = 0
    for jobs in (A, B, A + B):
        if not jobs:
            continue
        tab = job_table(jobs, DEV)
        y0, k0 = bwe_gather(rec_d, out_d, tab, L, K)
        y, k, c = bwe_declip_gather(rec_d, out_d, mask_d, levels, tab, L, K)
        assert y.shape == k.shape == (len(jobs), L) and torch.equal(c.cpu(), levels.cpu()[[r for r, *_ in jobs]])
        for j, (r, s, head, tail, lo, hi) in enumerate(jobs):
            k_ref = torch.from_numpy(window_state(N, L, K, s, head, tail, mask[r if mask.shape[0] > 1 else 0]))
            qc = (s + i).clamp(max=N - 1)
            y_ref = torch.where(k_ref == 1, out[r, qc], torch.where(k_ref == 0, rec[r, qc], torch.zeros(L)))
            assert torch.equal(k[j].cpu(), k_ref) and torch.equal(y[j].cpu(), y_ref), j
        diff = (k != k0)
        changed += int(diff.sum())
        assert torch.equal(y[~diff], y0[~diff]) and bool((k0[diff] == 0).all())                # everything else is untouched
        y1, k1 = y0.clone(), k0.clone()
        gap_states(y1, k1, mask_d, tab, R, N)                                                  # the launch alone, in place
        assert torch.equal(y1, y) and torch.equal(k1, k)
        y2, k2, _ = bwe_declip_gather(rec_d, out_d, None, levels, tab, L, K)                   # no mask: aid_bwe_gather's rows
        assert torch.equal(y2, y0) and torch.equal(k2, k0)
    assert changed > 0
    tab = job_table(A, DEV)
    y0 = torch.zeros(len(A), L, device=DEV)
    for bad in (dict(mask_ld=N - 1), dict(J=0), dict(J=65536), dict(R=0), dict(mask=None), dict(y=None), dict(m=None), dict(jobs=None)):
        kw = dict(J=len(A), R=R, mask_ld=N + 3, mask=mask_d.data_ptr(), y=y0.data_ptr(), m=y0.data_ptr(), jobs=tab.data_ptr())
        kw.update(bad)
        with pytest.raises(_lib.AidError):
            _lib.call("aid_gap_states", _lib.WindowGatherParams(None, None, kw["mask"], kw["y"], kw["m"], kw["jobs"], kw["J"], kw["R"], L, N, 0, 0, kw["mask_ld"]))
    assert bool((y0 == 0).all())


def test_an_invalid_job_row_of_gap_states_touches_nothing_outside_its_own_rows():
    """The table is device memory: a row with a recording outside [0, R), a negative or too large start is skipped -- its rows of y and m stay
    as they are -- and a valid row changes only its state-0 samples under a dropped sample below N.  The rows lie inside guarded buffers."""
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.restore import job_table
    R, N, L = 2, 300, 128
    mask = torch.ones(R, N)
    mask[0, 10:40] = 0
    mask[1, 190:] = 0
    mask_d = mask.to(DEV)
    jobs = [(R, 0, 0, 0, 0, L), (-1, 0, 0, 0, 0, L), (0, -4, 0, 0, 0, L), (0, N, 0, 0, 0, L), (1, 200, 0, 0, -5, 10 * L), (1 << 40, 1 << 40, 5, 5, 0, L), (0, 7, 0, 0, 0, L),
            (0, 0, 10 * L, 0, 0, L)]
    J = len(jobs)
    tab = job_table(jobs, DEV)
    pad = 64
    g = torch.Generator().manual_seed(3)
    k0 = torch.randint(-2, 2, (J, L), generator=g).float()
    k0[:, 100:] = 0                                                          # (state 0 also beyond the end of recording 1's window at s = 200)
    y0 = torch.randn(J, L, generator=g)
    bufs = [torch.full((pad + J * L + pad,), SENT, device=DEV) for _ in range(2)]
    y, k = (b[pad:-pad] for b in bufs)
    y.copy_(y0.reshape(-1))
    k.copy_(k0.reshape(-1))
    _lib.call("aid_gap_states", _lib.WindowGatherParams(None, None, mask_d.data_ptr(), y.data_ptr(), k.data_ptr(), tab.data_ptr(), J, R, L, N, 0, 0, N))
    assert all(bool((b[:pad] == SENT).all()) and bool((b[-pad:] == SENT).all()) for b in bufs)
    y, k = y.reshape(J, L).cpu(), k.reshape(J, L).cpu()
    for j in (0, 1, 2, 3, 5):
        assert torch.equal(y[j], y0[j]) and torch.equal(k[j], k0[j]), j
    for j, (r, s) in ((4, (1, 200)), (6, (0, 7)), (7, (0, 0))):
        n_in = min(L, N - s)
        drop = torch.zeros(L, dtype=torch.bool)
        drop[:n_in] = (mask[r, s:s + n_in] == 0) & (k0[j, :n_in] == 0)
        assert bool(drop.any()) and bool((~drop).any())
        assert torch.equal(k[j], torch.where(drop, -torch.ones(L), k0[j])) and torch.equal(y[j], torch.where(drop, torch.zeros(L), y0[j])), j
    assert bool((k[4, 100:] == 0).all())                                     # samples at or past N are not the mask's


# ---- the mode without clipping and dropouts: predict_bwe_long ------------------------------------------------------------------------------
def test_without_clipping_and_dropouts_the_result_is_predict_bwe_long_bit_for_bit():
    """Toy sampler, L = 4096, K = 33, two recordings of three windows: clip_value = None, mask = None gives predict_bwe_long's bits with the same
    seeds (the levels travel as +inf), and so does a mask of ones, which adds the aid_gap_states launches."""
    from test_gpu_generic import _sampler
    L, K, T = 4096, 33, 3
    N = 2 * L + L // 3
    taps = _lowpass(K)
    clean = torch.stack([torch.randn(N, generator=torch.Generator().manual_seed(50 + r)) for r in range(2)]) * 0.063
    y = _corr64(clean, taps, (K - 1) // 2).float().to(DEV)
    smp = _sampler(L, T, 0.25, **{"data_consistency.use": False})
    smp.seeds = [99]
    ref = smp.predict_bwe_long(y, taps, "firwin", seeds=[3, 4])
    n0 = smp.n_evals
    out = smp.predict_bwe_declip_long(y, taps, "firwin", seeds=[3, 4])
    assert smp.n_evals - n0 == 6 * (2 * T - 1) and smp.seeds == [99] and out.is_cuda and out.shape == (2, N)
    assert torch.equal(out, ref) and not torch.equal(out, y)
    assert torch.equal(smp.predict_bwe_declip_long(y, taps, "firwin", clip_value=None, mask=torch.ones(N), seeds=[3, 4]), ref)
    # ... and clipping changes it
    assert not torch.equal(smp.predict_bwe_declip_long(y.clamp(-0.02, 0.02), taps, "firwin", clip_value=0.02, seeds=[3, 4]), ref)


# ---- reduced HIP network -------------------------------------------------------------------------------------------------------------------
def test_hip_network_pass_a_and_pass_b_shaped_windows_vs_oracle():
    """Item 0 is shaped as a window of pass A: the first P existing samples unobserved, a 200-sample dropout, the last Q existing samples
    unobserved and the last 37 samples absent.  Item 1 as one of pass B: the first and last end - (K - 1) samples known.  K = 33, T = 3, guidance
    only; each item clips at its own level, the 0.7 quantile of its filtered |taps * x| (20-40 % of the filtered samples clip) --
    predict_resample with FIRClipObserved against the oracle sampler driven with the same operator written as a torch lambda.  Bound: the
    documented 5e-4 of test_gpu_degrade.py::test_hip_network_bwe_and_declipping_vs_oracle.
    Measured on one MI355X: rel-L2 = 4.25e-06 (30 % of the filtered samples of either item clip)."""
    from audio_inpainting_diffusion_amd.bwe_declip_long import FIRClipObserved
    from audio_inpainting_diffusion_amd.sampler import autoregressive_overlap
    smp, osmp, Ls = _small_net()
    K = 33
    P, Q, m = (K - 1) // 2, K - 1 - (K - 1) // 2, K - 1
    end = int(autoregressive_overlap(smp.args) * Ls)
    taps = _lowpass(K)
    clean = torch.stack([torch.randn(Ls, generator=torch.Generator().manual_seed(40 + i)) for i in range(2)]) * 0.063
    k = torch.zeros(2, Ls)
    k[0, :P] = -1
    k[0, Ls // 3:Ls // 3 + 200] = -1
    k[0, Ls - 37 - Q:Ls - 37] = -1
    k[0, Ls - 37:] = -2
    k[1, :end - m] = 1
    k[1, Ls - (end - m):] = 1

    def filt(x):
        return torch.nn.functional.conv1d(torch.where(k == -2, torch.zeros_like(x), x)[:, None], taps[None, None], padding="same").squeeze(1)
    c = filt(clean)
    clip = torch.stack([c[b][k[b] == 0].abs().quantile(0.7) for b in range(2)])
    frac = [float((c[b][k[b] == 0].abs() > clip[b]).float().mean()) for b in range(2)]
    assert all(0.2 <= f <= 0.4 for f in frac), frac

    def deg(x):
        cc = filt(x)
        return torch.where(k == 1, x, torch.where(k == 0, torch.maximum(torch.minimum(cc, clip[:, None]), -clip[:, None]), torch.zeros_like(x)))
    y = deg(clean)
    assert bool((y[0][k[0] < 0] == 0).all()) and torch.equal(y[1][k[1] == 1], clean[1][k[1] == 1]) and bool((y[k == 0].abs() <= clip[:, None].expand(2, Ls)[k == 0]).all())
    smp.seeds = [7, 8]
    out = smp.predict_resample(y.to(DEV), (2, Ls), FIRClipObserved(taps, k.to(DEV), clip))
    ref = osmp.predict_resample(y, (2, Ls), deg, seeds=[7, 8])
    e = rel_l2(out.cpu(), ref)
    print(f"HIP network, FIRClipObserved windows ({frac[0]:.0%} / {frac[1]:.0%} of the filtered samples clip): rel-L2 vs oracle = {e:.2e}")
    assert e <= 5e-4


def test_hip_network_result_across_batch_compositions_and_pooled():
    """Two recordings of N = 2 Ls + Ls // 3 samples (three windows each) low-passed with K = 33 taps, clipped at their own levels and with two
    dropouts each (one across a window border), T = 3.  Restored together, each alone, and with max_batch 1 against 8; form_batch is left
    unpinned, so the documented bound for results across batch compositions applies (<= 5e-6,
    tests/test_gpu_degrade.py::test_predict_bwe_batch_of_four_takes_the_sub_batch_streams).  The pooled call over the two recordings as two
    groups runs the same chunks and is bit-equal to the plain one; every window is a job: n_evals = jobs * (2 T - 1).
    Measured on one MI355X: all four comparisons 0.0 (bit-equal) -- the bound stays at the documented 5e-6."""
    from audio_inpainting_diffusion_amd.bwe_long import bwe_plan
    from audio_inpainting_diffusion_amd.sampler import autoregressive_overlap
    smp, _, Ls = _small_net()
    K, T = 33, 3
    end = int(autoregressive_overlap(smp.args) * Ls)
    N, step = 2 * Ls + Ls // 3, Ls - end
    taps = _lowpass(K)
    clean = torch.stack([torch.randn(N, generator=torch.Generator().manual_seed(70 + r)) for r in range(2)]) * 0.063
    filtered = _corr64(clean, taps, (K - 1) // 2).float()
    levels = [float(filtered[r].abs().quantile(0.7 + 0.1 * r)) for r in range(2)]
    mask = torch.ones(2, N)
    mask[0, step - 50:step + 150] = 0
    mask[0, 2 * step + Ls // 2:2 * step + Ls // 2 + 300] = 0
    mask[1, Ls // 4:Ls // 4 + 300] = 0
    mask[1, N - 100:] = 0
    rec = mask * torch.stack([filtered[r].clamp(-levels[r], levels[r]) for r in range(2)])
    A, B = bwe_plan(2, N, Ls, end, K)
    assert len(A) == 4 and len(B) == 2
    rec_d = rec.to(DEV)
    seeds = [31, 32]
    n0 = smp.n_evals
    both = smp.predict_bwe_declip_long(rec_d, taps, "firwin", clip_value=levels, mask=mask, max_batch=8, seeds=seeds)
    assert smp.n_evals - n0 == 6 * (2 * T - 1) and both.shape == (2, N) and bool(torch.isfinite(both).all()) and not torch.equal(both, rec_d)
    errs = {}
    for r in range(2):
        alone = smp.predict_bwe_declip_long(rec_d[r:r + 1], taps, "firwin", clip_value=levels[r], mask=mask[r], max_batch=8, seeds=seeds[r:r + 1])
        errs[f"recording {r} alone"] = rel_l2(alone.cpu(), both[r:r + 1].cpu())
    one = smp.predict_bwe_declip_long(rec_d, taps, "firwin", clip_value=levels, mask=mask, max_batch=1, seeds=seeds)
    for r in range(2):
        errs[f"recording {r} max_batch 1"] = rel_l2(one[r:r + 1].cpu(), both[r:r + 1].cpu())
    print("bwe_declip_long batch invariance, rel-L2:", {k: "%.2e" % v for k, v in errs.items()})
    n0 = smp.n_evals
    pooled = smp.predict_long_pooled("bwe_declip", [(rec_d[0:1], levels[0], mask[0]), (rec_d[1:2], [levels[1]], mask[1:2])], max_batch=8, seeds=seeds,
                                     filt=taps, filt_type="firwin")
    assert smp.n_evals - n0 == 6 * (2 * T - 1) and len(pooled) == 2
    assert torch.equal(torch.cat(pooled), both)
    assert all(e <= 5e-6 for e in errs.values()), errs
