"""GPU tests of bandwidth extension of whole recordings through an IIR filter (csrc/aid_bwe_iir_long.hip, bwe_iir_long.py,
Sampler.predict_bwe_iir_long): the operator of seed / filtered / known / unobserved / absent samples against the float64 model of
tests/test_bwe_iir_long_host.py and against IIRFilter, the gather bit-exact against Python indexing, the seeding property on the device, the two
passes stitched around a stub sampler, and the reduced HIP network against predict_bwe, the oracle, across batch compositions, pooled and
under a process group.  Toy and reduced-size models only."""
import functools
import math
import queue
import sys
import traceback
import os

import numpy as np
import pytest
import scipy.signal
import torch
import torch.multiprocessing as mp

from conftest import ROOT, rel_l2
from test_bwe_iir_long_host import END_HOST, L_HOST, N_HOST, iir_filters, iir_observed_torch
from test_gpu_bwe_long import SENT, _on_device, _strided

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _filter(order):
    """(b, a) of the given order: 16 from fixed poles of radius 0.8 (iir_coefficients and the conditioning check accept it)"""
    if order == 1:
        return np.array([0.2, 0.1]), np.array([1.0, -0.7])
    if order == 2:
        return scipy.signal.butter(2, 4000, fs=22050)
    if order == 4:
        return scipy.signal.cheby1(4, 0.05, 1000, fs=22050)
    if order == 8:
        return scipy.signal.cheby1(8, 0.05, 4000, fs=22050)
    a = np.poly(0.8 * np.exp(2j * np.pi * (np.arange(16) + 0.5) / 16)).real
    return np.random.default_rng(16).standard_normal(17) / 4, a


def _table(order):
    from audio_inpainting_diffusion_amd.bwe_iir_long import IIRTable
    t = IIRTable(_filter(order), "cheby1")
    assert t.order == order
    return t


def _states(B, L, order, rot, g):
    """rows whose leading seed runs are S = 0, order, order - 1, order + 3, L (row r takes entry r + rot), the four other states at random
    behind the run, a sample that ends the run, and a stray -3"""
    k = torch.randint(-2, 2, (B, L), generator=g).float()
    for r in range(B):
        S = min(L, (0, order, order - 1, order + 3, L)[(r + rot) % 5])
        k[r, :S] = -3
        if S < L:
            k[r, S] = (0.0, 1.0, -1.0, -2.0)[(r + rot) % 4]
        if S + 9 < L:
            k[r, S + 7] = -3                                                     # a -3 behind the run counts as -1
    return k


def _refs(x, y, gy, table, state):
    """apply, adjoint, projection, preparation in float64 on the host, and autograd's gradient of the apply"""
    k = state.double()
    x64, y64, g64 = x.double(), y.double(), gy.double()
    want = {m: iir_observed_torch(x64 if m != "adjoint" else g64, table.b, table.a, k, m, y64) for m in ("apply", "adjoint", "project", "prepare")}
    xr = x64.clone().requires_grad_()
    (auto,) = torch.autograd.grad(iir_observed_torch(xr, table.b, table.a, k), xr, g64)
    return want, auto


@pytest.mark.parametrize("B,L", [(1, 1000), (3, 4097), (2, 5), (2, 70001)])
@pytest.mark.parametrize("order", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("shared", [False, True])
def test_iir_observed_modes_against_float64_on_strided_misaligned_rows(B, L, order, shared):
    """apply, adjoint, projection (and the preparation) within rel-L2 1e-6 of the float64 model -- the bound the project holds IIRFilter and
    FIRObserved to --, the adjoint also against autograd and by the dot product; what the state selects is exact."""
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.bwe_iir_long import IIRObserved
    table = _table(order)
    hd = table.h.to(DEV)
    errs = {}
    for rot in range(5 if (shared or B == 1) else 3):
        g = torch.Generator().manual_seed(7 + L + B + order + rot)
        x, y, gy = (torch.randn(B, L, generator=g) for _ in range(3))
        state = _states(B, L, order, rot, g)
        if shared:
            state = state[:1]
        k = state.expand(B, L)
        want, auto = _refs(x, y, gy, table, state)
        assert rel_l2(want["adjoint"], auto) <= 1e-10
        (_, xd), (_, yd), (_, gd), (_, kd) = _on_device(x, 1), _on_device(y, 3), _on_device(gy, 0), _on_device(state, 2)
        absent, seedlike = (k <= -2) & (k != -3), (k == -3) | (k == -1)
        for out_shift, (mode, src, name) in zip((0, 1, 3, 2), ((0, xd, "apply"), (1, gd, "adjoint"), (2, xd, "project"), (3, xd, "prepare"))):
            obuf, od = _on_device(torch.full((B, L), SENT), out_shift)
            guard = torch.full((2, B, L + 3), SENT, device=DEV)
            _lib.call("aid_iir_observed", _lib.FirObservedParams(src.data_ptr(), yd.data_ptr() if mode == 2 else None, kd.data_ptr(), hd.data_ptr(), od.data_ptr(),
                                                                 B, order + 1, mode, L, L + 3, L + 3, 0 if shared else L + 3, L + 3))
            got = od.cpu()
            errs[(rot, name)] = rel_l2(got, want[name])
            pad = torch.ones(B, L + 3, dtype=torch.bool)
            pad[:, out_shift:out_shift + L] = False
            assert bool((obuf.cpu()[pad] == SENT).all()) and bool((guard == SENT).all())       # nothing outside the rows of out
            if mode in (0, 3):     # known outputs are x bit for bit; no observation: 0.0
                assert torch.equal(got[k == 1], x[k == 1]) and bool((got[k < 0] == 0).all())
            elif mode == 1:
                assert bool((got[absent] == 0).all())
            else:                  # known: the observation; no observation: x itself
                assert torch.equal(got[k == 1], y[k == 1]) and torch.equal(got[k < 0], x[k < 0])
        # the operator object (contiguous signals; the state keeps its row stride)
        op = IIRObserved(table, kd)
        assert op.shared_mask is False and (op.K, op.L, op.order) == (order + 1, L, order) and op.seed_error_bound == table.seed_error_bound
        ax, atg = op.apply(xd).cpu(), op.adjoint(gd).cpu()
        assert rel_l2(ax, want["apply"]) <= 1e-6 and rel_l2(op(xd).cpu(), want["apply"]) <= 1e-6
        assert rel_l2(atg, want["adjoint"]) <= 1e-6 and rel_l2(atg, auto) <= 1e-6
        assert rel_l2(op.project(xd, yd).cpu(), want["project"]) <= 1e-6 and rel_l2(op.prepare(xd).cpu(), want["prepare"]) <= 1e-6
        lhs, rhs = float((ax.double() * gy.double()).sum()), float((x.double() * atg.double()).sum())
        assert abs(lhs - rhs) <= 1e-6 * float(ax.double().norm() * gy.double().norm())
        assert seedlike.any() or L < 16
    print(f"IIRObserved B={B} L={L} order={order} shared={shared}: worst rel-L2 vs float64 = {max(errs.values()):.2e}")
    assert all(e <= 1e-6 for e in errs.values()), errs
    # refusals of the launcher: checked on the host, nothing is launched
    o = torch.zeros(B, L, device=DEV)
    for bad in (dict(mode=4), dict(mode=-1), dict(B=0), dict(K=1), dict(K=18), dict(x_ld=L - 1), dict(out_ld=L - 1), dict(state_ld=L - 1), dict(mode=2, y=None)):
        kw = dict(mode=0, B=B, K=order + 1, x_ld=L + 3, out_ld=L, state_ld=0 if shared else L + 3, y=yd.data_ptr())
        kw.update(bad)
        with pytest.raises(_lib.AidError):
            _lib.call("aid_iir_observed", _lib.FirObservedParams(xd.data_ptr(), kw["y"], kd.data_ptr(), hd.data_ptr(), o.data_ptr(), kw["B"], kw["K"], kw["mode"],
                                                                 L, kw["x_ld"], L + 3, kw["state_ld"], kw["out_ld"]))
    assert bool((o == 0).all())


@pytest.mark.parametrize("order", [4, 8])
@pytest.mark.parametrize("shared", [False, True])
def test_with_every_state_filtered_apply_and_adjoint_are_iir_filter_to_rounding(order, shared):
    """Every state 0, S = 0: degrade.IIRFilter(clamp=False)'s operator within rel-L2 1e-6.  Bit equality is not demanded: the recursion is chunked
    differently, so the fp64 partial sums differ; whether the outputs come out bit-equal is printed."""
    from audio_inpainting_diffusion_amd.bwe_iir_long import IIRObserved
    from audio_inpainting_diffusion_amd.degrade import IIRFilter
    B, L = 3, 4097
    g = torch.Generator().manual_seed(31 + order)
    xd, yd, gd = (torch.randn(B, L, generator=g).to(DEV) for _ in range(3))
    b, a = _filter(order)
    op, iir = IIRObserved(_table(order), torch.zeros(1 if shared else B, L, device=DEV)), IIRFilter(b, a, L, clamp=False, device=DEV)
    pairs = {"apply": (op.apply(xd), iir.apply(xd)), "adjoint": (op.adjoint(gd), iir.adjoint(gd)), "project": (op.project(xd, yd), iir.project(xd, yd))}
    print(f"IIRObserved vs IIRFilter, order {order}:", {n: ("bit-equal" if torch.equal(p, q) else f"rel-L2 {rel_l2(p.cpu(), q.cpu()):.2e}") for n, (p, q) in pairs.items()})
    assert all(rel_l2(p.cpu(), q.cpu()) <= 1e-6 for p, q in pairs.values())
    assert not torch.equal(pairs["apply"][0], xd)


def _op_case(B, L, order, seed):
    g = torch.Generator().manual_seed(seed)
    x, y, gy = (torch.randn(B, L, generator=g) for _ in range(3))
    return x, y, gy, _states(B, L, order, 1, g)


def test_iir_observed_apply_and_adjoint_on_two_concurrent_streams():
    """One operator of four items, its halves used by two streams at once (the pattern of the FIRObserved test)."""
    from audio_inpainting_diffusion_amd.bwe_iir_long import IIRObserved
    B, L, order = 4, 3000, 8
    x, _, gy, state = _op_case(B, L, order, 9)
    op = IIRObserved(_table(order), state.to(DEV))
    xd, gd = x.to(DEV), gy.to(DEV)
    halves = [op.rows(0, 2), op.rows(2, 4)]
    seq = [(halves[i].apply(xd[2 * i:2 * i + 2]), halves[i].adjoint(gd[2 * i:2 * i + 2])) for i in range(2)]
    assert not torch.equal(seq[0][0], seq[1][0])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [None, None]
    cur = torch.cuda.current_stream()
    for s in streams:
        s.wait_stream(cur)
    for i, s in enumerate(streams):
        with torch.cuda.stream(s):
            outs[i] = [halves[i].apply(xd[2 * i:2 * i + 2])]
    for i, s in enumerate(streams):
        with torch.cuda.stream(s):
            outs[i].append(halves[i].adjoint(gd[2 * i:2 * i + 2]))
    for s in streams:
        cur.wait_stream(s)
    torch.cuda.synchronize()
    assert all(torch.equal(outs[i][j], seq[i][j]) for i in range(2) for j in range(2))


@pytest.mark.parametrize("shared", [False, True])
def test_rows_is_the_operator_of_the_sliced_inputs(shared):
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.bwe_iir_long import IIRObserved
    B, L, order = 3, 4097, 8
    x, y, gy, state = _op_case(B, L, order, 21)
    state = (state[:1] if shared else state).to(DEV)
    xd, yd, gd = x.to(DEV), y.to(DEV), gy.to(DEV)
    table = _table(order)
    full = IIRObserved(table, state)
    sub = full.rows(1, 3)
    ref = IIRObserved(table, state if shared else state[1:3].contiguous())
    assert full.rows(1, 3) is sub and (sub.K, sub.L, sub.shared_mask) == (order + 1, L, False) and sub.state.shape[0] == (1 if shared else 2)
    assert sub.table is table and (not shared or sub.state.data_ptr() == state.data_ptr())                        # the table and a shared state row stay shared
    assert torch.equal(sub.apply(xd[1:3]), ref.apply(xd[1:3])) and torch.equal(sub.adjoint(gd[1:3]), ref.adjoint(gd[1:3]))
    assert torch.equal(sub.project(xd[1:3], yd[1:3]), ref.project(xd[1:3], yd[1:3]))
    assert torch.equal(sub.apply(xd[1:3]), full.apply(xd)[1:3])
    if not shared:
        assert not torch.equal(sub.apply(xd[1:3]), full.rows(0, 2).apply(xd[1:3]))                                 # (the states differ)
        for lo, hi in ((2, 2), (-1, 2), (1, 4)):
            with pytest.raises(_lib.AidError):
                full.rows(lo, hi)
        with pytest.raises(_lib.AidError):
            full.apply(xd[:2])


# ---- the gather --------------------------------------------------------------------------------------------------------------------------
GATHER_CASES = [(N_HOST, L_HOST, END_HOST), (1000, 256, 64), (100, 256, 64), (257, 256, 64), (449, 256, 64)]


@pytest.mark.parametrize("N,L,end", GATHER_CASES)
@pytest.mark.parametrize("order", [2, 8])
def test_iir_gather_is_bit_exact_against_python_indexing_and_prepares_the_observations(N, L, end, order):
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.bwe_iir_long import iir_gather, iir_plan, window_state
    from audio_inpainting_diffusion_amd.restore import job_table
    R = 3
    table = _table(order)
    A, B = iir_plan(R, N, L, end, order)
    _, rec = _strided(R, N, 1 + N, 0)
    _, out = _strided(R, N, 2 + N, 1)                                            # (out != rec; its rows start at an odd element)
    rec_d = torch.empty(R, N + 3, device=DEV)[:, :N].copy_(rec)
    out_d = torch.empty(R, N + 3, device=DEV)[:, 1:N + 1].copy_(out)
    i = torch.arange(L)
    for jobs in (A, B, A + B):
        if not jobs:
            continue
        tab = job_table(jobs, DEV)
        J = len(jobs)
        raw, k = torch.empty(J, L, device=DEV), torch.empty(J, L, device=DEV)
        _lib.call("aid_iir_gather", _lib.BweGatherParams(rec_d.data_ptr(), out_d.data_ptr(), raw.data_ptr(), k.data_ptr(), tab.data_ptr(), J, R, order + 1, L, N, N + 3, N + 3))
        k_ref, raw_ref = [], []
        for r, s, head, tail, lo, hi in jobs:
            kr = torch.from_numpy(window_state(N, L, order, s, head, tail))
            qc = (s + i).clamp(max=N - 1)
            k_ref.append(kr)
            raw_ref.append(torch.where(kr == 1, out[r, qc], torch.where((kr == 0) | (kr == -3), rec[r, qc], torch.zeros(L))))
        k_ref, raw_ref = torch.stack(k_ref), torch.stack(raw_ref)
        assert torch.equal(k.cpu(), k_ref) and torch.equal(raw.cpu(), raw_ref)
        yp, k2 = iir_gather(rec_d, out_d, tab, L, table)
        want = iir_observed_torch(raw_ref.double(), table.b, table.a, k_ref.double(), "prepare")
        assert torch.equal(k2.cpu(), k_ref) and rel_l2(yp.cpu(), want) <= 1e-6
        assert torch.equal(yp.cpu()[k_ref == 1], raw_ref[k_ref == 1]) and bool((yp.cpu()[k_ref < 0] == 0).all())
    tab = job_table(A, DEV)
    y0 = torch.zeros(len(A), L, device=DEV)
    for bad in (dict(rec_ld=N - 1), dict(out_ld=N - 1), dict(J=0), dict(J=65536), dict(K=1), dict(K=18)):
        kw = dict(J=len(A), K=order + 1, rec_ld=N + 3, out_ld=N + 3)
        kw.update(bad)
        with pytest.raises(_lib.AidError):
            _lib.call("aid_iir_gather", _lib.BweGatherParams(rec_d.data_ptr(), out_d.data_ptr(), y0.data_ptr(), y0.data_ptr(), tab.data_ptr(),
                                                             kw["J"], R, kw["K"], L, N, kw["rec_ld"], kw["out_ld"]))
    assert bool((y0 == 0).all())


def test_an_invalid_job_row_of_the_iir_gather_touches_nothing_outside_its_own_output():
    """The table is device memory: a row with a recording outside [0, R), a negative or too large start gathers zeros, all absent; head / tail
    beyond L are clamped.  The outputs lie inside guarded buffers: nothing before, between or after the rows is written."""
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.restore import job_table
    R, N, L, o = 2, 300, 128, 8
    rec = torch.randn(R, N, generator=torch.Generator().manual_seed(1)).to(DEV)
    out = torch.randn(R, N, generator=torch.Generator().manual_seed(2)).to(DEV)
    jobs = [(R, 0, 0, 0, 0, L), (-1, 0, 0, 0, 0, L), (0, -4, 0, 0, 0, L), (0, N, 0, 0, 0, L), (1, 200, 0, 0, -5, 10 * L), (1, 0, 10 * L, 0, 0, L), (0, 7, 3, 10 * L, 0, L),
            (1 << 40, 1 << 40, 5, 5, 0, L), (0, 7, 0, 0, 0, L), (1, N - 3, 0, 0, 0, L)]
    J = len(jobs)
    tab = job_table(jobs, DEV)
    pad = 64
    bufs = [torch.full((pad + J * L + pad,), SENT, device=DEV) for _ in range(2)]
    y, k = (b[pad:-pad] for b in bufs)
    _lib.call("aid_iir_gather", _lib.BweGatherParams(rec.data_ptr(), out.data_ptr(), y.data_ptr(), k.data_ptr(), tab.data_ptr(), J, R, o + 1, L, N, N, N))
    assert all(bool((b[:pad] == SENT).all()) and bool((b[-pad:] == SENT).all()) for b in bufs)
    y, k = y.reshape(J, L), k.reshape(J, L)
    for j in (0, 1, 2, 3, 7):
        assert bool((y[j] == 0).all()) and bool((k[j] == -2).all()), j
    # s = 200: the first o samples seed, 100 samples exist, the rest absent
    assert bool((k[4, :o] == -3).all()) and bool((k[4, o:100] == 0).all()) and torch.equal(y[4, :100], rec[1, 200:]) and bool((y[4, 100:] == 0).all()) and bool((k[4, 100:] == -2).all())
    assert torch.equal(y[5], out[1, :L]) and bool((k[5] == 1).all())             # s = 0, head clamped to L: the whole window known from out
    assert bool((k[6, :o] == -3).all()) and torch.equal(y[6, :o], rec[0, 7:7 + o]) and torch.equal(y[6, o:], out[0, 7 + o:7 + L]) and bool((k[6, o:] == 1).all())   # seeds before known
    assert bool((k[8, :o] == -3).all()) and bool((k[8, o:] == 0).all()) and torch.equal(y[8], rec[0, 7:7 + L])
    assert bool((k[9, :3] == -3).all()) and bool((k[9, 3:] == -2).all()) and torch.equal(y[9, :3], rec[1, N - 3:])      # the recording ends inside the seeds


# ---- the property on the device ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(iir_filters()))
def test_every_window_of_both_passes_reproduces_the_recording_on_the_device(name):
    """The true float32 signal and rec = float32(lfilter64(x)): in every window of both passes |apply(x_w) - y'| at the state-0 samples stays
    within (seed_error_bound + 2^-23) max|rec| -- the seed rounding, plus the float32 rounding of the recording and of the operator's output."""
    from audio_inpainting_diffusion_amd.bwe_iir_long import IIRObserved, IIRTable, iir_gather, iir_plan
    from audio_inpainting_diffusion_amd.restore import job_table, window_gather
    table = IIRTable(*iir_filters()[name])
    R, N, L, end = 2, N_HOST, L_HOST, END_HOST
    x = (torch.randn(R, N, generator=torch.Generator().manual_seed(3)) * 0.1)
    rec = torch.from_numpy(scipy.signal.lfilter(table.b, table.a, x.double().numpy(), axis=-1)).float()
    top = float(rec.abs().max())
    xd, rec_d = x.to(DEV), rec.to(DEV)
    worst = 0.0
    for jobs in iir_plan(R, N, L, end, table.order):
        tab = job_table(jobs, DEV)
        yp, k = iir_gather(rec_d, xd, tab, L, table)                              # (the result so far is the truth)
        xw, _ = window_gather(xd, xd, torch.ones(1, N, device=DEV), tab, L)        # the true windows (zeros beyond the end)
        dev = (IIRObserved(table, k).apply(xw) - yp).abs()[k == 0]
        assert dev.numel() and bool((k == 0).any(dim=1).all())
        worst = max(worst, float(dev.max()))
    print(f"{name}: worst |apply(x_w) - y'| = {worst / top:.2e} max|rec| (bound {table.seed_error_bound + 2.0 ** -23:.2e})")
    assert worst <= (table.seed_error_bound + 2.0 ** -23) * top


# ---- the two passes around a stub sampler ------------------------------------------------------------------------------------------------
class _Stub:
    """predict_resample(y, shape, op)[j, i] = w_j * L + i + r_j / 4, with (r_j, w_j) read from the job's seed (r_j + 1) * 65536 + w_j: every sample
    names the window it was written from."""

    def __init__(self):
        self.calls, self.seeds = [], "untouched"

    def predict_resample(self, y, shape, op):
        assert tuple(shape) == tuple(y.shape) and op.state.shape == y.shape and op.L == y.shape[1]
        self.calls.append((y.clone(), op.state.clone(), op.table, self.seeds))
        L = y.shape[1]
        base = torch.tensor([(s % 65536) * L + (s // 65536 - 1) / 4 for s in self.seeds], dtype=torch.float32, device=y.device)
        return base[:, None] + torch.arange(L, dtype=torch.float32, device=y.device)[None, :]


@pytest.mark.parametrize("N,L,end", GATHER_CASES)
@pytest.mark.parametrize("max_batch", [1, 3, 8])
def test_two_passes_stitch_the_stub_sampler_output(N, L, end, max_batch):
    from audio_inpainting_diffusion_amd.bwe_iir_long import bwe_iir_passes, iir_plan, window_state
    R, step, order = 3, L - end, 8
    _, rec = _strided(R, N, 11 + N, 1)
    rec_d = torch.empty(R, N + 3, device=DEV)[:, 1:N + 1].copy_(rec)
    filt = _filter(order)
    A, B = iir_plan(R, N, L, end, order)
    assert A and (B or N <= L)
    stub, seeds = _Stub(), [1, 2, 3]
    out = bwe_iir_passes(stub, rec_d, filt, "cheby1", L, end, max_batch=max_batch, seeds=seeds)
    assert out.is_cuda and out.shape == (R, N) and stub.seeds == "untouched"
    # every sample of [0, N) comes from the window that owns it, and from no other
    want = torch.full((R, N), float("nan"))
    for r, s, head, tail, lo, hi in A + B:
        assert bool(torch.isnan(want[r, s + lo:s + hi]).all())
        want[r, s + lo:s + hi] = (s // step) * L + torch.arange(lo, hi) + r / 4
    assert torch.equal(out.cpu(), want)
    nA, nB = math.ceil(len(A) / max_batch), math.ceil(len(B) / max_batch)
    assert len(stub.calls) == nA + nB and all(call[0].shape[0] <= max_batch and call[0].shape == call[1].shape for call in stub.calls)
    assert sum(call[0].shape[0] for call in stub.calls[:nA]) == len(A) and sum(call[0].shape[0] for call in stub.calls) == len(A) + len(B)
    assert [s for call in stub.calls for s in call[3]] == [seeds[r] * 65536 + s // step for r, s, *_ in A + B]      # each job once, with its seed
    assert all(call[2] is stub.calls[0][2] for call in stub.calls)                                                 # one coefficient table
    # pass A sees the recording and nothing known; pass B sees what pass A left at its heads and tails, bit for bit, as known
    ys, ks = torch.cat([call[0] for call in stub.calls]).cpu(), torch.cat([call[1] for call in stub.calls]).cpu()
    for j, (r, s, head, tail, lo, hi) in enumerate(A + B):
        k_ref = torch.from_numpy(window_state(N, L, order, s, head, tail))
        assert torch.equal(ks[j], k_ref) and bool((ys[j][k_ref < 0] == 0).all())
        if j < len(A):
            assert not bool((k_ref == 1).any())
        else:
            assert head == end - order and bool((k_ref[:order] == -3).all()) and bool((k_ref[order:head] == 1).all())
            assert torch.equal(ys[j, order:head], want[r, s + order:s + head])
            if tail:
                assert torch.equal(ys[j, L - tail:], want[r, s + L - tail:s + L]) and bool((k_ref[L - tail:] == 1).all())
            assert bool((want[r, s:s + head] < (s // step) * L).all())             # ... and those samples belong to the even neighbours

    class _Plain(_Stub):
        def predict_resample(self, y, shape, op):
            self.calls.append(self.seeds)
            return y + 1
    plain = _Plain()
    bwe_iir_passes(plain, rec_d, filt, "cheby1", L, end, max_batch=max_batch)
    assert len(plain.calls) == nA + nB and all(s is None for s in plain.calls) and plain.seeds == "untouched"


# ---- reduced HIP network -----------------------------------------------------------------------------------------------------------------
def _rec(table, N, R, seed0):
    """(clean [R, N], rec = float32(lfilter64(clean))) on the host"""
    clean = torch.stack([torch.randn(N, generator=torch.Generator().manual_seed(seed0 + r)) for r in range(R)]) * 0.063
    return clean, torch.from_numpy(scipy.signal.lfilter(table.b, table.a, clean.double().numpy(), axis=-1)).float()


def test_one_window_equals_predict_bwe_and_the_unclamped_biquad():
    """R = 1, N = L: one job, all samples in state 0, S = 0 -- predict_bwe "cheby1" within 5e-6; "biquad" against predict_conditional through
    IIRFilter.biquad(clamp=False), the LINEAR filter (the departure from predict_bwe "biquad", whose operator clamps); a "biquad" recording
    that touches +-1 is refused."""
    from test_gpu_bwe_long import _small_net
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.bwe_iir_long import IIRTable
    from audio_inpainting_diffusion_amd.degrade import IIRFilter
    smp, _, Ls = _small_net()
    seed = 23
    filt = _filter(4)
    _, y = _rec(IIRTable(filt, "cheby1"), Ls, 1, 4)
    yd = y.to(DEV)
    smp.seeds = [99]
    out = smp.predict_bwe_iir_long(yd, filt, "cheby1", seeds=[seed])
    assert smp.seeds == [99] and out.is_cuda and out.shape == (1, Ls)
    smp.seeds = [seed * 65536]
    ref = smp.predict_bwe(yd, filt, "cheby1")
    e = rel_l2(out.cpu(), ref.cpu())
    print(f"one window vs predict_bwe cheby1: rel-L2 = {e:.2e}")
    assert e <= 5e-6 and not torch.equal(out, yd)
    biq = iir_filters()["biquad"][0]
    _, y = _rec(IIRTable(biq, "biquad"), Ls, 1, 5)
    yd = y.to(DEV)
    out = smp.predict_bwe_iir_long(yd, biq, "biquad", seeds=[seed])
    smp.seeds = [seed * 65536]
    ref = smp.predict_conditional(yd, IIRFilter.biquad(*biq, audio_len=Ls, clamp=False, device=DEV))
    e = rel_l2(out.cpu(), ref.cpu())
    print(f"one window vs predict_conditional through the unclamped biquad: rel-L2 = {e:.2e}")
    assert e <= 5e-6
    n0 = smp.n_evals
    for v in (1.0, -1.0, 1.5):
        bad = yd.clone()
        bad[0, Ls // 2] = v
        with pytest.raises(_lib.AidError, match="clamp"):
            smp.predict_bwe_iir_long(bad, biq, "biquad", seeds=[seed])
    assert smp.n_evals == n0
    smp.predict_bwe_iir_long(bad, filt, "cheby1", seeds=[seed])                  # (lfilter with clamp=False: no such refusal)


def test_hip_network_pass_a_and_pass_b_shaped_windows_vs_oracle():
    """Item 0 is shaped as a window of pass A behind the start of the recording: ``order`` seeds, the last 37 samples absent.  Item 1 as one of
    pass B: seeds, then the head known up to end - order, the tail known.  Order 8, T = 3, guidance only -- predict_resample with IIRObserved
    against the oracle sampler driven with the float64 torch model of the operator.  Bound: the 5e-4 of the FIR test, same network."""
    from test_gpu_bwe_long import _small_net
    from audio_inpainting_diffusion_amd.bwe_iir_long import IIRObserved
    from audio_inpainting_diffusion_amd.sampler import autoregressive_overlap
    smp, osmp, Ls = _small_net()
    order, s0 = 8, 300
    table = _table(order)
    end = int(autoregressive_overlap(smp.args) * Ls)
    clean, rec = _rec(table, s0 + Ls, 2, 40)
    clean, rec = clean[:, s0:], rec[:, s0:]
    k = torch.zeros(2, Ls)
    k[:, :order] = -3
    k[0, Ls - 37:] = -2
    k[1, order:end - order] = 1
    k[1, Ls - (end - order):] = 1
    raw = torch.where((k == -3) | (k == 0), rec, torch.where(k == 1, clean, torch.zeros_like(rec)))
    y = iir_observed_torch(raw.double(), table.b, table.a, k.double(), "prepare").float()
    deg = lambda x: iir_observed_torch(x.double(), table.b, table.a, k.double()).to(x.dtype)                        # noqa: E731
    smp.seeds = [7, 8]
    out = smp.predict_resample(y.to(DEV), (2, Ls), IIRObserved(table, k.to(DEV)))
    ref = osmp.predict_resample(y, (2, Ls), deg, seeds=[7, 8])
    e = rel_l2(out.cpu(), ref)
    print(f"HIP network, IIRObserved windows: rel-L2 vs oracle = {e:.2e}")
    assert e <= 5e-4


def _long_case(smp, Ls, order=8):
    from audio_inpainting_diffusion_amd.bwe_iir_long import iir_plan
    from audio_inpainting_diffusion_amd.sampler import autoregressive_overlap
    end = int(autoregressive_overlap(smp.args) * Ls)
    N = 2 * Ls + Ls // 3
    _, rec = _rec(_table(order), N, 2, 70)
    A, B = iir_plan(2, N, Ls, end, order)
    assert len(A) == 4 and len(B) == 2
    return N, rec, _filter(order)


def test_hip_network_result_is_independent_of_the_other_recordings_and_of_max_batch():
    """Two recordings of three windows each, order 8, T = 3: restored together, each alone, and with max_batch 1 against 8 (<= 5e-6, the
    documented bound for results across batch compositions)."""
    from test_gpu_bwe_long import _small_net
    smp, _, Ls = _small_net()
    N, rec, filt = _long_case(smp, Ls)
    rec_d, seeds = rec.to(DEV), [31, 32]
    n0 = smp.n_evals
    both = smp.predict_bwe_iir_long(rec_d, filt, "cheby1", max_batch=8, seeds=seeds)
    assert smp.n_evals - n0 == 6 * (2 * 3 - 1) and both.shape == (2, N) and bool(torch.isfinite(both).all()) and not torch.equal(both, rec_d)
    errs = {}
    for r in range(2):
        alone = smp.predict_bwe_iir_long(rec_d[r:r + 1], filt, "cheby1", max_batch=8, seeds=seeds[r:r + 1])
        errs[f"recording {r} alone"] = rel_l2(alone.cpu(), both[r:r + 1].cpu())
    one = smp.predict_bwe_iir_long(rec_d, filt, "cheby1", max_batch=1, seeds=seeds)
    for r in range(2):
        errs[f"recording {r} max_batch 1"] = rel_l2(one[r:r + 1].cpu(), both[r:r + 1].cpu())
    print("bwe_iir_long batch invariance, rel-L2:", {k: "%.2e" % v for k, v in errs.items()})
    assert all(e <= 5e-6 for e in errs.values()), errs


@functools.lru_cache(maxsize=None)
def _dc_off_result():
    from test_gpu_generic import _sampler
    L = 4096
    smp = _sampler(L, 3, 0.25, **{"data_consistency.use": False})
    _, y = _rec(_table(4), 2 * L + L // 3, 2, 50)
    return y, smp.predict_bwe_iir_long(y.to(DEV), _filter(4), "cheby1", seeds=[3, 4]).cpu()


@pytest.mark.parametrize("dc_type", ["end", "always"])
def test_data_consistency_end_and_always_run_and_change_the_result(dc_type):
    """Two recordings of three windows, toy denoiser: the projection of IIRObserved (once on the final state / at every evaluation) runs, costs no
    evaluation, and changes the result."""
    from test_gpu_generic import _sampler
    y, off = _dc_off_result()
    smp = _sampler(4096, 3, 0.25, **{"data_consistency.use": True, "data_consistency.type": dc_type})
    n0 = smp.n_evals
    out = smp.predict_bwe_iir_long(y.to(DEV), _filter(4), "cheby1", seeds=[3, 4]).cpu()
    assert smp.n_evals - n0 == 6 * (2 * 3 - 1) and out.shape == y.shape and bool(torch.isfinite(out).all())
    assert bool(torch.isfinite(off).all()) and not torch.equal(out, off)


# ---- pooled and sharded --------------------------------------------------------------------------------------------------------------------
def test_pooled_over_two_lengths_equals_the_plain_calls_bit_for_bit():
    from test_gpu_bwe_long import _small_net
    from audio_inpainting_diffusion_amd import harness
    smp, _, Ls = _small_net()
    order = 8
    table, filt = _table(order), _filter(order)
    _, long_ = _rec(table, 2 * Ls + Ls // 3, 1, 80)
    _, short = _rec(table, Ls + Ls // 2, 2, 90)
    groups = [long_.to(DEV), short.to(DEV)]
    pooled = smp.predict_long_pooled("bwe_iir", groups, max_batch=3, seeds=[51, 52, 53], filt=filt, filt_type="cheby1")
    plain = [smp.predict_bwe_iir_long(groups[0], filt, "cheby1", max_batch=3, seeds=[51]), smp.predict_bwe_iir_long(groups[1], filt, "cheby1", max_batch=3, seeds=[52, 53])]
    assert all(torch.equal(p, q) for p, q in zip(pooled, plain)) and not torch.equal(pooled[0], groups[0])
    files = [long_[0], short[0], short[1]]
    a = harness.bwe_iir_long(smp, files, filt, "cheby1", seeds=[51, 52, 53], max_batch=3, device=DEV, pool=True)
    b = harness.bwe_iir_long(smp, files, filt, "cheby1", seeds=[51, 52, 53], max_batch=3, device=DEV, pool=False)
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and torch.equal(a[0], pooled[0][0]) and torch.equal(a[2], pooled[1][1])


WORLD, DIST_SEEDS = 3, [31, 32]


def _dist_call(smp, Ls, dev):
    N, rec, filt = _long_case(smp, Ls)
    return smp.predict_bwe_iir_long(rec.to(dev), filt, "cheby1", max_batch=8, seeds=DIST_SEEDS).cpu().numpy()


def _worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                          AID_DIST_BACKEND="gloo")
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from audio_inpainting_diffusion_amd import dist as D
        from test_gpu_long_dist import _samplers
        D.init_distributed()
        torch.cuda.set_device(0)
        net, _, smp, Ls = _samplers("cuda:0", seed_offset=rank)                    # ranks start with DIFFERENT weights: the broadcast must fix that
        D.broadcast_parameters(net, src=0)
        res = _dist_call(smp, Ls, "cuda:0")
        D.barrier()
        q.put((rank, res))
        torch.distributed.destroy_process_group()
    except BaseException:
        q.put((rank, traceback.format_exc()))
        raise


def test_three_ranks_on_one_gpu_return_the_single_process_result_on_every_rank():
    """Three ranks share the device (gloo, the pattern of tests/test_gpu_long_dist.py): every rank holds the single process's result, bit for bit."""
    from test_gpu_long_dist import _free_port, _samplers
    _, _, smp, Ls = _samplers("cuda")
    want = _dist_call(smp, Ls, "cuda")
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_worker, args=(r, WORLD, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    got = []
    try:
        for _ in range(WORLD):
            got.append(q.get(timeout=600))
            assert isinstance(got[-1][1], np.ndarray), got[-1][1]
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
    except queue.Empty:
        pytest.fail("a worker did not answer within 600 s")
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join(timeout=10)
    assert np.isfinite(want).all() and len(got) == WORLD
    for rank, res in sorted(got, key=lambda t: t[0]):
        assert np.array_equal(res, want), rank
