"""GPU tests of declipping whole recordings (csrc/aid_declip.hip, declip_long.py, Sampler.predict_declipping_long): the operator of
clipped / known / absent samples and the gather bit-exact against torch expressions, the two passes stitched around a stub sampler,
one window against predict_declipping, the data-consistency projection, and the reduced HIP network against the oracle and across
batch compositions.  Toy and reduced-size models only."""
import ast
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2
from test_restore_long_host import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.5
ATOL_OBSERVED = 16 * 2.0 ** -24          # a handful of float32 roundings of values of the recording's size, relative to its largest sample
LEVELS = (0.25, 0.05, 1.0)
UP = 1 + 2.0 ** -23                      # the float32 after 1: c * UP is the first value above a level c


# ---- the operator ------------------------------------------------------------------------------------------------------------------------
def _on_device(t, shift):
    """host [B, L] -> (buffer [B, L + 3] filled with SENT, its view [:, shift:shift + L] holding t): rows strided and, in general, misaligned"""
    B, L = t.shape
    buf = torch.full((B, L + 3), SENT, device=DEV)
    view = buf[:, shift:shift + L]
    view.copy_(t)
    return buf, view


def _edge_values(t, c):
    """samples exactly at +-c and one float32 beyond, at positions 0..3 and at the last 3 (c: [B, 1] float32)"""
    B, L = t.shape
    first = torch.cat([c, -c, c * UP, -c * UP], dim=1)
    t[:, :4] = first[:, :min(4, L)]
    t[:, L - 3:] = torch.cat([-c * UP, c, -c], dim=1)
    return t


def _signals(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.tensor(LEVELS[:B], dtype=torch.float32)[:, None]
    x, xref, y = (_edge_values(torch.randn(B, L, generator=g) * c * 1.2, c) for _ in range(3))
    y = torch.maximum(torch.minimum(y, c * UP), -c * UP)
    if L > 8:
        y[:, 4] = c[:, 0] * (1 - 2.0 ** -24)                             # the last value below the level: not clipped
    gy = torch.randn(B, L, generator=g)
    state = torch.randint(-1, 2, (B, L), generator=g).float()
    if L >= 16:
        state[:, 2:14] = torch.tensor([1.0, 0.0, -1.0, 0.0, 1.0, -1.0] * 2)   # all three next to each other across every float4 boundary in 2..14
    return c, x, xref, y, gy, state


def _references(c, x, xref, y, gy, state):
    """modes 0, 1, 2 as torch expressions on the host, and autograd's gradient of mode 0 at xref"""
    k = state.expand_as(x)
    zero = torch.zeros_like(x)
    clamp = lambda v: torch.stack([torch.clamp(v[b], min=-float(c[b]), max=float(c[b])) for b in range(v.shape[0])])
    apply = lambda v: torch.where(k == 1, v, torch.where(k == 0, clamp(v), zero))
    inside = (xref >= -c) & (xref <= c)
    adj = torch.where(k == 1, gy, torch.where(k == 0, gy * inside, zero))
    xr = xref.clone().requires_grad_()
    (auto,) = torch.autograd.grad(apply(xr), xr, gy)
    proj = torch.where(k == 1, y, torch.where(k == -1, x, torch.where(y.abs() < c, y, torch.where(y >= c, torch.maximum(x, c), torch.minimum(x, -c)))))
    return apply(x), adj, auto, proj


@pytest.mark.parametrize("B,L", [(1, 1000), (3, 4097), (2, 5)])
@pytest.mark.parametrize("shared", [False, True])
def test_clip_known_modes_are_exact_on_strided_misaligned_rows(B, L, shared):
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.declip_long import ClipObserved
    c, x, xref, y, gy, state = _signals(B, L, 7 + L + B)
    if shared:
        state = state[:1]
    want0, want1, auto, want2 = _references(c, x, xref, y, gy, state)
    assert torch.equal(want1, auto)
    clip_d = c.reshape(-1).to(DEV)
    (_, xd), (_, rd), (_, yd), (_, gd), (_, kd) = _on_device(x, 1), _on_device(xref, 2), _on_device(y, 3), _on_device(gy, 0), _on_device(state, 2)
    obs = state.expand(B, L) == 0
    low, high = obs & (y.abs() < c), obs & (y.abs() >= c)
    assert L < 16 or (bool(low.any()) and bool(high.any()))
    for out_shift in (0, 1, 3):
        for mode, src, want in ((0, xd, want0), (1, gd, want1), (2, xd, want2)):
            obuf, od = _on_device(torch.full((B, L), SENT), out_shift)
            guard = torch.full((2, B, L + 3), SENT, device=DEV)
            _lib.call("aid_clip_known", _lib.ClipKnownParams(src.data_ptr(), rd.data_ptr() if mode == 1 else None, yd.data_ptr() if mode == 2 else None,
                                                             kd.data_ptr(), clip_d.data_ptr(), od.data_ptr(), B, mode, L, L + 3, L + 3, L + 3,
                                                             0 if shared else L + 3, L + 3))
            got = od.cpu()
            assert torch.equal(got, want), (out_shift, mode)
            if mode == 2:   # the device's projection: unclipped samples are the observation bit for bit, clipped ones lie at or beyond the level on its side
                assert torch.equal(got[low], y[low]) and bool(((got * torch.sign(y))[high] >= c.expand(B, L)[high]).all())
            pad = torch.ones(B, L + 3, dtype=torch.bool)
            pad[:, out_shift:out_shift + L] = False
            assert bool((obuf.cpu()[pad] == SENT).all()) and bool((guard == SENT).all())       # nothing outside the rows of out
    # the operator object (contiguous signals; the state keeps its row stride)
    op = ClipObserved(kd, clip_d)
    assert op.shared_mask is False and (op.B, op.L) == (B, L)
    assert torch.equal(op.apply(rd).cpu(), _references(c, xref, xref, y, gy, state)[0]) and torch.equal(op(xd).cpu(), want0)
    with pytest.raises(_lib.AidError, match="matching apply"):
        ClipObserved(kd, clip_d).adjoint(gd)
    op.apply(rd)
    assert torch.equal(op.adjoint(gd).cpu(), want1)
    assert torch.equal(op.project(xd, yd).cpu(), want2)
    # refusals of the launcher: checked on the host, nothing is launched
    o = torch.zeros(B, L, device=DEV)
    for bad in (dict(mode=3), dict(mode=-1), dict(B=0), dict(x_ld=L - 1), dict(out_ld=L - 1), dict(state_ld=L - 1), dict(mode=1, xref=None), dict(mode=2, y=None)):
        kw = dict(mode=0, B=B, x_ld=L + 3, out_ld=L, state_ld=0 if shared else L + 3, xref=rd.data_ptr(), y=yd.data_ptr())
        kw.update(bad)
        with pytest.raises(_lib.AidError):
            _lib.call("aid_clip_known", _lib.ClipKnownParams(xd.data_ptr(), kw["xref"], kw["y"], kd.data_ptr(), clip_d.data_ptr(), o.data_ptr(), kw["B"], kw["mode"],
                                                             L, kw["x_ld"], L + 3, L + 3, kw["state_ld"], kw["out_ld"]))
    assert bool((o == 0).all())


def test_clip_known_apply_and_adjoint_on_two_concurrent_streams():
    """One operator of two items, used by two streams at once: the x_hat of an apply is kept per stream (the pattern of the HardClip test)."""
    from audio_inpainting_diffusion_amd.declip_long import ClipObserved
    L = 3000
    g = torch.Generator().manual_seed(9)
    x = torch.randn(4, L, generator=g) * 0.3
    gy = torch.randn(4, L, generator=g)
    state = torch.randint(-1, 2, (1, L), generator=g).float().to(DEV)
    op = ClipObserved(state, [0.25, 0.05])
    xd, gd = x.to(DEV), gy.to(DEV)
    seq = [op.adjoint(gd[:2]) if op.apply(xd[:2]) is not None else None, op.adjoint(gd[2:]) if op.apply(xd[2:]) is not None else None]
    assert not torch.equal(seq[0], seq[1])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [None, None]
    cur = torch.cuda.current_stream()
    for s in streams:
        s.wait_stream(cur)
    with torch.cuda.stream(streams[0]):
        op.apply(xd[:2])
    with torch.cuda.stream(streams[1]):
        op.apply(xd[2:])
    with torch.cuda.stream(streams[0]):
        outs[0] = op.adjoint(gd[:2])
    with torch.cuda.stream(streams[1]):
        outs[1] = op.adjoint(gd[2:])
    for s in streams:
        cur.wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], seq[0]) and torch.equal(outs[1], seq[1])


@pytest.mark.parametrize("shared", [False, True])
def test_rows_is_the_operator_of_the_sliced_inputs(shared):
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.declip_long import ClipObserved
    B, L = 3, 4097
    c, x, xref, y, gy, state = _signals(B, L, 21)
    state = (state[:1] if shared else state).to(DEV)
    xd, rd, yd, gd, cd = x.to(DEV), xref.to(DEV), y.to(DEV), gy.to(DEV), c.reshape(-1).to(DEV)
    sub = ClipObserved(state, cd).rows(1, 3)
    ref = ClipObserved(state if shared else state[1:3].contiguous(), cd[1:3].clone())
    assert (sub.B, sub.L, sub.shared_mask) == (2, L, False) and sub.state.shape[0] == (1 if shared else 2)
    assert not shared or sub.state.data_ptr() == state.data_ptr()                          # a shared state row stays shared
    assert torch.equal(sub.apply(rd[1:3]), ref.apply(rd[1:3])) and torch.equal(sub.adjoint(gd[1:3]), ref.adjoint(gd[1:3]))
    assert torch.equal(sub.project(xd[1:3], yd[1:3]), ref.project(xd[1:3], yd[1:3]))
    assert not torch.equal(sub.apply(rd[1:3]), ClipObserved(state, cd).rows(0, 2).apply(rd[1:3]))     # (the levels differ)
    for lo, hi in ((2, 2), (-1, 2), (1, 4)):
        with pytest.raises(_lib.AidError):
            ClipObserved(state, cd).rows(lo, hi)


# ---- the gather --------------------------------------------------------------------------------------------------------------------------
def _all_windows(N, L, end, R):
    from audio_inpainting_diffusion_amd.restore import restore_plan
    return restore_plan(torch.zeros(1, N), L, end, R=R)[:2]


def _strided(R, N, seed, shift):
    """[R, N] view with row stride N + 3 starting ``shift`` elements into its buffer -> (buffer, view), on the host"""
    base = torch.randn(R, N + 3, generator=torch.Generator().manual_seed(seed))
    return base, base[:, shift:shift + N]


@pytest.mark.parametrize("N,L,end", CASES)
def test_declip_gather_is_bit_exact_against_python_indexing(N, L, end):
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.declip_long import declip_gather
    from audio_inpainting_diffusion_amd.restore import job_table
    R = 3
    A, B = _all_windows(N, L, end, R)
    _, rec = _strided(R, N, 1 + N, 0)
    _, out = _strided(R, N, 2 + N, 1)                                            # (out != rec; its rows start at an odd element)
    rec_d = torch.empty(R, N + 3, device=DEV)[:, :N].copy_(rec)
    out_d = torch.empty(R, N + 3, device=DEV)[:, 1:N + 1].copy_(out)
    clip_d = torch.tensor(LEVELS, device=DEV)
    i = torch.arange(L)
    for jobs in (A, B, A + B):
        if not jobs:
            continue
        y, k, c = declip_gather(rec_d, out_d, clip_d, job_table(jobs, DEV), L)
        assert y.shape == k.shape == (len(jobs), L) and c.shape == (len(jobs),)
        assert c.cpu().tolist() == [float(np.float32(LEVELS[r])) for r, *_ in jobs]
        for j, (r, s, head, tail, lo, hi) in enumerate(jobs):
            inside, qc = (s + i) < N, (s + i).clamp(max=N - 1)
            edge = (i < head) | (i >= L - tail)
            k_ref = torch.where(inside, edge.float(), torch.full((L,), -1.0))
            y_ref = torch.where(inside, torch.where(edge, out[r, qc], rec[r, qc]), torch.zeros(L))
            assert torch.equal(k[j].cpu(), k_ref) and torch.equal(y[j].cpu(), y_ref), j
    tab = job_table(A, DEV)
    y0 = torch.zeros(len(A), L, device=DEV)
    for bad in (dict(rec_ld=N - 1), dict(out_ld=N - 1), dict(J=0), dict(J=65536)):
        kw = dict(J=len(A), rec_ld=N + 3, out_ld=N + 3)
        kw.update(bad)
        with pytest.raises(_lib.AidError):
            _lib.call("aid_declip_gather", _lib.DeclipGatherParams(rec_d.data_ptr(), out_d.data_ptr(), clip_d.data_ptr(), y0.data_ptr(), y0.data_ptr(), y0.data_ptr(),
                                                                   tab.data_ptr(), kw["J"], R, L, N, kw["rec_ld"], kw["out_ld"]))
    assert bool((y0 == 0).all())


def test_an_invalid_job_row_of_the_declip_gather_touches_nothing_outside_its_own_output():
    """The table is device memory: a row with a recording outside [0, R), a negative or too large start gathers zeros, all absent, level 0;
    head / tail beyond L are clamped.  The outputs lie inside guarded buffers: nothing before, between or after the rows is written."""
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.restore import job_table
    R, N, L = 2, 300, 128
    rec = torch.randn(R, N, generator=torch.Generator().manual_seed(1)).to(DEV)
    out = torch.randn(R, N, generator=torch.Generator().manual_seed(2)).to(DEV)
    clip = torch.tensor([0.25, 0.05], device=DEV)
    jobs = [(R, 0, 0, 0, 0, L), (-1, 0, 0, 0, 0, L), (0, -4, 0, 0, 0, L), (0, N, 0, 0, 0, L), (1, 200, 0, 0, -5, 10 * L), (1, 0, 10 * L, 0, 0, L), (0, 7, 3, 10 * L, 0, L)]
    J = len(jobs)
    tab = job_table(jobs, DEV)
    pad = 64
    bufs = [torch.full((pad + n + pad,), SENT, device=DEV) for n in (J * L, J * L, J)]
    y, k, c = (b[pad:-pad] for b in bufs)
    _lib.call("aid_declip_gather", _lib.DeclipGatherParams(rec.data_ptr(), out.data_ptr(), clip.data_ptr(), y.data_ptr(), k.data_ptr(), c.data_ptr(), tab.data_ptr(),
                                                           J, R, L, N, N, N))
    assert all(bool((b[:pad] == SENT).all()) and bool((b[-pad:] == SENT).all()) for b in bufs)
    y, k = y.reshape(J, L), k.reshape(J, L)
    assert bool((y[:4] == 0).all()) and bool((k[:4] == -1).all()) and c[:4].cpu().tolist() == [0.0] * 4
    assert torch.equal(y[4, :100], rec[1, 200:]) and bool((k[4, :100] == 0).all()) and bool((y[4, 100:] == 0).all()) and bool((k[4, 100:] == -1).all())
    assert torch.equal(y[5], out[1, :L]) and bool((k[5] == 1).all())             # head clamped to L: the whole window known from out
    assert torch.equal(y[6], out[0, 7:7 + L]) and bool((k[6] == 1).all())         # tail clamped to L
    assert c[4:].cpu().tolist() == [float(np.float32(0.05)), float(np.float32(0.05)), 0.25]


# ---- the two passes around a stub sampler ------------------------------------------------------------------------------------------------
class _Stub:
    """predict_resample(y, shape, op) = y + 7 * (state == 0) * (|y| >= c): known and unclipped samples pass through, every clipped one moves by 7"""

    def __init__(self):
        self.calls, self.seeds = [], "untouched"

    def predict_resample(self, y, shape, op):
        assert tuple(shape) == tuple(y.shape) and (op.B, op.L) == tuple(y.shape)
        self.calls.append((y.clone(), op.state.clone(), op.clip.clone(), self.seeds))
        return y + 7 * (op.state == 0) * (y.abs() >= op.clip[:, None])


def _clipped_recordings(R, N, seed):
    c = torch.tensor(LEVELS[:R])[:, None]
    buf, rec = _strided(R, N, seed, 1)
    rec.copy_(torch.maximum(torch.minimum(rec * c * 0.6, c), -c))                # about one sample in ten is clipped, in every window
    return c, rec


@pytest.mark.parametrize("N,L,end", CASES)
@pytest.mark.parametrize("max_batch", [2, 8])
def test_two_passes_stitch_the_stub_sampler_output(N, L, end, max_batch):
    from audio_inpainting_diffusion_amd.declip_long import declip_passes, declip_plan
    R, step = 3, L - end
    c, rec = _clipped_recordings(R, N, 11 + N)
    rec_d = torch.empty(R, N + 3, device=DEV)[:, 1:N + 1].copy_(rec)
    A, B, _ = declip_plan(rec, np.float32(LEVELS), L, end)
    assert A and (B or N <= L)
    clipped = rec.abs() >= c
    stub, seeds = _Stub(), [5, 6, 7]
    out = declip_passes(stub, rec_d, LEVELS, L, end, max_batch=max_batch, seeds=seeds)
    assert out.is_cuda and torch.equal(out.cpu(), torch.where(clipped, rec + 7, rec))
    assert stub.seeds == "untouched"
    nA, nB = math.ceil(len(A) / max_batch), math.ceil(len(B) / max_batch)
    assert len(stub.calls) == nA + nB and all(call[0].shape[0] <= max_batch and call[0].shape == call[1].shape for call in stub.calls)
    assert sum(call[0].shape[0] for call in stub.calls[:nA]) == len(A) and sum(call[0].shape[0] for call in stub.calls) == len(A) + len(B)
    assert [s for call in stub.calls for s in call[3]] == [seeds[r] * 65536 + s // step for r, s, *_ in A + B]
    assert torch.cat([call[2] for call in stub.calls]).cpu().tolist() == [float(np.float32(LEVELS[r])) for r, *_ in A + B]
    # what pass B sees at its windows' heads and tails is what pass A left there, bit for bit, and it is known; the rest is the clipped recording
    after_A = rec.clone()
    for r, s, head, tail, lo, hi in A:
        after_A[r, s + lo:s + hi] = torch.where(clipped[r, s + lo:s + hi], rec[r, s + lo:s + hi] + 7, rec[r, s + lo:s + hi])
    yB = torch.cat([call[0] for call in stub.calls[nA:]]).cpu() if B else torch.zeros(0, L)
    kB = torch.cat([call[1] for call in stub.calls[nA:]]).cpu() if B else torch.zeros(0, L)
    for j, (r, s, head, tail, lo, hi) in enumerate(B):
        assert head == end and torch.equal(yB[j, :head], after_A[r, s:s + head]) and bool((kB[j, :head] == 1).all())
        if tail:
            assert torch.equal(yB[j, L - tail:], after_A[r, s + L - tail:s + L]) and bool((kB[j, L - tail:] == 1).all())
        n_in = min(L - tail, N - s)
        assert torch.equal(yB[j, head:n_in], rec[r, s + head:s + n_in]) and bool((kB[j, head:n_in] == 0).all()) and bool((kB[j, n_in:L - tail] == -1).all())
    # the global generator when no seeds are given; recordings below their levels make no call and come back as a copy
    stub2 = _Stub()
    out2 = declip_passes(stub2, rec_d, LEVELS, L, end, max_batch=max_batch)
    assert torch.equal(out2, out) and all(call[3] is None for call in stub2.calls) and stub2.seeds == "untouched"
    stub3 = _Stub()
    quiet = rec_d * 0.5
    out3 = declip_passes(stub3, quiet, LEVELS, L, end, max_batch=max_batch, seeds=seeds)
    assert stub3.calls == [] and torch.equal(out3, quiet) and out3.data_ptr() != quiet.data_ptr()


# ---- one window: the existing path -------------------------------------------------------------------------------------------------------
def test_one_window_equals_predict_declipping_bit_for_bit():
    """R = 1, N = L, data consistency off: one job, all samples in state 0 -- the same arithmetic in the same order on one stream."""
    from test_gpu_generic import _sampler
    L, seed, c = 4096, 23, 0.05
    smp = _sampler(L, 3, 0.25, **{"data_consistency.use": False})
    y = (torch.randn(1, L, generator=torch.Generator().manual_seed(4)) * 0.063).clamp(-c, c).to(DEV)
    smp.seeds = [99]
    out = smp.predict_declipping_long(y, c, seeds=[seed])
    assert smp.seeds == [99] and out.is_cuda and out.shape == (1, L)
    smp.seeds = [seed * 65536]
    ref = smp.predict_declipping(y, c)
    assert torch.equal(out, ref) and not torch.equal(out, y)


# ---- data consistency --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dc_type", ["end", "always"])
def test_data_consistency_keeps_the_unclipped_samples_and_the_side_of_the_clipped_ones(dc_type):
    """Two recordings of three windows, toy denoiser.  "end": the final state is projected -- unclipped samples are the recording's bit for bit,
    clipped ones lie at or beyond the level on the recording's side.  "always": every x_hat is projected and the last Euler step onto t = 0,
    x + h * (x - x_hat) / t, leaves the unclipped samples within a handful of roundings of the recording's size (ATOL_OBSERVED of its peak).
    Measured on one MI355X: max |out - y| over the unclipped samples 2.9e-11 against the bound 4.8e-08."""
    from test_gpu_generic import _sampler
    L = 4096
    N = 2 * L + L // 3
    smp = _sampler(L, 3, 0.25, **{"data_consistency.use": True, "data_consistency.type": dc_type})
    c = torch.tensor([0.05, 0.03])[:, None]
    clean = torch.stack([torch.randn(N, generator=torch.Generator().manual_seed(50 + r)) for r in range(2)]) * 0.063
    y = torch.maximum(torch.minimum(clean, c), -c)
    n0 = smp.n_evals
    out = smp.predict_declipping_long(y.to(DEV), [0.05, 0.03], seeds=[3, 4]).cpu()
    assert smp.n_evals - n0 == 6 * (2 * 3 - 1) and bool(torch.isfinite(out).all())
    low = y.abs() < c
    assert not torch.equal(out[~low], y[~low])
    if dc_type == "end":
        assert torch.equal(out[low], y[low])
        assert bool(((out * torch.sign(y))[~low] >= c.expand_as(y)[~low]).all())
    else:
        err = float((out[low] - y[low]).abs().max())
        print(f"declip_long, data consistency 'always': max |out - y| over unclipped samples = {err:.3e} (bound {ATOL_OBSERVED * float(y.abs().max()):.3e})")
        assert err <= ATOL_OBSERVED * float(y.abs().max())


# ---- reduced HIP network -----------------------------------------------------------------------------------------------------------------
def _small_net(xi=0.25, dc=False):
    """Reduced HIP network and its oracle twin (the recipe of tests/test_gpu_degrade.py::_small_net)."""
    from audio_inpainting_diffusion_amd.config import small_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.init import seeded_init_
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    from audio_inpainting_diffusion_amd.sampler import Sampler
    from oracle.edm import OracleEDM
    from oracle.nsgt_cqt import OracleCQT
    from oracle.sampler import OracleSampler
    from oracle.unet import OracleUnet
    z = np.load(os.path.join(GOLDEN, "unet_small_a.npz"))
    kw = ast.literal_eval(str(z["cfg"]))
    args = small_args(**kw)
    args.tester.T, args.tester.posterior_sampling.xi = 3, xi
    args.tester.data_consistency.use = dc
    net = seeded_init_(Unet_CQT_oct_with_attention(args, torch.device(DEV)), int(z["seed"]), gate_scale=10.0, affine_scale=10.0)
    Ls = kw["audio_len"]
    orc = OracleUnet(kw["num_octs"], kw["bins_per_oct"], OracleCQT(kw["num_octs"], kw["bins_per_oct"], "oct", ("kaiser", 1), kw["fs"], Ls)).load_state_dict(net.state_dict())
    smp = Sampler(model=net, diff_params=EDM(args), args=args)
    osmp = OracleSampler(orc, OracleEDM(), T=3, xi=xi, data_consistency=dc, audio_len=Ls)
    return smp, osmp, Ls


def test_hip_network_window_with_known_and_absent_samples_vs_oracle():
    """One pass-B-shaped window per item: the first and last ``end`` samples known, the last 37 absent instead, the rest seen through the clipper
    (levels 0.05 and 0.03), T = 3, guidance only -- predict_resample with ClipObserved against the oracle sampler driven with the same operator
    written as a torch lambda.  Bound: the documented 5e-4 of test_gpu_degrade.py::test_hip_network_bwe_and_declipping_vs_oracle.
    Measured on one MI355X: rel-L2 = 3.33e-06."""
    from audio_inpainting_diffusion_amd.declip_long import ClipObserved
    from audio_inpainting_diffusion_amd.sampler import autoregressive_overlap
    smp, osmp, Ls = _small_net()
    end = int(autoregressive_overlap(smp.args) * Ls)
    c = torch.tensor([0.05, 0.03])[:, None]
    clean = torch.stack([torch.randn(Ls, generator=torch.Generator().manual_seed(40 + i)) for i in range(2)]) * 0.063
    k = torch.zeros(2, Ls)
    k[:, :end] = 1
    k[:, Ls - end:] = 1
    k[:, Ls - 37:] = -1
    deg = lambda x: torch.where(k == 1, x, torch.where(k == 0, torch.maximum(torch.minimum(x, c), -c), torch.zeros_like(x)))
    y = deg(clean)
    assert bool((y[:, Ls - 37:] == 0).all()) and bool((y[:, :end].abs() > c).any()) and bool((y[:, end:Ls - end].abs() <= c).all())
    smp.seeds = [7, 8]
    out = smp.predict_resample(y.to(DEV), (2, Ls), ClipObserved(k.to(DEV), [0.05, 0.03]))
    ref = osmp.predict_resample(y, (2, Ls), deg, seeds=[7, 8])
    e = rel_l2(out.cpu(), ref)
    print(f"HIP network, ClipObserved window: rel-L2 vs oracle = {e:.2e}")
    assert e <= 5e-4


def test_hip_network_result_is_independent_of_the_other_recordings_and_of_max_batch():
    """Two recordings of N = 2 Ls + Ls // 3 samples (three windows each) clipped at 0.05 and 0.03, T = 3; recording 1 is attenuated over the
    owned middle of window 1, so that window is no job.  Declipped together, each alone, and with max_batch 1 against 8; form_batch is left
    unpinned, so the documented bound for results across batch compositions applies (<= 5e-6,
    tests/test_gpu_degrade.py::test_predict_bwe_batch_of_four_takes_the_sub_batch_streams).  The floor is printed next to it:
    predict_declipping itself on the windows of pass A, at batch 1 against all at once.
    Measured on one MI355X: all four comparisons 0.0 (bit-equal), and so is the floor -- the bound stays at the documented 5e-6."""
    from audio_inpainting_diffusion_amd.declip_long import declip_plan
    from audio_inpainting_diffusion_amd.sampler import autoregressive_overlap
    smp, _, Ls = _small_net()
    end = int(autoregressive_overlap(smp.args) * Ls)
    N, step, T = 2 * Ls + Ls // 3, Ls - end, 3
    levels = [0.05, 0.03]
    c = torch.tensor(levels)[:, None]
    clean = torch.stack([torch.randn(N, generator=torch.Generator().manual_seed(70 + r)) for r in range(2)]) * 0.063
    a, b = step + end, step + Ls - end                                       # the owned middle of window 1
    clean[1, a:b] *= 0.9 * levels[1] / float(clean[1, a:b].abs().max())
    rec = torch.maximum(torch.minimum(clean, c), -c)
    assert float(rec[1, a:b].abs().max()) < float(np.float32(levels[1]))
    A, B, _ = declip_plan(rec, np.float32(levels), Ls, end)
    assert len(A) == 4 and B == [(0, step, end, end, end, Ls - end)]
    rec_d = rec.to(DEV)
    seeds = [31, 32]
    n0 = smp.n_evals
    both = smp.predict_declipping_long(rec_d, levels, max_batch=8, seeds=seeds)
    assert smp.n_evals - n0 == 5 * (2 * T - 1) and both.shape == (2, N) and bool(torch.isfinite(both).all())
    assert torch.equal(both[1, a:b], rec_d[1, a:b])                          # no job: the recording's samples, bit for bit
    clipped = rec.abs() >= c
    assert not torch.equal(both.cpu()[clipped], rec[clipped])
    errs = {}
    for r in range(2):
        alone = smp.predict_declipping_long(rec_d[r:r + 1], levels[r], max_batch=8, seeds=seeds[r:r + 1])
        errs[f"recording {r} alone"] = rel_l2(alone.cpu(), both[r:r + 1].cpu())
    one = smp.predict_declipping_long(rec_d, levels, max_batch=1, seeds=seeds)
    for r in range(2):
        errs[f"recording {r} max_batch 1"] = rel_l2(one[r:r + 1].cpu(), both[r:r + 1].cpu())
    yw = torch.stack([rec_d[0, s:s + Ls] for s in (0, step // 2, step, N - Ls)])           # (four windows of recording 0: one level)
    smp.seeds = list(range(1, yw.shape[0] + 1))
    whole = smp.predict_declipping(yw, levels[0])
    floor = []
    for j in range(yw.shape[0]):
        smp.seeds = [j + 1]
        floor.append(rel_l2(smp.predict_declipping(yw[j:j + 1], levels[0]).cpu(), whole[j:j + 1].cpu()))
    print("declip_long batch invariance, rel-L2:", {k: "%.2e" % v for k, v in errs.items()}, "| floor (predict_declipping, batch 1 vs all):", ["%.2e" % e for e in floor])
    assert all(e <= 5e-6 for e in errs.values()), errs
