"""GPU tests of bandwidth extension of whole low-sample-rate recordings (csrc/aid_lowrate_long.hip, lowrate_long.py,
Sampler.predict_bwe_lowrate_long): the operator of known / observed / unobserved / absent entries against float64 torch expressions and bit
for bit against SincResample, the gather bit-exact against Python indexing, the two passes stitched around a stub sampler, one window
against predict_bwe, and the reduced HIP network against the oracle and across batch compositions.  Toy and reduced-size models only."""
import math

import pytest
import torch

from conftest import rel_l2
from test_gpu_bwe_long import SENT, _on_device, _strided

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- the operator ------------------------------------------------------------------------------------------------------------------------
def _rate(o, n, decimate=False):
    from audio_inpainting_diffusion_amd.degrade import sinc_kernel
    from audio_inpainting_diffusion_amd.lowrate_long import Rate
    width = 0 if decimate else sinc_kernel(o, n)[1]
    return Rate(o, n, width, 2 * width + o, decimate)


def _kernel64(rate):
    """the float64 definition: oracle.resample's kernel [new, 1, K], or the decimator's one-row table"""
    from oracle.resample import sinc_resample_kernel
    if rate.decimate:
        k = torch.zeros(1, 1, rate.K, dtype=torch.float64)
        k[0, 0, 0] = 1.0
        return k
    k, width = sinc_resample_kernel(rate.orig, rate.new)
    assert width == rate.width and tuple(k.shape) == (rate.new, 1, rate.K)
    return k


def _resample64(v, k64, rate, Mw):
    """oracle.resample.resample's expression (tests/test_gpu_resample_op.py::_gpu_resampler) in float64 with the given kernel"""
    xp = torch.nn.functional.pad(v, (rate.width, rate.width + rate.orig))
    y = torch.nn.functional.conv1d(xp[:, None], k64, stride=rate.orig).transpose(1, 2).reshape(v.shape[0], -1)
    return y[..., :Mw]


def _apply64(x, k64, rate, state):
    L = x.shape[1]
    kh, kl = state[:, :L].expand(x.shape[0], -1), state[:, L:].expand(x.shape[0], -1)
    c = _resample64(torch.where(kh == -2, torch.zeros_like(x), x), k64, rate, kl.shape[1])
    return torch.cat([torch.where(kh == 1, x, torch.zeros_like(x)), torch.where(kl == 0, c, torch.zeros_like(c))], dim=1)


def _adjoint64(g, k64, rate, state, L):
    """the transposed resampler written out: every observed low-rate entry spreads its kernel row over the K samples it read"""
    B, Mw = g.shape[0], g.shape[1] - L
    kh, kl = state[:, :L].expand(B, -1), state[:, L:].expand(B, -1)
    frames = -(-Mw // rate.new)
    gin = torch.zeros(B, frames * rate.new, dtype=torch.float64)
    gin[:, :Mw] = torch.where(kl == 0, g[:, L:], torch.zeros_like(g[:, L:]))
    a = torch.nn.functional.conv_transpose1d(gin.reshape(B, frames, rate.new).transpose(1, 2), k64, stride=rate.orig).squeeze(1)
    a = torch.nn.functional.pad(a, (0, rate.width + L))[:, rate.width:rate.width + L]
    return torch.where(kh == -2, torch.zeros_like(a), torch.where(kh == 1, a + g[:, :L], a))


def _states(B, L, Mw, gen):
    """high side from {-2, -1, 1}, low side from {-2, -1, 0}, in runs that cross the borders of the 256-thread blocks of both modes (entries
    256, 512, ... of the row and of the high side; L itself is the seam between the two sides), and single changes next to them"""
    kh = torch.randint(-2, 1, (B, L), generator=gen).float()
    kh[kh == 0] = 1.0
    kl = torch.randint(-2, 1, (B, Mw), generator=gen).float()
    k = torch.cat([kh, kl], dim=1)
    hi_run = torch.tensor([-1.0] * 5 + [1.0] * 5 + [-2.0] * 5 + [-1.0] * 4 + [1.0])
    lo_run = torch.tensor([0.0] * 5 + [-1.0] * 5 + [-2.0] * 5 + [0.0] * 4 + [-1.0])
    for border in range(256, L + Mw, 256):
        a = border - 9
        if a + hi_run.numel() <= L:
            k[:, a:a + hi_run.numel()] = hi_run
            k[-1, a:a + hi_run.numel()] = hi_run.flip(0)
        if a >= L and a + lo_run.numel() <= L + Mw:
            k[:, a:a + lo_run.numel()] = lo_run
            k[-1, a:a + lo_run.numel()] = lo_run.flip(0)
    if L >= 8 and Mw >= 8:
        k[:, L - 4:L] = torch.tensor([1.0, -1.0, -2.0, 1.0])
        k[:, L:L + 4] = torch.tensor([0.0, -1.0, -2.0, 0.0])
    return k


def _tables(rate):
    from audio_inpainting_diffusion_amd.lowrate_long import rate_tables
    return rate_tables(rate, DEV)


OP_CASES = [(2, 1, 37, 3, False), (2, 1, 4097, 3, False), (3, 2, 1201, 2, False), (147, 100, 300, 2, False), (147, 100, 4097, 1, False), (5, 1, 41, 2, False),
            (3, 1, 1000, 2, True)]


@pytest.mark.parametrize("o,n,L,B,decimate", OP_CASES)
@pytest.mark.parametrize("shared", [False, True])
def test_rate_observed_modes_against_float64_on_strided_misaligned_rows(o, n, L, B, decimate, shared):
    """apply and adjoint within rel-L2 1e-6 of the float64 expression over oracle.resample's kernel (the bound
    tests/test_gpu_resample_op.py::test_resample_forward_adjoint_and_dot_product holds SincResample to), the adjoint also against autograd
    and by the dot product; what the state selects is exact."""
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.lowrate_long import RateObserved, window_len
    rate = _rate(o, n, decimate)
    Mw = window_len(L, rate)
    row = L + Mw
    gen = torch.Generator().manual_seed(1000 * o + L + B)
    x, gy = torch.randn(B, L, generator=gen), torch.randn(B, row, generator=gen)
    state = _states(B, L, Mw, gen)
    if shared:
        state = state[:1]
    k = state.expand(B, row)
    kh, kl = k[:, :L], k[:, L:]
    assert all(bool((kh == v).any()) for v in (-2, -1, 1)) and all(bool((kl == v).any()) for v in (-2, -1, 0))
    k64 = _kernel64(rate)
    want0 = _apply64(x.double(), k64, rate, state)
    want1 = _adjoint64(gy.double(), k64, rate, state, L)
    xr = x.double().requires_grad_()
    (auto,) = torch.autograd.grad(_apply64(xr, k64, rate, state), xr, gy.double())
    assert rel_l2(want1, auto) <= 1e-12
    tk, width, tkT, tlo, thi = _tables(rate)
    assert width == rate.width and tuple(tk.shape) == (n, rate.K)
    (_, xd), (_, gd), (_, kd) = _on_device(x, 1), _on_device(gy, 0), _on_device(state, 2)
    errs = {}
    for out_shift in (0, 1, 3):
        for mode, src, want in ((0, xd, want0), (1, gd, want1)):
            n_in, n_out = (L, row) if mode == 0 else (row, L)
            obuf, od = _on_device(torch.full((B, n_out), SENT), out_shift)
            guard = torch.full((2, B, n_out + 3), SENT, device=DEV)
            _lib.call("aid_rate_observed", _lib.RateObservedParams(src.data_ptr(), kd.data_ptr(), tk.data_ptr(), tkT.data_ptr(), tlo.data_ptr(), thi.data_ptr(),
                                                                   od.data_ptr(), L, Mw, n_in + 3, 0 if shared else row + 3, n_out + 3,
                                                                   B, mode, o, n, rate.width, rate.K))
            got = od.cpu()
            errs[(out_shift, mode)] = rel_l2(got, want)
            pad = torch.ones(B, n_out + 3, dtype=torch.bool)
            pad[:, out_shift:out_shift + n_out] = False
            assert bool((obuf.cpu()[pad] == SENT).all()) and bool((guard == SENT).all())       # nothing outside the rows of out
            if mode == 0:      # known outputs are x bit for bit; no observation: 0.0
                assert torch.equal(got[:, :L][kh == 1], x[kh == 1]) and bool((got[:, :L][kh != 1] == 0).all()) and bool((got[:, L:][kl != 0] == 0).all())
            else:
                assert bool((got[kh == -2] == 0).all())
    print(f"RateObserved {o}:{n} L={L} B={B} decimate={decimate} shared={shared}: worst rel-L2 vs float64 = {max(errs.values()):.2e}")
    assert all(e <= 1e-6 for e in errs.values()), errs
    # the operator object (contiguous signals; the state keeps its row stride)
    op = RateObserved((tk, width, tkT, tlo, thi), kd)
    assert op.shared_mask is False and (op.orig, op.new, op.K, op.L, op.Mw) == (o, n, rate.K, L, Mw)
    ax, atg = op.apply(xd).cpu(), op.adjoint(gd).cpu()
    assert tuple(ax.shape) == (B, row) and tuple(atg.shape) == (B, L)
    assert rel_l2(ax, want0) <= 1e-6 and torch.equal(op(xd).cpu(), ax)
    assert rel_l2(atg, want1) <= 1e-6 and rel_l2(atg, auto) <= 1e-6
    lhs, rhs = float((ax.double() * gy.double()).sum()), float((x.double() * atg.double()).sum())
    scale = float(ax.double().norm() * gy.double().norm())
    print(f"    <Ax,g> - <x,A^T g> = {abs(lhs - rhs) / scale:.2e} of |Ax||g|")
    assert abs(lhs - rhs) <= 1e-6 * scale
    with pytest.raises(AttributeError):
        op.project(xd, gd)
    if not shared and B > 1:
        sub = op.rows(1, B)
        assert op.rows(1, B) is sub and sub.state.shape[0] == B - 1 and sub.tables is op.tables
        assert torch.equal(sub.apply(xd[1:]).cpu(), ax[1:]) and torch.equal(sub.adjoint(gd[1:]).cpu(), atg[1:])
        for lo, hi in ((1, 1), (-1, 1), (0, B + 1)):
            with pytest.raises(_lib.AidError):
                op.rows(lo, hi)
        with pytest.raises(_lib.AidError):
            op.apply(xd[:1].repeat(B + 1, 1))
    elif shared:
        assert op.rows(0, 1).state.data_ptr() == kd.data_ptr()
    # refusals of the launcher: checked on the host, nothing is launched
    out0 = torch.zeros(B, row, device=DEV)
    for bad in (dict(mode=2), dict(mode=-1), dict(B=0), dict(B=65536), dict(K=rate.K + 1), dict(Mw=Mw + 1), dict(Mw=Mw - 1), dict(x_ld=L - 1), dict(out_ld=row - 1),
                dict(state_ld=row - 1), dict(k=None), dict(mode=1, kT=None), dict(mode=1, x_ld=row - 1)):
        kw = dict(mode=0, B=B, K=rate.K, Mw=Mw, x_ld=row + 3, out_ld=row, state_ld=0 if shared else row + 3, k=tk.data_ptr(), kT=tkT.data_ptr())
        kw.update(bad)
        with pytest.raises(_lib.AidError):
            _lib.call("aid_rate_observed", _lib.RateObservedParams(gd.data_ptr(), kd.data_ptr(), kw["k"], kw["kT"], tlo.data_ptr(), thi.data_ptr(), out0.data_ptr(),
                                                                   L, kw["Mw"], kw["x_ld"], kw["state_ld"], kw["out_ld"], kw["B"], kw["mode"], o, n, rate.width, kw["K"]))
    assert bool((out0 == 0).all())


@pytest.mark.parametrize("o,n", [(2, 1), (147, 100)])
@pytest.mark.parametrize("shared", [False, True])
def test_with_every_low_rate_entry_observed_apply_and_adjoint_are_sinc_resample_bit_for_bit(o, n, shared):
    from audio_inpainting_diffusion_amd.degrade import SincResample, resample_tables
    from audio_inpainting_diffusion_amd.lowrate_long import RateObserved
    B, L = 3, 4097
    ref = SincResample(o, n, L, device=DEV)
    Mw = ref.L_out
    gen = torch.Generator().manual_seed(31 + o)
    xd, gd = torch.randn(B, L, generator=gen).to(DEV), torch.randn(B, Mw, generator=gen).to(DEV)
    state = torch.cat([torch.full((1 if shared else B, L), -1.0), torch.zeros(1 if shared else B, Mw)], dim=1).to(DEV)
    op = RateObserved(resample_tables(o, n, DEV), state)
    ax = op.apply(xd)
    assert torch.equal(ax[:, L:], ref.apply(xd)) and bool((ax[:, :L] == 0).all()) and bool((ax[:, L:] != 0).any())
    assert torch.equal(op.adjoint(torch.cat([torch.zeros(B, L, device=DEV), gd], dim=1)), ref.adjoint(gd))


# ---- the gather --------------------------------------------------------------------------------------------------------------------------
# (factor, filt_type, L, end, N): one window shorter than L, more windows with a last one cut by N, (N - 1) % f == 0, an even and an odd last window
GATHER_CASES = [(2, "resample", 256, 64, 1000), (2, "resample", 256, 64, 1001), (1.5, "resample", 256, 64, 449), (3, "decimate", 256, 64, 769),
                (4, "decimate", 256, 63, 100), (1.47, "resample", 4096, 1024, 9217)]


def _gather_ref(rec, out, N, L, rate, job):
    from audio_inpainting_diffusion_amd.lowrate_long import window_state
    r, s, head, tail, lo, hi = job
    M = rec.shape[1]
    k_ref = torch.from_numpy(window_state(N, M, L, rate, s, head, tail))
    qc = (s + torch.arange(L)).clamp(max=N - 1)
    mc = ((s // rate.orig) * rate.new + torch.arange(k_ref.numel() - L)).clamp(max=M - 1)
    y_ref = torch.cat([torch.where(k_ref[:L] == 1, out[r, qc], torch.zeros(L)), torch.where(k_ref[L:] == 0, rec[r, mc], torch.zeros(mc.numel()))])
    return y_ref, k_ref


@pytest.mark.parametrize("factor,ftype,L,end,N", GATHER_CASES)
def test_lowrate_gather_is_bit_exact_against_python_indexing(factor, ftype, L, end, N):
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.lowrate_long import low_len, lowrate_gather, lowrate_plan, rate_of, window_len
    from audio_inpainting_diffusion_amd.restore import job_table
    R = 3
    rate = rate_of(factor, ftype)
    M, Mw = low_len(N, rate), window_len(L, rate)
    A, B = lowrate_plan(R, N, L, end, rate)
    assert A and (B or N <= L)
    _, rec = _strided(R, M, 1 + N, 0)
    _, out = _strided(R, N, 2 + N, 1)                                            # (its rows start at an odd element)
    rec_d = torch.empty(R, M + 3, device=DEV)[:, :M].copy_(rec)
    out_d = torch.empty(R, N + 3, device=DEV)[:, 1:N + 1].copy_(out)
    # a skipped job: a start that is no multiple of orig, a recording and a start out of range
    bad_jobs = [(0, A[0][1] + 1, 0, 0, 0, L), (R, 0, 0, 0, 0, L), (0, N + (-N % rate.orig), 0, 0, 0, L), (-1, 0, 0, 0, 0, L)]
    for jobs in (A, B, A + bad_jobs[:1] + B + bad_jobs[1:]):
        if not jobs:
            continue
        y, k = lowrate_gather(rec_d, out_d, job_table(jobs, DEV), L, rate)
        assert y.shape == k.shape == (len(jobs), L + Mw)
        for j, job in enumerate(jobs):
            if job in bad_jobs:
                assert bool((y[j] == 0).all()) and bool((k[j] == -2).all()), j
                continue
            y_ref, k_ref = _gather_ref(rec, out, N, L, rate, job)
            assert torch.equal(k[j].cpu(), k_ref) and torch.equal(y[j].cpu(), y_ref), j
        if jobs is A:
            assert not bool((k[:, :L] == 1).any()) and bool((k[:, L:] == 0).any())
            assert bool((k[:, L:] == -1).any()) == (N > L)
        elif jobs is B:
            assert bool((k[:, :L] == 1).any())
    # guarded outputs: nothing before or after the rows is written
    tab = job_table(A + bad_jobs, DEV)
    J, pad = tab.shape[0], 64
    bufs = [torch.full((pad + J * (L + Mw) + pad,), SENT, device=DEV) for _ in range(2)]
    _lib.call("aid_lowrate_gather", _lib.LowrateGatherParams(rec_d.data_ptr(), out_d.data_ptr(), bufs[0][pad:].data_ptr(), bufs[1][pad:].data_ptr(), tab.data_ptr(),
                                                             L, Mw, N, M, M + 3, N + 3, J, R, rate.orig, rate.new, rate.width, rate.K))
    assert all(bool((b[:pad] == SENT).all()) and bool((b[-pad:] == SENT).all()) and not bool((b[pad:-pad] == SENT).any()) for b in bufs)
    y0 = torch.zeros(len(A), L + Mw, device=DEV)
    for bad in (dict(rec_ld=M - 1), dict(out_ld=N - 1), dict(J=0), dict(J=65536), dict(K=rate.K + 1), dict(Mw=Mw + 1), dict(M=0)):
        kw = dict(J=len(A), K=rate.K, Mw=Mw, M=M, rec_ld=M + 3, out_ld=N + 3)
        kw.update(bad)
        with pytest.raises(_lib.AidError):
            _lib.call("aid_lowrate_gather", _lib.LowrateGatherParams(rec_d.data_ptr(), out_d.data_ptr(), y0.data_ptr(), y0.data_ptr(), tab.data_ptr(),
                                                                     L, kw["Mw"], N, kw["M"], kw["rec_ld"], kw["out_ld"], kw["J"], R, rate.orig, rate.new, rate.width, kw["K"]))
    assert bool((y0 == 0).all())


# ---- the two passes around a stub sampler ------------------------------------------------------------------------------------------------
class _Stub:
    """predict_resample(y, shape, op)[j, i] = w_j * L + i + r_j / 4, with (r_j, w_j) read from the job's seed (r_j + 1) * 65536 + w_j: every sample
    names the window it was written from."""

    def __init__(self):
        self.calls, self.seeds = [], "untouched"

    def predict_resample(self, y, shape, op):
        B, L = shape
        assert y.shape[0] == B and op.state.shape == y.shape and (op.L, op.L + op.Mw) == (L, y.shape[1])
        self.calls.append((y.clone(), op.state.clone(), op.tables, self.seeds))
        base = torch.tensor([(s % 65536) * L + (s // 65536 - 1) / 4 for s in self.seeds], dtype=torch.float32, device=y.device)
        return base[:, None] + torch.arange(L, dtype=torch.float32, device=y.device)[None, :]


@pytest.mark.parametrize("factor,ftype,L,end,N", GATHER_CASES)
@pytest.mark.parametrize("max_batch", [2, 8])
def test_two_passes_stitch_the_stub_sampler_output(factor, ftype, L, end, N, max_batch):
    from audio_inpainting_diffusion_amd.lowrate_long import aligned_end, low_len, lowrate_passes, lowrate_plan, rate_of, rate_tables
    rate = rate_of(factor, ftype)
    R, M = 3, low_len(N, rate)
    end2 = aligned_end(L, end, rate.orig)
    step, m = L - end2, rate.K - 1
    _, rec = _strided(R, M, 11 + N, 1)
    rec_d = torch.empty(R, M + 3, device=DEV)[:, 1:M + 1].copy_(rec)
    A, B = lowrate_plan(R, N, L, end, rate)
    stub, seeds = _Stub(), [1, 2, 3]
    out = lowrate_passes(stub, rec_d, factor, ftype, L, end, length=N, max_batch=max_batch, seeds=seeds)
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
    assert [s for call in stub.calls for s in call[3]] == [seeds[r] * 65536 + s // step for r, s, *_ in A + B]
    assert all(call[2] is rate_tables(rate, DEV) for call in stub.calls)
    # pass A sees the recording's low-rate samples and nothing known; pass B sees what pass A left at its heads and tails, bit for bit, as known
    ys, ks = torch.cat([call[0] for call in stub.calls]).cpu(), torch.cat([call[1] for call in stub.calls]).cpu()
    for j, job in enumerate(A + B):
        r, s, head, tail, lo, hi = job
        y_ref, k_ref = _gather_ref(rec, want.nan_to_num(0.0), N, L, rate, job)
        assert torch.equal(ks[j], k_ref) and torch.equal(ys[j], y_ref)
        assert bool((k_ref[L:] == 0).any())
        if j < len(A):
            assert not bool((k_ref == 1).any())
        else:
            assert head == end2 - m and tail in (0, head)
            assert torch.equal(ys[j, :head], want[r, s:s + head]) and bool((k_ref[:head] == 1).all())
            if tail:
                assert torch.equal(ys[j, L - tail:L], want[r, s + L - tail:s + L]) and bool((k_ref[L - tail:L] == 1).all())
            # ... and those samples belong to the even neighbours (pass A wrote them)
            assert bool((want[r, s:s + head] < (s // step) * L).all())
    # the default length (the largest consistent with M), and the global generator when no seeds are given
    class _Plain(_Stub):
        def predict_resample(self, y, shape, op):
            self.calls.append(self.seeds)
            return y[:, :shape[1]] + 1
    from audio_inpainting_diffusion_amd.lowrate_long import default_length
    plain = _Plain()
    full = lowrate_passes(plain, rec_d, factor, ftype, L, end, max_batch=max_batch)
    assert full.shape == (R, default_length(M, rate)) and all(s is None for s in plain.calls) and plain.seeds == "untouched"


# ---- one window: the existing path -------------------------------------------------------------------------------------------------------
def test_one_window_is_predict_bwe_resample():
    """R = 1, N = L, data consistency off, factor 2: one job, every low-rate entry observed and no high-rate one known -- the same resampler
    terms in the same order; the guidance norm runs over L extra zeros, so bit equality is not promised and the bound is 5e-6 rel-L2 (the
    documented bound between two summation orders of one result).
    Measured on one MI355X: 0.0, torch.equal -- the bound stays."""
    from test_gpu_generic import _sampler
    from test_gpu_resample_op import _gpu_resampler
    L, seed = 4096, 23
    smp = _sampler(L, 3, 0.25, **{"data_consistency.use": False})
    clean = torch.randn(1, L, generator=torch.Generator().manual_seed(4)) * 0.063
    y = _gpu_resampler(2, 1)(clean).to(DEV)
    assert tuple(y.shape) == (1, L // 2)
    smp.seeds = [99]
    out = smp.predict_bwe_lowrate_long(y, 2, seeds=[seed])
    assert smp.seeds == [99] and out.is_cuda and out.shape == (1, L)
    assert torch.equal(out, smp.predict_bwe_lowrate_long(y, 2, "resample", length=L, max_batch=1, seeds=[seed]))
    smp.seeds = [seed * 65536]
    ref = smp.predict_bwe(y, 2, "resample")
    e = rel_l2(out.cpu(), ref.cpu())
    print(f"one window, predict_bwe_lowrate_long vs predict_bwe resample: rel-L2 = {e:.2e}, bit-equal: {torch.equal(out, ref)}")
    assert e <= 5e-6 and not torch.equal(out[:, :L // 2], y)


def test_the_sampler_refuses_on_the_gpu_what_it_refuses_on_the_host():
    from test_gpu_generic import _sampler
    from audio_inpainting_diffusion_amd import _lib
    L = 4096
    y = torch.zeros(2, L, device=DEV)
    for dc in ("always", "end"):
        smp = _sampler(L, 3, 0.25, **{"data_consistency.use": True, "data_consistency.type": dc})
        with pytest.raises(_lib.AidError, match="data consistency"):
            smp.predict_bwe_lowrate_long(y, 2)
        assert smp.n_evals == 0
    smp = _sampler(L, 3, 0.25, **{"data_consistency.use": False})
    for call, why in ((lambda: smp.predict_bwe_lowrate_long(y, 1), "identity"), (lambda: smp.predict_bwe_lowrate_long(y, 2, length=2 * L + 1), "not consistent"),
                      (lambda: smp.predict_bwe_lowrate_long(y, 2, seeds=[1]), "seeds"), (lambda: smp.predict_bwe_lowrate_long(y.cpu(), 2), "GPU only")):
        with pytest.raises(_lib.AidError, match=why):
            call()
    assert smp.n_evals == 0 and smp.y is None


# ---- reduced HIP network -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [2, 1.47])
def test_hip_network_pass_a_and_pass_b_shaped_windows_vs_oracle(factor):
    """Item 0 is shaped as a window of pass A: the low-rate entries whose kernel support leaves the window at its start unobserved, the last 37
    samples absent and with them the low-rate entries past the recording's last one, and the three frames before those unobserved.  Item 1 as one of pass B: the first and last end' - (K - 1) samples known, every low-rate entry
    observed.  T = 3, guidance only -- predict_resample with RateObserved against the oracle sampler driven with the same operator written
    as a torch lambda over oracle.resample.  Bound: the documented 5e-4 of
    tests/test_gpu_resample_op.py::test_hip_network_bwe_resample_vs_oracle.
    Measured on one MI355X: rel-L2 = 4.87e-06 (factor 2) and 6.95e-06 (factor 1.47)."""
    from test_gpu_degrade import _small_net
    from audio_inpainting_diffusion_amd.lowrate_long import RateObserved, aligned_end, rate_of, rate_tables, window_len
    from audio_inpainting_diffusion_amd.sampler import autoregressive_overlap
    from oracle.resample import resample
    smp, osmp, Ls, _ = _small_net()
    rate = rate_of(factor)
    o, n, m = rate.orig, rate.new, rate.K - 1
    Mw = window_len(Ls, rate)
    end2 = aligned_end(Ls, int(autoregressive_overlap(smp.args) * Ls), o)
    assert end2 >= 2 * m
    clean = torch.stack([torch.randn(Ls, generator=torch.Generator().manual_seed(40 + i)) for i in range(2)]) * 0.063
    k = torch.cat([torch.full((2, Ls), -1.0), torch.zeros(2, Mw)], dim=1)
    a0 = (torch.arange(Mw) // n) * o - rate.width
    gone = -(-n * (Ls - 37) // o)                                            # the low-rate samples of a recording that ends 37 samples early
    k[0, Ls - 37:Ls] = -2
    k[0, Ls:][a0 < 0] = -1
    k[0, Ls + gone - 3 * n:Ls + gone] = -1
    k[0, Ls + gone:] = -2
    k[1, :end2 - m] = 1
    k[1, Ls - (end2 - m):Ls] = 1
    kh, kl = k[:, :Ls], k[:, Ls:]
    assert all(bool((kl[0] == v).any()) for v in (-2, -1, 0)) and bool((kh[1] == 1).any())

    def deg(x):
        c = resample(torch.where(kh == -2, torch.zeros_like(x), x), o, n)
        return torch.cat([torch.where(kh == 1, x, torch.zeros_like(x)), torch.where(kl == 0, c, torch.zeros_like(c))], dim=1)
    y = deg(clean)
    assert tuple(y.shape) == (2, Ls + Mw) and torch.equal(y[1, :Ls][kh[1] == 1], clean[1][kh[1] == 1]) and bool((y[0, :Ls] == 0).all())
    smp.seeds = [7, 8]
    out = smp.predict_resample(y.to(DEV), (2, Ls), RateObserved(rate_tables(rate, DEV), k.to(DEV)))
    ref = osmp.predict_resample(y, (2, Ls), deg, seeds=[7, 8])
    e = rel_l2(out.cpu(), ref)
    print(f"HIP network, RateObserved windows at factor {factor} ({o}:{n}): rel-L2 vs oracle = {e:.2e}")
    assert e <= 5e-4


def test_hip_network_result_is_independent_of_the_other_recordings_and_of_max_batch():
    """Two recordings of N = 2 Ls + Ls // 3 samples (three windows each) resampled 2:1, T = 3.  Restored together, each alone, and with
    max_batch 1 against 8; form_batch is left unpinned, so the documented bound for results across batch compositions applies (<= 5e-6,
    tests/test_gpu_resample_op.py::test_predict_bwe_resample_batch_of_four_takes_the_sub_batch_streams).
    Measured on one MI355X: all four comparisons 0.0 (bit-equal) -- the bound stays at the documented 5e-6."""
    from test_gpu_degrade import _small_net
    from audio_inpainting_diffusion_amd.lowrate_long import lowrate_plan, rate_of
    from audio_inpainting_diffusion_amd.sampler import autoregressive_overlap
    from oracle.resample import resample
    smp, _, Ls, _ = _small_net()
    T = 3
    end = int(autoregressive_overlap(smp.args) * Ls)
    N = 2 * Ls + Ls // 3
    clean = torch.stack([torch.randn(N, generator=torch.Generator().manual_seed(70 + r)) for r in range(2)]) * 0.063
    rec_d = resample(clean, 2, 1).to(DEV)
    A, B = lowrate_plan(2, N, Ls, end, rate_of(2))
    assert len(A) == 4 and len(B) == 2
    seeds = [31, 32]
    n0 = smp.n_evals
    both = smp.predict_bwe_lowrate_long(rec_d, 2, "resample", length=N, max_batch=8, seeds=seeds)
    assert smp.n_evals - n0 == 6 * (2 * T - 1) and both.shape == (2, N) and bool(torch.isfinite(both).all())
    errs = {}
    for r in range(2):
        alone = smp.predict_bwe_lowrate_long(rec_d[r:r + 1], 2, "resample", length=N, max_batch=8, seeds=seeds[r:r + 1])
        errs[f"recording {r} alone"] = rel_l2(alone.cpu(), both[r:r + 1].cpu())
    one = smp.predict_bwe_lowrate_long(rec_d, 2, "resample", length=N, max_batch=1, seeds=seeds)
    for r in range(2):
        errs[f"recording {r} max_batch 1"] = rel_l2(one[r:r + 1].cpu(), both[r:r + 1].cpu())
    print("bwe_lowrate_long batch invariance, rel-L2:", {k: "%.2e" % v for k, v in errs.items()})
    assert all(e <= 5e-6 for e in errs.values()), errs
