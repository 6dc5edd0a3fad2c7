"""GPU tests of phase retrieval of whole recordings (csrc/aid_phase_long.hip, phase_long.py, Sampler.predict_pr_long): the operator of known /
absent samples and observed / unobserved / absent frames against float64 torch expressions and bit for bit against STFTMagnitude, the gather
bit-exact against Python indexing, the two passes stitched around a stub sampler, one window against predict_resample, and the reduced HIP
network against the oracle and across batch compositions.  Toy and reduced-size models only."""
import math

import pytest
import torch

from conftest import rel_l2
from test_gpu_bwe_long import SENT, _on_device
from test_gpu_phase import _harmonic, _ref_stft_mag

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- the operator ------------------------------------------------------------------------------------------------------------------------
def _mag64(x, N, hop, safe):
    """|STFT| as tests/test_gpu_phase.py::_ref_stft_mag.  ``safe``: the same values with gradient 0 where |X| = 0 (the kernels' rule; autograd
    through sqrt gives 0 * inf = NaN there)"""
    if not safe:
        return _ref_stft_mag(x, N, hop)
    x2 = torch.cat((x, torch.zeros(x.shape[0], N, dtype=x.dtype)), -1)
    X = torch.view_as_real(torch.stft(x2, N, hop_length=hop, window=torch.hamming_window(N, dtype=x.dtype), center=False, return_complex=True))
    p = X[..., 0] ** 2 + X[..., 1] ** 2
    return torch.where(p > 0, torch.sqrt(torch.where(p > 0, p, torch.ones_like(p))), torch.zeros_like(p))


def _apply64(x, state, N, hop, safe=True):
    """the operator with its selects written in torch: x [B, L], state [1|B, L + Tw] -> [B, L + F*Tw]"""
    B, L = x.shape
    kh, kf = state[:, :L].expand(B, -1), state[:, L:].expand(B, -1)
    mag = _mag64(torch.where(kh <= -2, torch.zeros_like(x), x), N, hop, safe)
    mag = torch.where((kf == 0)[:, None, :], mag, torch.zeros_like(mag))
    return torch.cat([torch.where(kh > 0, x, torch.zeros_like(x)), mag.reshape(B, -1)], dim=1)


def _states(B, L, N, hop, gen):
    """samples from {-2, -1, 1}, frames from {-2, -1, 0}.  Row 0: frame 0 unobserved, frame 1 observed over absent samples only, frame 2 absent"""
    Tw = 1 + L // hop
    kh = torch.randint(-2, 1, (B, L), generator=gen).float()
    kh[kh == 0] = 1.0
    kf = torch.randint(-2, 1, (B, Tw), generator=gen).float()
    kf[0, :3] = torch.tensor([-1.0, 0.0, -2.0])
    kh[0, hop:hop + N] = -2.0
    kh[0, 0], kh[0, 1] = 1.0, -1.0
    return torch.cat([kh, kf], dim=1)


OP_CASES = [(16, 16, 53, 1), (16, 5, 200, 3), (256, 64, 2085, 3), (1024, 256, 4133, 2), (2048, 512, 16384, 1), (8192, 2048, 24576, 1)]


@pytest.mark.parametrize("N,hop,L,B", OP_CASES)
@pytest.mark.parametrize("shared", [False, True])
def test_stft_mag_observed_modes_against_float64_on_strided_misaligned_rows(N, hop, L, B, shared):
    """apply within rel-L2 2e-6 and the VJP within 1e-5 of torch.stft and autograd in float64 (the bounds tests/test_gpu_phase.py holds
    STFTMagnitude to); what the state selects is exact; an observed frame over absent samples only gives magnitude 0 and gradient 0.
    Measured on one MI355X over the six shapes: forward 4.0e-08 ... 1.1e-07, VJP 9.4e-09 ... 3.5e-07."""
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.phase_long import STFTMagObserved, tables
    F, Tw = N // 2 + 1, 1 + L // hop
    row = L + F * Tw
    gen = torch.Generator().manual_seed(1000 * N + L + B)
    x, gy = torch.randn(B, L, generator=gen) * 0.1, torch.randn(B, row, generator=gen)
    state = _states(B, L, N, hop, gen)
    if shared:
        state = state[:1]
    k = state.expand(B, L + Tw)
    kh, kf = k[:, :L], k[:, L:]
    assert all(bool((kh == v).any()) for v in (-2, -1, 1)) and all(bool((kf == v).any()) for v in (-2, -1, 0))
    obs = (kf == 0)[:, None, :].expand(B, F, Tw).reshape(B, -1)
    want0 = _apply64(x.double(), state, N, hop)
    assert torch.equal(want0, _apply64(x.double(), state, N, hop, safe=False))
    assert bool((want0[0, L:].reshape(F, Tw)[:, 1] == 0).all()) and bool((want0[:, L:][obs] != 0).any())      # the frame over absent samples; the others
    xr = x.double().requires_grad_()
    (want1,) = torch.autograd.grad(_apply64(xr, state, N, hop), xr, gy.double())
    assert bool(torch.isfinite(want1).all())
    window, twiddle = tables(N, DEV)
    (_, xd), (_, gd), (_, kd) = _on_device(x, 1), _on_device(gy, 0), _on_device(state, 2)
    frames = torch.empty(B, Tw, N, device=DEV)
    errs = {}
    for out_shift in (0, 1, 3):
        for mode, want in ((0, want0), (1, want1)):
            n_out = row if mode == 0 else L
            obuf, od = _on_device(torch.full((B, n_out), SENT), out_shift)
            guard = torch.full((2, B, n_out + 3), SENT, device=DEV)
            _lib.call("aid_stft_mag_observed", _lib.StftMagObservedParams(xd.data_ptr(), gd.data_ptr() if mode else None, kd.data_ptr(), window.data_ptr(),
                                                                          twiddle.data_ptr(), frames.data_ptr() if mode else None, od.data_ptr(),
                                                                          L, L + 3, row + 3, 0 if shared else L + Tw + 3, n_out + 3, B, N, hop, Tw, mode))
            got = od.cpu()
            pad = torch.ones(B, n_out + 3, dtype=torch.bool)
            pad[:, out_shift:out_shift + n_out] = False
            assert bool((obuf.cpu()[pad] == SENT).all()) and bool((guard == SENT).all())       # nothing outside the rows of out
            assert bool(torch.isfinite(got).all())
            if mode == 0:      # known outputs are x bit for bit; no observation: 0.0
                errs[(out_shift, 0)] = rel_l2(got[:, L:], want[:, L:])
                assert torch.equal(got[:, :L][kh == 1], x[kh == 1]) and bool((got[:, :L][kh != 1] == 0).all()) and bool((got[:, L:][~obs] == 0).all())
                assert bool((got[0, L:].reshape(F, Tw)[:, 1] == 0).all())
            else:
                errs[(out_shift, 1)] = max(rel_l2(got, want), rel_l2(got[kh != 1], want[kh != 1]))     # (with and without the g added at known samples)
                assert bool((got[kh == -2] == 0).all())
    fwd, vjp = max(v for (_, m), v in errs.items() if m == 0), max(v for (_, m), v in errs.items() if m == 1)
    print(f"STFTMagObserved N={N} hop={hop} L={L} B={B} shared={shared}: worst rel-L2 vs float64: forward {fwd:.2e}, VJP {vjp:.2e}")
    assert fwd <= 2e-6 and vjp <= 1e-5, errs
    # the operator object (contiguous signals; the state keeps its row stride)
    op = STFTMagObserved(N, hop, kd)
    assert op.shared_mask is False and getattr(op, "matrix_obs", None) is None and (op.N, op.hop, op.L, op.F, op.T, op.row) == (N, hop, L, F, Tw, row)
    with pytest.raises(_lib.AidError, match="matching apply"):
        op.adjoint(gd)
    ax = op.apply(xd).cpu()
    atg = op.adjoint(gd).cpu()
    assert tuple(ax.shape) == (B, row) and tuple(atg.shape) == (B, L)
    assert rel_l2(ax[:, L:], want0[:, L:]) <= 2e-6 and torch.equal(op(xd).cpu(), ax) and rel_l2(atg, want1) <= 1e-5
    with pytest.raises(AttributeError):
        op.project(xd, gd)
    # refusals of the launcher: checked on the host, nothing is launched
    out0 = torch.zeros(B, row, device=DEV)
    for bad in (dict(mode=2), dict(mode=-1), dict(B=0), dict(B=65536), dict(n_fft=N + 1), dict(n_fft=8), dict(n_fft=16384), dict(hop=0), dict(hop=N + 1),
                dict(Tw=Tw + 1), dict(Tw=Tw - 1), dict(x_ld=L - 1), dict(out_ld=row - 1), dict(state_ld=L + Tw - 1), dict(mode=1, g=None), dict(mode=1, frames=None),
                dict(mode=1, g_ld=row - 1), dict(mode=1, out_ld=L - 1)):
        kw = dict(mode=0, B=B, n_fft=N, hop=hop, Tw=Tw, x_ld=L + 3, g_ld=row + 3, out_ld=row, state_ld=0 if shared else L + Tw + 3, g=gd.data_ptr(), frames=frames.data_ptr())
        kw.update(bad)
        with pytest.raises(_lib.AidError):
            _lib.call("aid_stft_mag_observed", _lib.StftMagObservedParams(xd.data_ptr(), kw["g"], kd.data_ptr(), window.data_ptr(), twiddle.data_ptr(), kw["frames"],
                                                                          out0.data_ptr(), L, kw["x_ld"], kw["g_ld"], kw["state_ld"], kw["out_ld"], kw["B"], kw["n_fft"],
                                                                          kw["hop"], kw["Tw"], kw["mode"]))
    assert bool((out0 == 0).all())


@pytest.mark.parametrize("N,hop,L", [(256, 64, 2085), (1024, 256, 4096)])
@pytest.mark.parametrize("shared", [False, True])
def test_with_every_frame_observed_apply_and_adjoint_are_stft_magnitude_bit_for_bit(N, hop, L, shared):
    from audio_inpainting_diffusion_amd.phase import STFTMagnitude
    from audio_inpainting_diffusion_amd.phase_long import STFTMagObserved
    B = 3
    ref = STFTMagnitude(N, hop, L, device=DEV)
    gen = torch.Generator().manual_seed(31 + N)
    xd, gd = (torch.randn(B, L, generator=gen) * 0.1).to(DEV), torch.randn(B, ref.F, ref.T, generator=gen).to(DEV)
    state = torch.cat([torch.full((1 if shared else B, L), -1.0), torch.zeros(1 if shared else B, ref.T)], dim=1).to(DEV)
    op = STFTMagObserved(N, hop, state)
    ax, want = op.apply(xd), ref.apply(xd)
    assert torch.equal(ax[:, L:].reshape(B, ref.F, ref.T), want) and bool((ax[:, :L] == 0).all()) and bool((want != 0).any())
    assert torch.equal(op.adjoint(torch.cat([torch.zeros(B, L, device=DEV), gd.reshape(B, -1)], dim=1)), ref.adjoint(gd))


def test_rows_are_the_slices_of_the_whole_batch_and_two_streams_keep_their_own_point_of_linearisation():
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.phase_long import STFTMagObserved
    N, hop, L, B = 256, 64, 2085, 4
    gen = torch.Generator().manual_seed(5)
    state = _states(B, L, N, hop, gen).to(DEV)
    op = STFTMagObserved(N, hop, state)
    xa, xb = ((torch.randn(B, L, generator=gen) * 0.1).to(DEV) for _ in range(2))
    g = torch.randn(B, op.row, generator=gen).to(DEV)
    ax, atg = op.apply(xa), op.adjoint(g)
    bx, btg = op.apply(xb), op.adjoint(g)
    assert not torch.equal(atg, btg)
    lo_op, hi_op = op.rows(0, 2), op.rows(2, 4)
    assert op.rows(0, 2) is lo_op and lo_op.state.shape[0] == 2 and lo_op.window is op.window and hi_op.state.data_ptr() == state[2:].data_ptr()
    for lo, hi in ((1, 1), (-1, 1), (0, B + 1)):
        with pytest.raises(_lib.AidError):
            op.rows(lo, hi)
    with pytest.raises(_lib.AidError):
        op.apply(xa[:1].repeat(B + 1, 1))
    shared = STFTMagObserved(N, hop, state[:1])
    assert shared.rows(0, 3).state.data_ptr() == state.data_ptr()
    # two sub-operators on two streams, applies interleaved before the adjoints; then ONE operator on two streams at two points
    cur, s1, s2 = torch.cuda.current_stream(), torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(cur)
    s2.wait_stream(cur)
    with torch.cuda.stream(s1):
        a1 = lo_op.apply(xa[:2])
        c1 = shared.apply(xa[:1])
    with torch.cuda.stream(s2):
        a2 = hi_op.apply(xb[2:])
        c2 = shared.apply(xb[:1])
    with torch.cuda.stream(s1):
        g1 = lo_op.adjoint(g[:2])
        d1 = shared.adjoint(g[:1])
    with torch.cuda.stream(s2):
        g2 = hi_op.adjoint(g[2:])
        d2 = shared.adjoint(g[:1])
    cur.wait_stream(s1)
    cur.wait_stream(s2)
    torch.cuda.synchronize()
    assert torch.equal(a1, ax[:2]) and torch.equal(a2, bx[2:]) and torch.equal(g1, atg[:2]) and torch.equal(g2, btg[2:])
    assert torch.equal(c1, ax[:1]) and torch.equal(c2, bx[:1]) and torch.equal(d1, atg[:1]) and torch.equal(d2, btg[:1])
    assert len(shared._frames) == 2 and len(shared._x) == 2                         # (scratch and x_hat per stream)


# ---- the gather --------------------------------------------------------------------------------------------------------------------------
# (N, L, end, n_fft, hop): the host cases with more than one window
GATHER_CASES = [(9000, 4096, 1024, 256, 64), (9000, 4096, 1024, 256, 60), (9557, 4096, 1024, 256, 256), (12288, 4096, 1024, 512, 128), (20000, 4096, 1024, 256, 37)]


def _strided_spec(R, F, T, seed):
    """[R, F, T] view into a [R, F + 1, T + 3] buffer (item stride (F + 1)(T + 3), bin stride T + 3, first element misaligned), on the host"""
    base = torch.randn(R, F + 1, T + 3, generator=torch.Generator().manual_seed(seed)).abs()
    return base, base[:, :F, 1:T + 1]


def _gather_ref(rec, out, N, L, n_fft, hop, job):
    from audio_inpainting_diffusion_amd.phase_long import window_state
    r, s, head, tail, lo, hi = job
    k_ref = torch.from_numpy(window_state(N, L, n_fft, hop, s, head, tail))
    qc = (s + torch.arange(L)).clamp(max=N - 1)
    tc = (s // hop + torch.arange(k_ref.numel() - L)).clamp(max=rec.shape[2] - 1)
    cols = torch.where((k_ref[L:] == 0)[None, :], rec[r][:, tc], torch.zeros(rec.shape[1], tc.numel()))
    return torch.cat([torch.where(k_ref[:L] == 1, out[r, qc], torch.zeros(L)), cols.reshape(-1)]), k_ref


@pytest.mark.parametrize("N,L,end,n_fft,hop", GATHER_CASES)
def test_pr_gather_is_bit_exact_against_python_indexing(N, L, end, n_fft, hop):
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.phase_long import frames_of, pr_gather, pr_plan
    from audio_inpainting_diffusion_amd.restore import job_table
    R, F, T_rec, Tw = 3, n_fft // 2 + 1, frames_of(N, hop), frames_of(L, hop)
    row = L + F * Tw
    A, B = pr_plan(R, N, L, end, n_fft, hop)
    assert A and B
    base, rec = _strided_spec(R, F, T_rec, 1 + N)
    out = torch.randn(R, N, generator=torch.Generator().manual_seed(2 + N))
    rec_d = base.to(DEV)[:, :F, 1:T_rec + 1]
    out_d = torch.empty(R, N + 3, device=DEV)[:, 1:N + 1].copy_(out)           # (its rows start at an odd element)
    assert rec_d.stride() == ((F + 1) * (T_rec + 3), T_rec + 3, 1)
    # skipped jobs: a start off the hop grid (hop > 1 in every case), a recording and a start out of range
    bad_jobs = [(0, A[1][1] + 1, 0, 0, 0, L), (R, 0, 0, 0, 0, L), (0, N + (-N % hop), 0, 0, 0, L), (-1, 0, 0, 0, 0, L)]
    assert bad_jobs[0][1] % hop and bad_jobs[0][1] < N
    for jobs in (A, B, A + bad_jobs[:1] + B + bad_jobs[1:]):
        y, k = pr_gather(rec_d, out_d, job_table(jobs, DEV), L, n_fft, hop)
        assert y.shape == (len(jobs), row) and k.shape == (len(jobs), L + Tw)
        for j, job in enumerate(jobs):
            if job in bad_jobs:
                assert bool((y[j] == 0).all()) and bool((k[j] == -2).all()), j
                continue
            y_ref, k_ref = _gather_ref(rec, out, N, L, n_fft, hop, job)
            assert torch.equal(k[j].cpu(), k_ref) and torch.equal(y[j].cpu(), y_ref), j
        if jobs is A:
            assert not bool((k[:, :L] == 1).any()) and bool((k[:, L:] == 0).any()) and bool((k[:, L:] == -1).any())
        elif jobs is B:
            assert bool((k[:, :L] == 1).any())
    # guarded outputs: nothing before or after the rows is written
    tab = job_table(A + bad_jobs, DEV)
    J, pad = tab.shape[0], 64
    bufs = [torch.full((pad + J * n + pad,), SENT, device=DEV) for n in (row, L + Tw)]
    _lib.call("aid_pr_gather", _lib.PrGatherParams(rec_d.data_ptr(), out_d.data_ptr(), bufs[0][pad:].data_ptr(), bufs[1][pad:].data_ptr(), tab.data_ptr(),
                                                   L, N, T_rec, rec_d.stride(0), rec_d.stride(1), N + 3, J, R, n_fft, hop, Tw))
    assert all(bool((b[:pad] == SENT).all()) and bool((b[-pad:] == SENT).all()) and not bool((b[pad:-pad] == SENT).any()) for b in bufs)
    y0 = torch.zeros(len(A), row, device=DEV)
    for bad in (dict(bin_ld=T_rec - 1), dict(rec_ld=F * (T_rec + 3) - 4), dict(out_ld=N - 1), dict(J=0), dict(J=65536), dict(Tw=Tw + 1), dict(T_rec=T_rec + 1),
                dict(n_fft=n_fft + 2), dict(hop=0)):
        kw = dict(J=len(A), Tw=Tw, T_rec=T_rec, rec_ld=rec_d.stride(0), bin_ld=rec_d.stride(1), out_ld=N + 3, n_fft=n_fft, hop=hop)
        kw.update(bad)
        with pytest.raises(_lib.AidError):
            _lib.call("aid_pr_gather", _lib.PrGatherParams(rec_d.data_ptr(), out_d.data_ptr(), y0.data_ptr(), y0.data_ptr(), tab.data_ptr(),
                                                           L, N, kw["T_rec"], kw["rec_ld"], kw["bin_ld"], kw["out_ld"], kw["J"], R, kw["n_fft"], kw["hop"], kw["Tw"]))
    assert bool((y0 == 0).all())


# ---- the two passes around a stub sampler ------------------------------------------------------------------------------------------------
class _Stub:
    """predict_resample(y, shape, op)[j, i] = w_j * L + i + r_j / 4, with (r_j, w_j) read from the job's seed (r_j + 1) * 65536 + w_j: every sample
    names the window it was written from."""

    def __init__(self):
        self.calls, self.seeds = [], "untouched"

    def predict_resample(self, y, shape, op):
        B, L = shape
        assert y.shape == (B, op.row) and op.state.shape == (B, L + op.T) and op.L == L and getattr(op, "matrix_obs", None) is None
        self.calls.append((y.clone(), op.state.clone(), (op.N, op.hop), self.seeds))
        base = torch.tensor([(s % 65536) * L + (s // 65536 - 1) / 4 for s in self.seeds], dtype=torch.float32, device=y.device)
        return base[:, None] + torch.arange(L, dtype=torch.float32, device=y.device)[None, :]


@pytest.mark.parametrize("N,L,end,n_fft,hop", GATHER_CASES)
@pytest.mark.parametrize("max_batch", [2, 8])
def test_two_passes_stitch_the_stub_sampler_output(N, L, end, n_fft, hop, max_batch):
    from audio_inpainting_diffusion_amd.restore import aligned_end
    from audio_inpainting_diffusion_amd.phase_long import default_length, frames_of, pr_passes, pr_plan
    R, F, T_rec = 3, n_fft // 2 + 1, frames_of(N, hop)
    end2 = aligned_end(L, end, hop)
    step, m = L - end2, n_fft - 1
    base, rec = _strided_spec(R, F, T_rec, 11 + N)
    rec_d = base.to(DEV)[:, :F, 1:T_rec + 1]
    A, B = pr_plan(R, N, L, end, n_fft, hop)
    stub, seeds = _Stub(), [1, 2, 3]
    out = pr_passes(stub, rec_d, n_fft, hop, L, end, length=N, max_batch=max_batch, seeds=seeds)
    assert out.is_cuda and out.shape == (R, N) and stub.seeds == "untouched"
    # every sample of [0, N) comes from the window that owns it, and from no other
    want = torch.full((R, N), float("nan"))
    for r, s, head, tail, lo, hi in A + B:
        assert bool(torch.isnan(want[r, s + lo:s + hi]).all())
        want[r, s + lo:s + hi] = (s // step) * L + torch.arange(lo, hi) + r / 4
    assert torch.equal(out.cpu(), want)
    nA, nB = math.ceil(len(A) / max_batch), math.ceil(len(B) / max_batch)
    assert len(stub.calls) == nA + nB and all(call[0].shape[0] <= max_batch and call[0].shape[0] == call[1].shape[0] for call in stub.calls)
    assert sum(call[0].shape[0] for call in stub.calls[:nA]) == len(A) and sum(call[0].shape[0] for call in stub.calls) == len(A) + len(B)
    assert [s for call in stub.calls for s in call[3]] == [seeds[r] * 65536 + s // step for r, s, *_ in A + B]
    assert all(call[2] == (n_fft, hop) for call in stub.calls)
    # pass A sees the recording's magnitude columns and nothing known; pass B sees what pass A left at its heads and tails, bit for bit, as known
    ys, ks = torch.cat([call[0] for call in stub.calls]).cpu(), torch.cat([call[1] for call in stub.calls]).cpu()
    for j, job in enumerate(A + B):
        r, s, head, tail, lo, hi = job
        y_ref, k_ref = _gather_ref(rec, want.nan_to_num(0.0), N, L, n_fft, hop, job)
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

    # the default length (the largest consistent with T_rec), and the global generator when no seeds are given
    class _Plain(_Stub):
        def predict_resample(self, y, shape, op):
            self.calls.append(self.seeds)
            return y[:, :shape[1]] + 1
    plain = _Plain()
    full = pr_passes(plain, rec_d, n_fft, hop, L, end, max_batch=max_batch)
    assert full.shape == (R, default_length(T_rec, hop)) and all(s is None for s in plain.calls) and plain.seeds == "untouched"


# ---- one window: the existing path -------------------------------------------------------------------------------------------------------
class _FlatMagnitude:
    """STFTMagnitude with L zeros in front of the flattened magnitudes and no matrix_obs: what STFTMagObserved is with every frame observed and
    no sample known or absent"""
    shared_mask = True

    def __init__(self, op):
        self.op = op

    def apply(self, x):
        m = self.op.apply(x)
        return torch.cat([torch.zeros(x.shape[0], self.op.L, device=x.device), m.reshape(x.shape[0], -1)], dim=1)

    def adjoint(self, g):
        return self.op.adjoint(g[:, self.op.L:])

    def __call__(self, x):
        return self.apply(x)


def test_one_window_is_predict_resample_through_stft_magnitude_and_differs_from_predict_pr():
    """R = 1, N = L = 4096, win_size 256, hop_size 64, T = 3: one job, every frame observed and no sample known -- the same frame terms in the
    same order as STFTMagnitude's; bound 5e-6 rel-L2 (the documented bound between two summation orders of one result).  predict_pr on the
    same input takes the induced matrix norm of the spectrogram, predict_pr_long the element-wise norm of the row: the results must differ.
    Measured on one MI355X: 0.0, torch.equal -- the bound stays; against predict_pr rel-L2 = 3.18e-01."""
    from test_gpu_generic import _sampler
    from audio_inpainting_diffusion_amd.phase import STFTMagnitude
    L, N, hop, seed = 4096, 256, 64, 23
    smp = _sampler(L, 3, 0.25, **{"data_consistency.use": False, "phase_retrieval.win_size": N, "phase_retrieval.hop_size": hop})
    y = _ref_stft_mag(_harmonic(L, 1, 4), N, hop).to(DEV)
    assert tuple(y.shape) == (1, N // 2 + 1, 1 + L // hop)
    smp.seeds = [99]
    out = smp.predict_pr_long(y, length=L, seeds=[seed])
    assert smp.seeds == [99] and out.is_cuda and out.shape == (1, L)
    assert torch.equal(out, smp.predict_pr_long(y, length=L, max_batch=1, seeds=[seed]))
    smp.seeds = [seed * 65536]
    ref = smp.predict_resample(torch.cat([torch.zeros(1, L, device=DEV), y.reshape(1, -1)], dim=1), (1, L), _FlatMagnitude(STFTMagnitude(N, hop, L, device=DEV)))
    e = rel_l2(out.cpu(), ref.cpu())
    smp.seeds = [seed * 65536]
    pr = smp.predict_pr(y)
    d = rel_l2(out.cpu(), pr.cpu())
    print(f"one window, predict_pr_long vs predict_resample through STFTMagnitude: rel-L2 = {e:.2e}, bit-equal: {torch.equal(out, ref)}; "
          f"vs predict_pr (induced matrix norm): rel-L2 = {d:.2e}")
    assert e <= 5e-6
    assert not torch.equal(out, pr) and d > 5e-6                               # the norm differs: the departure from predict_pr is pinned


def test_the_sampler_refuses_on_the_gpu_what_it_refuses_on_the_host():
    from test_gpu_generic import _sampler
    from audio_inpainting_diffusion_amd import _lib
    L, N, hop = 4096, 256, 64
    sizes = {"phase_retrieval.win_size": N, "phase_retrieval.hop_size": hop}
    F, T = N // 2 + 1, 1 + 2 * L // hop
    y = torch.zeros(2, F, T, device=DEV)
    for dc in ("always", "end"):
        smp = _sampler(L, 3, 0.25, **{"data_consistency.use": True, "data_consistency.type": dc}, **sizes)
        with pytest.raises(_lib.AidError, match="data consistency"):
            smp.predict_pr_long(y)
        assert smp.n_evals == 0
    smp = _sampler(L, 3, 0.0, **{"data_consistency.use": False}, **sizes)
    with pytest.raises(_lib.AidError, match="xi must be > 0"):
        smp.predict_pr_long(y)
    assert smp.n_evals == 0
    smp = _sampler(L, 3, 0.25, **{"data_consistency.use": False, "_rid": True}, **sizes)
    with pytest.raises(_lib.AidError, match="rid"):
        smp.predict_pr_long(y)
    assert smp.n_evals == 0
    smp = _sampler(L, 3, 0.25, **{"data_consistency.use": False}, **sizes)
    for call, why in ((lambda: smp.predict_pr_long(torch.zeros(2, F + 1, T, device=DEV)), f"F = {F}"), (lambda: smp.predict_pr_long(y, length=T * hop), "not consistent"),
                      (lambda: smp.predict_pr_long(y, seeds=[1]), "seeds"), (lambda: smp.predict_pr_long(y, max_batch=0), "max_batch"),
                      (lambda: smp.predict_pr_long(y.cpu()), "GPU only")):
        with pytest.raises(_lib.AidError, match=why):
            call()
    assert smp.n_evals == 0 and smp.y is None


# ---- reduced HIP network -----------------------------------------------------------------------------------------------------------------
def _small_net_pr():
    from test_gpu_degrade import _small_net
    smp, osmp, Ls, _ = _small_net()
    smp.args.tester.phase_retrieval.win_size, smp.args.tester.phase_retrieval.hop_size = 256, 64
    return smp, osmp, Ls


@pytest.mark.parametrize("norm", [2, "smoothl1"])
def test_hip_network_pass_a_and_pass_b_shaped_windows_vs_oracle(norm):
    """Item 0 is shaped as a window of pass A: the last 37 samples absent, the frames past the recording's last one absent and the three frames
    before those unobserved.  Item 1 as one of pass B: the first and last end' - (n_fft - 1) samples known, every frame observed.  win_size 256,
    hop_size 64, T = 3, guidance only -- predict_resample with STFTMagObserved against the oracle sampler driven with the same operator written
    as a torch lambda (magnitude sqrt(re^2 + im^2), selection with torch.where).  Ls = 4096 is a multiple of hop, so the last frame of a window
    reads the appended zeros only: where it is observed (item 1) the reference's NaN lands on the padding that torch.cat's backward drops, as in
    tests/test_gpu_phase.py::test_hip_network_predict_pr_vs_oracle; every other observed frame holds signal.  Bound: the documented 5e-4 of that
    test.
    Measured on one MI355X: rel-L2 = 4.47e-06 (norm 2) and 4.35e-06 ("smoothl1")."""
    from audio_inpainting_diffusion_amd.restore import aligned_end
    from audio_inpainting_diffusion_amd.phase_long import STFTMagObserved
    from audio_inpainting_diffusion_amd.sampler import autoregressive_overlap
    smp, osmp, Ls = _small_net_pr()
    smp.args.tester.posterior_sampling.norm = osmp.norm = norm
    N, hop = 256, 64
    F, Tw, m = N // 2 + 1, 1 + Ls // hop, N - 1
    end2 = aligned_end(Ls, int(autoregressive_overlap(smp.args) * Ls), hop)
    assert end2 >= 2 * m
    clean = _harmonic(Ls, 2, 3)
    k = torch.cat([torch.full((2, Ls), -1.0), torch.zeros(2, Tw)], dim=1)
    last = 1 + (Ls - 37) // hop                                              # the frames of a recording that ends 37 samples early
    k[0, Ls - 37:Ls] = -2
    k[0, Ls + last - 3:Ls + last] = -1
    k[0, Ls + last:] = -2
    k[1, :end2 - m] = 1
    k[1, Ls - (end2 - m):Ls] = 1
    kh, kf = k[:, :Ls], k[:, Ls:]
    assert all(bool((kf[0] == v).any()) for v in (-2, -1, 0)) and bool((kh[1] == 1).any()) and bool((kf[1] == 0).all())

    def deg(x):
        mag = _ref_stft_mag(torch.where(kh == -2, torch.zeros_like(x), x), N, hop)
        mag = torch.where((kf == 0)[:, None, :], mag, torch.zeros_like(mag))
        return torch.cat([torch.where(kh == 1, x, torch.zeros_like(x)), mag.reshape(2, -1)], dim=1)
    y = deg(clean)
    spec = y[:, Ls:].reshape(2, F, Tw)
    assert tuple(y.shape) == (2, Ls + F * Tw) and torch.equal(y[1, :Ls][kh[1] == 1], clean[1][kh[1] == 1]) and bool((y[0, :Ls] == 0).all())
    assert all(bool((spec[i][:, kf[i] == 0][:, :-1].abs().amax(dim=0) > 0).all()) for i in range(2)) and bool((spec[0][:, kf[0] != 0] == 0).all())
    smp.seeds = [7, 8]
    out = smp.predict_resample(y.to(DEV), (2, Ls), STFTMagObserved(N, hop, k.to(DEV)))
    ref = osmp.predict_resample(y, (2, Ls), deg, seeds=[7, 8])
    assert bool(torch.isfinite(ref).all())
    e = rel_l2(out.cpu(), ref)
    print(f"HIP network, STFTMagObserved windows, norm={norm}: rel-L2 vs oracle = {e:.2e}")
    assert e <= 5e-4


def test_hip_network_result_is_independent_of_the_other_recordings_and_of_max_batch():
    """Two recordings of N = 2 Ls + Ls // 3 samples (three windows each: 4 + 2 jobs), win_size 256, hop_size 64, T = 3.  Restored together, each
    alone, and with max_batch 1 against 8; form_batch is left unpinned, so the documented bound for results across batch compositions applies
    (<= 5e-6, tests/test_gpu_phase.py::test_predict_pr_batch_of_four_takes_the_sub_batch_streams).
    Measured on one MI355X: all four comparisons 0.0 (bit-equal) -- the bound stays at the documented 5e-6."""
    from audio_inpainting_diffusion_amd.phase_long import pr_plan
    from audio_inpainting_diffusion_amd.sampler import autoregressive_overlap
    smp, _, Ls = _small_net_pr()
    T, N_fft, hop = 3, 256, 64
    end = int(autoregressive_overlap(smp.args) * Ls)
    N = 2 * Ls + Ls // 3
    rec_d = _ref_stft_mag(_harmonic(N, 2, 70), N_fft, hop).to(DEV)
    A, B = pr_plan(2, N, Ls, end, N_fft, hop)
    assert len(A) == 4 and len(B) == 2
    seeds = [31, 32]
    n0 = smp.n_evals
    both = smp.predict_pr_long(rec_d, length=N, max_batch=8, seeds=seeds)
    assert smp.n_evals - n0 == 6 * (2 * T - 1) and both.shape == (2, N) and bool(torch.isfinite(both).all())
    errs = {}
    for r in range(2):
        alone = smp.predict_pr_long(rec_d[r:r + 1], length=N, max_batch=8, seeds=seeds[r:r + 1])
        errs[f"recording {r} alone"] = rel_l2(alone.cpu(), both[r:r + 1].cpu())
    one = smp.predict_pr_long(rec_d, length=N, max_batch=1, seeds=seeds)
    for r in range(2):
        errs[f"recording {r} max_batch 1"] = rel_l2(one[r:r + 1].cpu(), both[r:r + 1].cpu())
    print("pr_long batch invariance, rel-L2:", {k: "%.2e" % v for k, v in errs.items()})
    assert all(e <= 5e-6 for e in errs.values()), errs
