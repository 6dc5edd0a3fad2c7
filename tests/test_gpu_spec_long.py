"""GPU tests of spectrogram inpainting of whole recordings (csrc/aid_spec_long.hip, spec_long.py,
Sampler.predict_spectrogram_inpainting_long): the window operator in its three modes against the float64 formula of
tests/test_spec_long_host.py and bit for bit against SpectralMask, the gather bit-exact against Python indexing, the two passes stitched
around a stub sampler, one window against predict_spectrogram_inpainting, and the reduced HIP network against the oracle and across batch
compositions.  Reduced-size models only."""
import math

import pytest
import torch

from conftest import rel_l2
from test_gpu_bwe_long import SENT, _on_device
from test_gpu_phase import _harmonic
from test_spec_long_host import rec_operator64, rect_mask, window_apply64, window_project64

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- the operator ------------------------------------------------------------------------------------------------------------------------
# (n_fft, hop, L, end, N0, r): N0 a multiple of n_fft, r > n_fft / 2 -- the recordings of N0 and N0 + r samples share Np, have four windows
# each and a last window that the recording ends in
OP_CASES = [(64, 16, 1000, 260, 3008, 40), (128, 32, 1500, 520, 3840, 100), (64, 16, 1024, 260, 3008, 40)]


def _four_windows(n_fft, hop, L, end, N0, r):
    """[(recording, window, N)] x 4: a first window (s = 0: left reflection), an interior pass-B window (known head and tail), a last window
    with N - s < L and N % n_fft > half (the reflection about Np reads signal), a last window with N % n_fft == 0; and the states"""
    from audio_inpainting_diffusion_amd.spec_long import padded_length, spec_windows, window_state
    N1 = N0 + r
    w1, w0 = spec_windows(N1, L, end, n_fft, hop), spec_windows(N0, L, end, n_fft, hop)
    assert len(w1) == len(w0) == 4 and padded_length(N1, n_fft) == padded_length(N0, n_fft) and N0 % n_fft == 0 and N1 % n_fft > n_fft // 2
    items = [(0, w1[0], N1), (1, w1[1], N1), (0, w1[3], N1), (1, w0[3], N0)]
    assert items[0][1][0] == 0 and items[1][1][1] > 0 and items[1][1][2] > 0 and all(N - w[0] < L for _, w, N in items[2:])
    states = torch.stack([torch.from_numpy(window_state(N, L, n_fft, hop, w[0], w[1], w[2])) for _, w, N in items])
    assert all(bool((states == v).any()) for v in (-2.0, -1.0, 0.0, 1.0))
    return items, states, padded_length(N1, n_fft)


def _strided_mask(Rm, F, T, seed):
    """host mask [Rm, F, T] of zeros and ones, and its copy on the device as a view into [Rm, F + 1, T + 3] (bin stride T + 3, first element
    misaligned)"""
    m = (torch.rand(Rm, F, T, generator=torch.Generator().manual_seed(seed)) > 0.3).float()
    buf = torch.full((Rm, F + 1, T + 3), SENT, device=DEV)
    view = buf[:, :F, 1:T + 1]
    view.copy_(m)
    return m, view


@pytest.mark.parametrize("n_fft,hop,L,end,N0,r", OP_CASES)
@pytest.mark.parametrize("per_item", [False, True])
def test_stft_mask_observed_modes_against_float64_on_strided_misaligned_rows(n_fft, hop, L, end, N0, r, per_item):
    """apply, adjoint and project within rel-L2 2e-6 of the float64 formula (adjoint: its autograd VJP) -- the bound tests/test_gpu_spectral.py
    holds SpectralMask to -- on four window shapes in one batch; <A x, g> = <x, A^T g> on the device results to 1e-5; what the state selects is
    exact; the scratch of a frame that is not computable is never read (it holds NaN); nothing outside the rows is written.
    Measured on one MI355X over the three shapes, both mask forms: apply <= 8.9e-08, adjoint <= 8.8e-08, project <= 7.4e-08."""
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.spec_long import spec_tables, window_frames
    items, states, Np = _four_windows(n_fft, hop, L, end, N0, r)
    B, F, T_rec, Tw = 4, n_fft // 2 + 1, 1 + Np // hop, window_frames(L, n_fft, hop)
    Rm = 2 if per_item else 1
    mask, mask_d = _strided_mask(Rm, F, T_rec, 7 + n_fft)
    gen = torch.Generator().manual_seed(L + n_fft)
    x, g, y = (torch.randn(B, L, generator=gen) for _ in range(3))
    window, inv_env, twiddle = spec_tables(N0, n_fft, hop, None, DEV)
    assert inv_env.numel() == Np
    (_, xd), (_, gd), (_, yd), (_, kd) = (_on_device(t, 1) for t in (x, g, y, states))
    it_d = torch.tensor([(rr, w[0], N) for rr, w, N in items], dtype=torch.int64, device=DEV)
    frames = torch.full((B, Tw, n_fft), float("nan"), device=DEV)
    kh = states[:, :L]

    def run(mode, inp):
        buf = torch.full((B, L + 3), SENT, device=DEV)
        _lib.call("aid_stft_mask_observed", _lib.StftMaskObservedParams(
            inp.data_ptr(), yd.data_ptr() if mode == 2 else None, kd.data_ptr(), it_d.data_ptr(), window.data_ptr(), twiddle.data_ptr(), inv_env.data_ptr(),
            mask_d.data_ptr(), frames.data_ptr(), buf[:, 2:].data_ptr(), L, Np, L + 3, L + 3, states.shape[1] + 3, L + 3,
            mask_d.stride(0) if per_item else 0, mask_d.stride(1), B, Rm, n_fft, hop, Tw, mode))
        torch.cuda.synchronize()
        assert bool((buf[:, :2] == SENT).all()) and bool((buf[:, L + 2:] == SENT).all())
        return buf[:, 2:L + 2].cpu()

    got, adj, prj = run(0, xd), run(1, gd), run(2, xd)
    assert all(bool(torch.isfinite(t).all()) for t in (got, adj, prj))
    assert bool(torch.isnan(frames).any())                                        # (some frame was not computable, and stayed unwritten)
    m64 = mask.double()
    xt = x.double().requires_grad_()
    ref = torch.stack([window_apply64(xt[b], states[b], w[0], N, m64[rr if per_item else 0], n_fft, hop) for b, (rr, w, N) in enumerate(items)])
    (ref * g.double()).sum().backward()
    prj_ref = torch.stack([window_project64(x[b].double(), y[b].double(), states[b], w[0], N, m64[rr if per_item else 0], n_fft, hop)
                           for b, (rr, w, N) in enumerate(items)])
    e = (rel_l2(got, ref.detach()), rel_l2(adj, xt.grad), rel_l2(prj, prj_ref))
    print((n_fft, hop, L, per_item), "apply %.2e adjoint %.2e project %.2e" % e)
    assert max(e) <= 2e-6
    # selections are exact
    assert torch.equal(got[kh > 0], x[kh > 0]) and bool((got[kh < 0] == 0).all()) and bool((got[kh == 0] != 0).any())
    assert bool((adj[kh <= -2] == 0).all()) and torch.equal(prj[kh > 0], y[kh > 0]) and torch.equal(prj[kh < 0], x[kh < 0])
    # <A x, g> == <x, A^T g> on the device results themselves (absent samples do not enter A: leave them out of x)
    xa = torch.where(kh <= -2, torch.zeros_like(x), x)
    lhs, rhs = float((got.double() * g.double()).sum()), float((xa.double() * adj.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), 1.0)
    # the launcher refuses what it can see
    out0 = torch.zeros(B, L, device=DEV)
    for bad in (dict(mode=3), dict(B=0), dict(B=65536), dict(Tw=Tw + 1), dict(Np=Np + hop), dict(hop=hop + 1), dict(n_fft=n_fft + 2), dict(x_ld=L - 1),
                dict(state_ld=L + Tw - 1), dict(mask_ld=T_rec - 1), dict(Rm=0), dict(mode=2)):
        kw = dict(mode=0, B=B, Tw=Tw, Np=Np, hop=hop, n_fft=n_fft, x_ld=L + 3, state_ld=states.shape[1] + 3, mask_ld=mask_d.stride(1), Rm=Rm)
        kw.update(bad)
        with pytest.raises(_lib.AidError):
            _lib.call("aid_stft_mask_observed", _lib.StftMaskObservedParams(
                xd.data_ptr(), None, kd.data_ptr(), it_d.data_ptr(), window.data_ptr(), twiddle.data_ptr(), inv_env.data_ptr(), mask_d.data_ptr(),
                frames.data_ptr(), out0.data_ptr(), L, kw["Np"], kw["x_ld"], L, kw["state_ld"], L, 0, kw["mask_ld"], kw["B"], kw["Rm"], kw["n_fft"], kw["hop"],
                kw["Tw"], kw["mode"]))
    assert bool((out0 == 0).all())


def test_an_item_the_kernels_cannot_trust_runs_no_frame_and_reads_nothing_of_the_recording():
    """items are device memory: a start off the hop grid, a start past the recording, a length that does not fit Np and a recording without a
    mask give c = a = 0 under the selects, with every frame scratch left unwritten"""
    from audio_inpainting_diffusion_amd.spec_long import SpectralMaskObserved, spec_tables, window_frames, window_state
    n_fft, hop, L, N = 64, 16, 1000, 3048
    Np, Tw = 3072, window_frames(L, n_fft, hop)
    mask = torch.ones(2, n_fft // 2 + 1, 1 + Np // hop, device=DEV)
    st = torch.from_numpy(window_state(N, L, n_fft, hop, 736, 0, 0))
    bad = [(0, 737, N), (0, N + 16, N), (0, 736, Np), (0, 736, Np - n_fft - 1), (2, 736, N), (-1, 736, N), (0, -16, N)]
    state = st[None, :].repeat(len(bad), 1).to(DEV)
    op = SpectralMaskObserved(mask, n_fft, hop, state, torch.tensor(bad, dtype=torch.int64, device=DEV), spec_tables(N, n_fft, hop, None, DEV))
    x, y = (torch.randn(len(bad), L, generator=torch.Generator().manual_seed(1)).to(DEV) for _ in range(2))
    kh = state[:, :L]
    op._frames[(len(bad), torch.cuda.current_stream().cuda_stream)] = fr = torch.full((len(bad), Tw, n_fft), float("nan"), device=DEV)
    assert bool((op.apply(x) == 0).all()) and bool((op.adjoint(x) == 0).all())
    assert torch.equal(op.project(x, y), torch.where(kh == 0, y + x, x))
    assert bool(torch.isnan(fr).all())


@pytest.mark.parametrize("L,n_fft,hop", [(1000, 64, 16), (4096, 256, 64)])
@pytest.mark.parametrize("per_item", [False, True])
def test_with_one_window_and_every_sample_observed_the_three_modes_are_spectral_mask_bit_for_bit(L, n_fft, hop, per_item):
    from audio_inpainting_diffusion_amd.spec_long import SpectralMaskObserved, rec_frames, spec_tables, window_state
    from audio_inpainting_diffusion_amd.stft import SpectralMask
    B = 3
    T_rec = rec_frames(L, n_fft, hop)
    gen = torch.Generator().manual_seed(31 + L)
    mask = (torch.rand((B if per_item else 1, n_fft // 2 + 1, T_rec), generator=gen) > 0.3).float().to(DEV)
    x, g, y = ((torch.randn(B, L, generator=gen)).to(DEV) for _ in range(3))
    st = torch.from_numpy(window_state(L, L, n_fft, hop, 0, 0, 0))
    assert bool((st[:L] == 0).all()) and bool((st[L:L + T_rec] == 0).all()) and bool((st[L + T_rec:] == -2).all())
    items = torch.tensor([(b, 0, L) for b in range(B)], dtype=torch.int64, device=DEV)
    op = SpectralMaskObserved(mask, n_fft, hop, st[None, :].repeat(B, 1).to(DEV), items, spec_tables(L, n_fft, hop, None, DEV))
    ref = SpectralMask(mask if per_item else mask[0], L, n_fft, hop, n_fft, device=DEV)
    assert torch.equal(op.inv_env, ref.inv_env) and torch.equal(op.window, ref.window)
    want = ref.apply(x)
    assert torch.equal(op.apply(x), want) and bool((want != x).any())
    assert torch.equal(op.adjoint(g), ref.adjoint(g))
    assert torch.equal(op.project(x, y), ref.project(x, y))


def test_rows_are_the_slices_of_the_whole_batch_and_two_streams_keep_their_own_frame_scratch():
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.spec_long import SpectralMaskObserved, spec_tables
    n_fft, hop, L, end, N0, r = OP_CASES[0]
    items, states, Np = _four_windows(n_fft, hop, L, end, N0, r)
    B = 4
    mask, _ = _strided_mask(2, n_fft // 2 + 1, 1 + Np // hop, 3)
    mask = mask.to(DEV)
    it_d = torch.tensor([(rr, w[0], N) for rr, w, N in items], dtype=torch.int64, device=DEV)
    tables = spec_tables(N0, n_fft, hop, None, DEV)
    op = SpectralMaskObserved(mask, n_fft, hop, states.to(DEV), it_d, tables)
    assert op.shared_mask is False and (op.L, op.Tw, op.Np) == (L, 1 + (L + n_fft) // hop, Np)
    gen = torch.Generator().manual_seed(5)
    xa, xb, g, y = (torch.randn(B, L, generator=gen).to(DEV) for _ in range(4))
    ax, bx, atg, pa = op.apply(xa), op.apply(xb), op.adjoint(g), op.project(xa, y)
    lo_op, hi_op = op.rows(0, 2), op.rows(2, 4)
    assert op.rows(0, 2) is lo_op and lo_op.state.shape[0] == 2 and lo_op.window is op.window and lo_op.mask is op.mask
    assert hi_op.state.data_ptr() == op.state[2:].data_ptr() and hi_op.items.data_ptr() == it_d[2:].data_ptr()
    for lo, hi in ((1, 1), (-1, 1), (0, B + 1)):
        with pytest.raises(_lib.AidError):
            op.rows(lo, hi)
    with pytest.raises(_lib.AidError):
        op.apply(xa[:3])
    assert torch.equal(lo_op.apply(xa[:2]), ax[:2]) and torch.equal(hi_op.adjoint(g[2:]), atg[2:]) and torch.equal(hi_op.project(xa[2:], y[2:]), pa[2:])
    # two sub-operators on two streams, interleaved; then ONE operator on two streams
    cur, s1, s2 = torch.cuda.current_stream(), torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(cur)
    s2.wait_stream(cur)
    for _ in range(2):
        with torch.cuda.stream(s1):
            a1 = lo_op.apply(xa[:2])
            c1 = op.apply(xa)
        with torch.cuda.stream(s2):
            a2 = hi_op.apply(xb[2:])
            c2 = op.apply(xb)
        with torch.cuda.stream(s1):
            g1 = lo_op.adjoint(g[:2])
        with torch.cuda.stream(s2):
            g2 = hi_op.adjoint(g[2:])
    cur.wait_stream(s1)
    cur.wait_stream(s2)
    torch.cuda.synchronize()
    assert torch.equal(a1, ax[:2]) and torch.equal(a2, bx[2:]) and torch.equal(g1, atg[:2]) and torch.equal(g2, atg[2:])
    assert torch.equal(c1, ax) and torch.equal(c2, bx)
    assert len(op._frames) == 3 and len({f.data_ptr() for f in op._frames.values()}) == 3          # (the current stream and the two others)
    assert len(lo_op._frames) == 2 and len(hi_op._frames) == 2


# ---- the gather --------------------------------------------------------------------------------------------------------------------------
# (N, L, end, n_fft, hop): the host cases with more than one window, and recordings that end just past half a block and on a block
GATHER_CASES = [(5000, 1200, 300, 64, 16), (3777, 1000, 260, 64, 16), (3999, 1000, 257, 64, 32), (3041, 1000, 260, 64, 16), (3008, 1000, 260, 64, 16)]


def _gather_ref(rec, out, N, L, n_fft, hop, job):
    from audio_inpainting_diffusion_amd.spec_long import window_state
    r, s, head, tail, lo, hi = job
    k = torch.from_numpy(window_state(N, L, n_fft, hop, s, head, tail))
    qc = (s + torch.arange(L)).clamp(max=N - 1)
    y = torch.where(k[:L] == 1, out[r, qc], torch.where(k[:L] == 0, rec[r, qc], torch.zeros(L)))
    return y, k, torch.tensor([r, s, N])


def _all_windows(R, N, L, end, n_fft, hop):
    from audio_inpainting_diffusion_amd.spec_long import spec_windows
    wins = spec_windows(N, L, end, n_fft, hop)
    return [(r,) + w for r in range(R) for w in wins[0::2]], [(r,) + w for r in range(R) for w in wins[1::2]]


@pytest.mark.parametrize("N,L,end,n_fft,hop", GATHER_CASES)
def test_spec_gather_is_bit_exact_against_python_indexing_and_the_host_states(N, L, end, n_fft, hop):
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.restore import job_table
    from audio_inpainting_diffusion_amd.spec_long import padded_length, spec_gather, window_frames
    R, Tw, Np = 3, window_frames(L, n_fft, hop), padded_length(N, n_fft)
    A, B = _all_windows(R, N, L, end, n_fft, hop)
    assert A and B
    gen = torch.Generator().manual_seed(2 + N)
    rec, out = torch.randn(R, N, generator=gen), torch.randn(R, N, generator=gen)
    rec_d = torch.empty(R, N + 5, device=DEV)[:, 2:N + 2].copy_(rec)
    out_d = torch.empty(R, N + 3, device=DEV)[:, 1:N + 1].copy_(out)           # (its rows start at an odd element)
    # skipped jobs: a start off the hop grid, a recording and a start out of range
    bad_jobs = [(0, A[1][1] + 1, 0, 0, 0, L), (R, 0, 0, 0, 0, L), (0, N + (-N % hop), 0, 0, 0, L), (-1, 0, 0, 0, 0, L)]
    assert bad_jobs[0][1] % hop and bad_jobs[0][1] < N
    for jobs in (A, B, A + bad_jobs[:1] + B + bad_jobs[1:]):
        y, k, it = spec_gather(rec_d, out_d, job_table(jobs, DEV), L, n_fft, hop)
        assert y.shape == (len(jobs), L) and k.shape == (len(jobs), L + Tw) and it.shape == (len(jobs), 3) and it.dtype == torch.int64
        for j, job in enumerate(jobs):
            if job in bad_jobs:
                assert bool((y[j] == 0).all()) and bool((k[j] == -2).all()) and it[j].tolist() == [-1, -1, 0], j
                continue
            y_ref, k_ref, it_ref = _gather_ref(rec, out, N, L, n_fft, hop, job)
            assert torch.equal(k[j].cpu(), k_ref) and torch.equal(y[j].cpu(), y_ref) and torch.equal(it[j].cpu(), it_ref), j
        if jobs is A:
            assert not bool((k[:, :L] == 1).any()) and bool((k[:, :L] == 0).any()) and bool((k[:, :L] == -1).any()) and bool((k[:, L:] == -1).any())
        elif jobs is B:
            assert bool((k[:, :L] == 1).any())
    # zero jobs: nothing is launched, empty results
    y, k, it = spec_gather(rec_d, out_d, job_table([], DEV), L, n_fft, hop)
    assert y.shape == (0, L) and k.shape == (0, L + Tw) and it.shape == (0, 3)
    # guarded outputs: nothing before or after the rows is written
    tab = job_table(A + bad_jobs, DEV)
    J, pad = tab.shape[0], 64
    bufs = [torch.full((pad + J * n + pad,), SENT, device=DEV) for n in (L, L + Tw)]
    itb = torch.full((8 + J * 3 + 8,), -77, dtype=torch.int64, device=DEV)
    _lib.call("aid_spec_gather", _lib.SpecGatherParams(rec_d.data_ptr(), out_d.data_ptr(), bufs[0][pad:].data_ptr(), bufs[1][pad:].data_ptr(), itb[8:].data_ptr(),
                                                       tab.data_ptr(), L, N, Np, N + 5, N + 3, J, R, n_fft, hop, Tw))
    assert all(bool((b[:pad] == SENT).all()) and bool((b[-pad:] == SENT).all()) and not bool((b[pad:-pad] == SENT).any()) for b in bufs)
    assert bool((itb[:8] == -77).all()) and bool((itb[-8:] == -77).all()) and not bool((itb[8:-8] == -77).any())
    y0 = torch.zeros(len(A), L + Tw, device=DEV)
    i0 = torch.zeros(len(A), 3, dtype=torch.int64, device=DEV)
    for bad in (dict(rec_ld=N - 1), dict(out_ld=N - 1), dict(J=0), dict(J=65536), dict(Tw=Tw + 1), dict(Np=Np + n_fft), dict(n_fft=n_fft + 2), dict(hop=0),
                dict(hop=hop + 1), dict(R=0)):
        kw = dict(J=len(A), R=R, Tw=Tw, Np=Np, rec_ld=N + 5, out_ld=N + 3, n_fft=n_fft, hop=hop)
        kw.update(bad)
        with pytest.raises(_lib.AidError):
            _lib.call("aid_spec_gather", _lib.SpecGatherParams(rec_d.data_ptr(), out_d.data_ptr(), y0.data_ptr(), y0.data_ptr(), i0.data_ptr(), tab.data_ptr(),
                                                               L, N, kw["Np"], kw["rec_ld"], kw["out_ld"], kw["J"], kw["R"], kw["n_fft"], kw["hop"], kw["Tw"]))
    assert bool((y0 == 0).all()) and bool((i0 == 0).all())


# ---- the two passes around a stub sampler ------------------------------------------------------------------------------------------------
class _Stub:
    """predict_resample(y, shape, op)[j, i] = w_j * L + i + r_j / 4, with (r_j, w_j) read from the job's seed (r_j + 1) * 65536 + w_j: every sample
    names the window it was written from."""

    def __init__(self):
        self.calls, self.seeds = [], "untouched"

    def predict_resample(self, y, shape, op):
        B, L = shape
        assert y.shape == (B, L) and op.state.shape == (B, L + op.Tw) and op.items.shape == (B, 3) and op.L == L and op.shared_mask is False
        self.calls.append((y.clone(), op.state.clone(), op.items.clone(), (op.N, op.hop, op.mask.shape[0]), self.seeds))
        base = torch.tensor([(s % 65536) * L + (s // 65536 - 1) / 4 for s in self.seeds], dtype=torch.float32, device=y.device)
        return base[:, None] + torch.arange(L, dtype=torch.float32, device=y.device)[None, :]


@pytest.mark.parametrize("N,L,end,n_fft,hop", GATHER_CASES[:3])
@pytest.mark.parametrize("max_batch", [2, 8])
def test_two_passes_stitch_the_stub_sampler_output_and_leave_the_rest_of_the_recording(N, L, end, n_fft, hop, max_batch):
    """Recording 0 has a rectangle over the border of windows 1 and 2 (a job in each pass), recording 1 one inside window 0, recording 2 none.
    Every owned sample of a job comes from its window; every other sample stays y."""
    from audio_inpainting_diffusion_amd.restore import aligned_end
    from audio_inpainting_diffusion_amd.spec_long import rec_frames, spec_passes, spec_plan, spec_windows, touched_frames
    R, T_rec = 3, rec_frames(N, n_fft, hop)
    end2 = aligned_end(L, end, hop)
    step, m = L - end2, 2 * (n_fft - 1)
    wins = spec_windows(N, L, end, n_fft, hop)
    border = (wins[1][0] + wins[1][4]) // hop                                 # the frame centred where window 1's owned range ends
    mask = torch.stack([rect_mask(N, n_fft, hop, border - 2, border + 3), rect_mask(N, n_fft, hop, 10, 14), rect_mask(N, n_fft, hop, 0, 0)])
    A, B = spec_plan(touched_frames(mask), R, N, L, end, n_fft, hop)
    assert A == [(0,) + wins[2], (1,) + wins[0]] and B == [(0,) + wins[1]]
    y = torch.randn(R, N, generator=torch.Generator().manual_seed(11 + N))
    y_d = torch.empty(R, N + 3, device=DEV)[:, 1:N + 1].copy_(y)
    stub, seeds = _Stub(), [1, 2, 3]
    out = spec_passes(stub, y_d, mask.to(DEV), n_fft, hop, L, end, max_batch=max_batch, seeds=seeds)
    assert out.is_cuda and out.shape == (R, N) and stub.seeds == "untouched"
    want, refs = y.clone(), []
    for jobs in (A, B):
        refs += [_gather_ref(y, want.clone(), N, L, n_fft, hop, job) for job in jobs]       # (pass B gathers what pass A scattered)
        for r, s, head, tail, lo, hi in jobs:
            want[r, s + lo:s + hi] = (s // step) * L + torch.arange(lo, hi) + r / 4
    assert torch.equal(out.cpu(), want) and torch.equal(out[2].cpu(), y[2])
    nA, nB = math.ceil(len(A) / max_batch), math.ceil(len(B) / max_batch)
    assert len(stub.calls) == nA + nB and all(call[0].shape[0] <= max_batch for call in stub.calls)
    assert [s for call in stub.calls for s in call[4]] == [seeds[r] * 65536 + s // step for r, s, *_ in A + B]
    assert all(call[3] == (n_fft, hop, R) for call in stub.calls)
    ys, ks, its = (torch.cat([call[i] for call in stub.calls]).cpu() for i in range(3))
    for j, (job, (y_ref, k_ref, it_ref)) in enumerate(zip(A + B, refs)):
        assert torch.equal(ks[j], k_ref) and torch.equal(ys[j], y_ref) and torch.equal(its[j], it_ref), j
    head = B[0][2]
    assert head == end2 - m and bool((ks[2, :head] == 1).all()) and torch.equal(ys[2, :head], y[0, B[0][1]:B[0][1] + head])   # (window 0 of recording 0 was no job: y)
    assert torch.equal(ys[2, L - head:], want[0, B[0][1] + L - head:B[0][1] + L]) and bool((ys[2, L - head:] >= 2 * L).all())     # (window 2 was: pass A's samples)

    # an all-ones mask: no job, no call, the output is y; one mask for all recordings repeats its jobs; no seeds: the global generator
    class _Plain(_Stub):
        def predict_resample(self, y, shape, op):
            self.calls.append((self.seeds, op.mask.shape[0]))
            return y + 1
    plain = _Plain()
    same = spec_passes(plain, y_d, torch.ones(n_fft // 2 + 1, T_rec), n_fft, hop, L, end, max_batch=max_batch)
    assert plain.calls == [] and torch.equal(same.cpu(), y) and same.data_ptr() != y_d.data_ptr()
    spec_passes(plain, y_d, mask[1], n_fft, hop, L, end, max_batch=max_batch)
    assert sum(1 for c in plain.calls) == math.ceil(R / max_batch) and all(c == (None, 1) for c in plain.calls) and plain.seeds == "untouched"


# ---- reduced HIP network -----------------------------------------------------------------------------------------------------------------
NF, HOP = 128, 32


def _small_net_spec(dc=None):
    from test_gpu_degrade import _small_net
    smp, osmp, Ls, _ = _small_net(dc=dc is not None)
    st = smp.args.tester.spectrogram_inpainting.stft
    st.n_fft, st.hop_length, st.win_length = NF, HOP, NF
    if dc is not None:
        smp.args.tester.data_consistency.type = dc
        smp.data_consistency, smp.data_consistency_end = dc == "always", dc == "end"
        osmp.data_consistency, osmp.data_consistency_end = dc == "always", dc == "end"
    return smp, osmp, Ls


@pytest.mark.parametrize("dc", [None, "always", "end"])
def test_one_window_is_predict_spectrogram_inpainting(dc):
    """R = 1, N = L = 4096, n_fft 128, hop 32, T = 3: one job, every sample observed, the same frame terms in the same order as SpectralMask's;
    bound 5e-6 rel-L2 (the documented bound across batch compositions).
    Measured on one MI355X: 0.0, torch.equal, for guidance only, "always" and "end" -- the bound stays."""
    from audio_inpainting_diffusion_amd.spec_long import rec_frames
    from oracle.sampler import spectral_mask_apply
    smp, _, L = _small_net_spec(dc)
    seed = 23
    mask = rect_mask(L, NF, HOP, 40, 70, 5, 30)
    assert mask.shape[1] == rec_frames(L, NF, HOP)
    y = spectral_mask_apply(_harmonic(L, 1, 4), mask, NF, HOP, NF).to(DEV)
    smp.seeds = [99]
    n0 = smp.n_evals
    out = smp.predict_spectrogram_inpainting_long(y, mask.to(DEV), seeds=[seed])
    assert smp.n_evals - n0 == 2 * smp.nb_steps - 1 and smp.seeds == [99] and out.is_cuda and out.shape == (1, L)
    smp.seeds = [seed * 65536]
    ref = smp.predict_spectrogram_inpainting(y, mask.to(DEV))
    e = rel_l2(out.cpu(), ref.cpu())
    print(f"one window, dc={dc}: predict_spectrogram_inpainting_long vs predict_spectrogram_inpainting rel-L2 = {e:.2e}, bit-equal: {torch.equal(out, ref)}")
    assert e <= 5e-6 and not torch.equal(out, y)


@pytest.mark.parametrize("dc", [None, "always"])
def test_hip_network_pass_a_and_pass_b_shaped_windows_vs_oracle(dc):
    """A recording of N = 2 Ls + Ls // 3 samples (Ls = 4096, n_fft 128, hop 32, T = 3) with a rectangle of masked bins in window 2 and one in
    window 1.  Item 0 is window 2 as pass A sees it (the last window: absent samples, unobserved samples at its start, frames that are not
    computable), item 1 is window 1 as pass B sees it (known head and tail, taken here from the clean recording).  predict_resample through
    SpectralMaskObserved against the oracle sampler driven with the same operator written as a torch lambda (the float64 formula of
    tests/test_spec_long_host.py), guidance only and with the projection at every evaluation.  Bound: the documented 5e-4 of the sibling tests.
    Measured on one MI355X: rel-L2 = 5.05e-06 (guidance only) and 2.66e-06 ("always")."""
    from audio_inpainting_diffusion_amd.restore import job_table
    from audio_inpainting_diffusion_amd.sampler import autoregressive_overlap
    from audio_inpainting_diffusion_amd.spec_long import SpectralMaskObserved, spec_gather, spec_tables, spec_windows
    smp, osmp, Ls = _small_net_spec(dc)
    N = 2 * Ls + Ls // 3
    end = int(autoregressive_overlap(smp.args) * Ls)
    wins = spec_windows(N, Ls, end, NF, HOP)
    assert len(wins) == 3
    mask = rect_mask(N, NF, HOP, (wins[2][0] + 1500) // HOP, (wins[2][0] + 2600) // HOP, 5, 30)
    mask[10:40, (wins[1][0] + 1800) // HOP:(wins[1][0] + 2400) // HOP] = 0
    clean = _harmonic(N, 1, 3)
    y_rec = rec_operator64(clean[0].double(), mask.double(), NF, HOP).float()[None, :]
    jobs = [(0,) + wins[2], (0,) + wins[1]]
    yw, kw, iw = spec_gather(y_rec.to(DEV), clean.to(DEV), job_table(jobs, DEV), Ls, NF, HOP)
    k = kw.cpu()
    kh = k[:, :Ls]
    assert all(bool((kh[0] == v).any()) for v in (-2, -1, 0)) and not bool((kh[0] == 1).any()) and bool((k[0, Ls:] == -1).any())
    assert all(bool((kh[1] == v).any()) for v in (1, 0)) and bool((k[1, Ls:] == -1).any())
    m64 = mask.double()

    def deg(x):
        return torch.stack([window_apply64(x[b].double(), k[b], jobs[b][1], N, m64, NF, HOP) for b in range(2)]).to(x.dtype)
    y = yw.cpu()
    osmp.y, osmp.degradation, osmp._shape = y, deg, (2, Ls)
    osmp.project = lambda x: torch.stack([window_project64(x[b].double(), y[b].double(), k[b], jobs[b][1], N, m64, NF, HOP) for b in range(2)]).to(x.dtype)
    ref = osmp._predict([7, 8], False, shape=(2, Ls))
    smp.seeds = [7, 8]
    out = smp.predict_resample(yw, (2, Ls), SpectralMaskObserved(mask.to(DEV)[None], NF, HOP, kw, iw, spec_tables(N, NF, HOP, None, DEV)))
    assert bool(torch.isfinite(ref).all())
    e = rel_l2(out.cpu(), ref)
    print(f"HIP network, SpectralMaskObserved windows, dc={dc}: rel-L2 vs oracle = {e:.2e}")
    assert e <= 5e-4


def test_hip_network_result_is_independent_of_the_other_recordings_and_of_max_batch():
    """Two recordings of N = 2 Ls + Ls // 3 samples (three windows each) under one mask whose rectangle lies across the border of windows 0 and
    1 and another inside window 2: 4 + 2 jobs, n_fft 128, hop 32, T = 3, data consistency "always".  Restored together, each alone, and with
    max_batch 1 against 8; the documented bound for results across batch compositions applies (<= 5e-6).
    Measured on one MI355X: all four comparisons 0.0 (bit-equal) -- the bound stays at the documented 5e-6."""
    from audio_inpainting_diffusion_amd.sampler import autoregressive_overlap
    from audio_inpainting_diffusion_amd.spec_long import spec_plan, spec_windows, touched_frames
    smp, _, Ls = _small_net_spec("always")
    T = smp.nb_steps
    end = int(autoregressive_overlap(smp.args) * Ls)
    N = 2 * Ls + Ls // 3
    wins = spec_windows(N, Ls, end, NF, HOP)
    border = (wins[0][0] + wins[0][4]) // HOP
    mask = rect_mask(N, NF, HOP, border - 6, border + 6, 5, 30)
    mask[10:40, (wins[2][0] + 1500) // HOP:(wins[2][0] + 1900) // HOP] = 0
    A, B = spec_plan(touched_frames(mask), 2, N, Ls, end, NF, HOP)
    assert len(A) == 4 and len(B) == 2
    clean = _harmonic(N, 2, 70)
    y = torch.stack([rec_operator64(clean[r].double(), mask.double(), NF, HOP).float() for r in range(2)]).to(DEV)
    mask_d = mask.to(DEV)
    seeds = [31, 32]
    n0 = smp.n_evals
    both = smp.predict_spectrogram_inpainting_long(y, mask_d, max_batch=8, seeds=seeds)
    assert smp.n_evals - n0 == 6 * (2 * T - 1) and both.shape == (2, N) and bool(torch.isfinite(both).all())
    assert not torch.equal(both, y)
    errs = {}
    for r in range(2):
        alone = smp.predict_spectrogram_inpainting_long(y[r:r + 1], mask_d, max_batch=8, seeds=seeds[r:r + 1])
        errs[f"recording {r} alone"] = rel_l2(alone.cpu(), both[r:r + 1].cpu())
    one = smp.predict_spectrogram_inpainting_long(y, mask_d[None].expand(2, -1, -1), max_batch=1, seeds=seeds)
    for r in range(2):
        errs[f"recording {r} max_batch 1"] = rel_l2(one[r:r + 1].cpu(), both[r:r + 1].cpu())
    print("spec_long batch invariance, rel-L2:", {k: "%.2e" % v for k, v in errs.items()})
    assert max(errs.values()) <= 5e-6


def test_the_sampler_refuses_on_the_gpu_what_it_refuses_on_the_host():
    from test_gpu_generic import _sampler
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.spec_long import rec_frames
    L = 4096
    sizes = {"spectrogram_inpainting.stft.n_fft": NF, "spectrogram_inpainting.stft.hop_length": HOP, "spectrogram_inpainting.stft.win_length": NF}
    F, N = NF // 2 + 1, 2 * L
    y, mask = torch.zeros(2, N, device=DEV), torch.ones(F, rec_frames(N, NF, HOP), device=DEV)
    smp = _sampler(L, 3, 0.25, **{"data_consistency.use": False, "_rid": True}, **sizes)
    with pytest.raises(_lib.AidError, match="rid"):
        smp.predict_spectrogram_inpainting_long(y, mask)
    smp = _sampler(L, 3, 0.25, **{"data_consistency.use": False, "spectrogram_inpainting.stft.window": "hamming"}, **sizes)
    with pytest.raises(NotImplementedError, match="hann"):
        smp.predict_spectrogram_inpainting_long(y, mask)
    smp = _sampler(L, 3, 0.25, **{"data_consistency.use": False}, **sizes)
    call = smp.predict_spectrogram_inpainting_long
    for fn, why in ((lambda: call(y, mask[:, :-1]), "must be"), (lambda: call(y, mask, seeds=[1]), "seeds"), (lambda: call(y, mask, max_batch=0), "max_batch"),
                    (lambda: call(y.cpu(), mask), "GPU only"), (lambda: call(y[:, ::2], mask), "float32 recordings")):
        with pytest.raises(_lib.AidError, match=why):
            fn()
    assert smp.n_evals == 0 and smp.y is None and smp.spectral is None
    assert torch.equal(call(y, mask), y) and smp.n_evals == 0                           # nothing masked: nothing to do
