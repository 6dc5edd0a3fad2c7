"""CPU tests (no GPU) of spectrogram inpainting of whole recordings (spec_long.py, include/aid_spec_long.h,
Sampler.predict_spectrogram_inpainting_long, harness.spectrogram_inpainting_long): the computable-frame
rule and the sample states against brute force, the hop-aligned grid and its ownership, the exactness of the computable frames and of the
state-0 samples of a window in float64, the job rule, the seed rule, and the refusals, all raised before anything touches a GPU.

The float64 reference of the recording's operator (``rec_operator64``) and of the window's (``window_c64``, ``window_apply64``) is the formula
of include/aid_spec_long.h written with torch, so autograd gives the exact VJP; tests/test_gpu_spec_long.py imports them."""

import numpy as np
import pytest
import torch


# (N, L, end, n_fft, hop)
SPEC_CASES = [(5000, 1200, 300, 64, 16), (3777, 1000, 260, 64, 16), (2048, 1024, 260, 64, 16), (4000, 1100, 150, 32, 8), (900, 1000, 300, 64, 16),
              (3999, 1000, 257, 64, 32)]
# N % n_fft in {0, 1, half, half + 1, n_fft - 1} at n_fft 64, hop 16
TAIL_CASES = [(3008 + r, 1000, 260, 64, 16) for r in (0, 1, 32, 33, 63)]


# ---- the float64 reference -----------------------------------------------------------------------------------------------------------
def hann64(n_fft):
    """the periodic Hann window rounded to fp32, as float64 (what the kernels multiply with)"""
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
    return torch.from_numpy(w.astype(np.float32).astype(np.float64))


def frame_positions(N, n_fft, hop):
    """q [T_rec, n_fft]: the position frame t reads at entry j, after the two reflections"""
    Np = N + (n_fft - N % n_fft)
    q = torch.arange(1 + Np // hop)[:, None] * hop - n_fft // 2 + torch.arange(n_fft)[None, :]
    q = torch.where(q < 0, -q, q)
    return torch.where(q >= Np, 2 * (Np - 1) - q, q)


def env64(N, n_fft, hop, w=None):
    """the overlap-added squared window of the recording at centred positions n + half, [Np + n_fft]"""
    Np, w = N + (n_fft - N % n_fft), hann64(n_fft) if w is None else w
    idx = torch.arange(1 + Np // hop)[:, None] * hop + torch.arange(n_fft)[None, :]
    return torch.zeros(Np + n_fft, dtype=torch.float64).index_add(0, idx.reshape(-1), (w * w).expand(idx.shape[0], -1).reshape(-1))


def masked_frames64(fr, cols, n_fft, w=None):
    """w . F^-1 diag(cols[:, t]) F (w . fr[t]): fr [T, n_fft], cols [F, T]"""
    w = hann64(n_fft) if w is None else w
    return torch.fft.irfft(torch.fft.rfft(fr * w, dim=1) * cols.T.to(torch.float64), n=n_fft, dim=1) * w


def rec_frames64(x, n_fft, hop):
    """the frame input vectors [T_rec, n_fft] of the recording x [N], before the window"""
    N = x.shape[0]
    q = frame_positions(N, n_fft, hop)
    return torch.where(q < N, x[q.clamp(max=N - 1)], torch.zeros((), dtype=x.dtype))


def rec_operator64(x, mask, n_fft, hop, w=None):
    """A(x) [N] of the recording x [N] under mask [F, T_rec], float64; w: another window than hann64's (the exact Hann window of torch.stft)"""
    N, half = x.shape[0], n_fft // 2
    Np = N + (n_fft - N % n_fft)
    fr = masked_frames64(rec_frames64(x, n_fft, hop), mask, n_fft, w)
    idx = torch.arange(fr.shape[0])[:, None] * hop + torch.arange(n_fft)[None, :]
    acc = torch.zeros(Np + n_fft, dtype=torch.float64).index_add(0, idx.reshape(-1), fr.reshape(-1))
    return acc[half:half + N] / env64(N, n_fft, hop, w)[half:half + N]


def window_frames64(xw, kh, kf, s, N, n_fft, hop):
    """(t, fr): the recording frames t = s / hop + j of the window frames j with kf == 0, and their input vectors [len(t), n_fft] read from
    the window xw [L] (absent samples as 0; a position outside the window reads 0)"""
    L = xw.shape[0]
    t = s // hop + torch.nonzero(kf == 0).reshape(-1)
    q = frame_positions(N, n_fft, hop)[t]
    i = q - s
    xin = torch.where(kh <= -2, torch.zeros((), dtype=xw.dtype), xw)
    return t, torch.where((q < N) & (i >= 0) & (i < L), xin[i.clamp(0, L - 1)], torch.zeros((), dtype=xw.dtype))


def window_c64(xw, state, s, N, mask, n_fft, hop):
    """c [L]: the recording's operator over the computable frames of the window, at s + i (0 at absent positions)"""
    L, half = xw.shape[0], n_fft // 2
    kh, kf = state[:L], state[L:]
    Np = N + (n_fft - N % n_fft)
    t, fr = window_frames64(xw, kh, kf, s, N, n_fft, hop)
    fr = masked_frames64(fr, mask[:, t], n_fft)
    size = max(Np + n_fft, s + half + L)
    idx = t[:, None] * hop + torch.arange(n_fft)[None, :]
    acc = torch.zeros(size, dtype=torch.float64).index_add(0, idx.reshape(-1), fr.reshape(-1))
    env = torch.ones(size, dtype=torch.float64)
    env[:Np + n_fft] = env64(N, n_fft, hop)
    env = torch.where(env > 0, env, torch.ones_like(env))
    return acc[s + half:s + half + L] / env[s + half:s + half + L]


def window_apply64(xw, state, s, N, mask, n_fft, hop):
    """apply of include/aid_spec_long.h for one item, float64"""
    L = xw.shape[0]
    kh = state[:L]
    c = window_c64(xw, state, s, N, mask, n_fft, hop)
    return torch.where(kh > 0, xw, torch.where(kh == 0, c, torch.zeros_like(c)))


def window_project64(xw, yw, state, s, N, mask, n_fft, hop):
    L = xw.shape[0]
    kh = state[:L]
    c = window_c64(xw, state, s, N, mask, n_fft, hop)
    return torch.where(kh > 0, yw, torch.where(kh == 0, (-c + yw) + xw, xw))


def rect_mask(N, n_fft, hop, t_lo, t_hi, f_lo=3, f_hi=None):
    """ones [F, T_rec] with zeros over bins [f_lo, f_hi) of frames [t_lo, t_hi)"""
    Np = N + (n_fft - N % n_fft)
    m = torch.ones(n_fft // 2 + 1, 1 + Np // hop)
    m[f_lo:(n_fft // 4 if f_hi is None else f_hi), t_lo:t_hi] = 0
    return m


# ---- the computable-frame rule and the states ----------------------------------------------------------------------------------------
def _brute_state(N, L, n_fft, hop, s, head, tail):
    """window_state from the rule itself: entry by entry, frame by frame"""
    half, Np = n_fft // 2, N + (n_fft - N % n_fft)
    T_rec, Tw = 1 + Np // hop, 1 + (L + n_fft) // hop

    def ok(t):
        for j in range(n_fft):
            q = t * hop - half + j
            if q < 0:
                q = -q
            if q >= Np:
                q = 2 * (Np - 1) - q
            if q < N and not s <= q < s + L:
                return False
        return True
    comp = [ok(t) for t in range(T_rec)]
    st = np.empty(L + Tw, dtype=np.float32)
    for i in range(L):
        n = s + i
        if n >= N:
            st[i] = -2
        elif i < head or i >= L - tail:
            st[i] = 1
        else:
            cover = [t for t in range(T_rec) if t * hop - half <= n < t * hop - half + n_fft]
            st[i] = 0 if cover and all(comp[t] for t in cover) else -1
    for j in range(Tw):
        t = s // hop + j
        st[L + j] = -2 if t >= T_rec else (0 if comp[t] else -1)
    return st


@pytest.mark.parametrize("N,L,end,n_fft,hop", SPEC_CASES + TAIL_CASES)
def test_window_state_is_the_brute_force_rule_and_owned_ranges_tile_the_recording_in_state_0(N, L, end, n_fft, hop):
    from audio_inpainting_diffusion_amd.bwe_long import bwe_windows
    from audio_inpainting_diffusion_amd.restore import aligned_end
    from audio_inpainting_diffusion_amd.spec_long import padded_length, rec_frames, spec_windows, window_frames, window_state
    end2 = aligned_end(L, end, hop)
    Np, T_rec, Tw = padded_length(N, n_fft), rec_frames(N, n_fft, hop), window_frames(L, n_fft, hop)
    assert Np == N + (n_fft - N % n_fft) and Np % n_fft == 0 and 0 < Np - N <= n_fft and T_rec == 1 + Np // hop and Tw == 1 + (L + n_fft) // hop
    wins = spec_windows(N, L, end, n_fft, hop)
    assert wins == bwe_windows(N, L, end2, 2 * n_fft - 1) and (len(wins) > 1) == (N > L)
    assert all(w[0] % hop == 0 for w in wins)
    count = np.zeros(N, dtype=np.int64)
    for w, (s, head, tail, lo, hi) in enumerate(wins):
        st = window_state(N, L, n_fft, hop, s, head, tail)
        assert st.dtype == np.float32 and st.shape == (L + Tw,)
        assert np.array_equal(st, _brute_state(N, L, n_fft, hop, s, head, tail)), (w, s)
        kh, kf = st[:L], st[L:]
        count[s + lo:s + hi] += 1
        assert bool((kh[lo:hi] == 0).all()), (w, s, lo, hi)                         # every owned sample is observed
        run = np.flatnonzero(kh == 0)
        assert run.size and bool((np.diff(run) == 1).all())                        # one contiguous run
        if s > 0 and head == 0:
            assert run[0] == n_fft - hop                                            # the first sample whose frames all start inside the window
        assert bool((kf[np.arange(Tw) + s // hop >= T_rec] == -2).all()) and bool((kf[np.arange(Tw) + s // hop < T_rec] != -2).all())
        if s + L >= N:
            assert T_rec - 1 - s // hop < Tw and kf[T_rec - 1 - s // hop] == 0       # the recording's last frame is a slot of the last window, and computable
    assert bool((count == 1).all())                                                # [0, N) exactly once
    with pytest.raises(Exception, match="no multiple of hop_length"):
        window_state(N, L, n_fft, hop, 1, 0, 0)


def test_the_reflection_about_the_padded_end_reads_signal_only_from_half_a_block_on():
    """N % n_fft >= half: the recording's last frame reads real samples through the reflection about Np (its lowest position is Np - half - 1;
    at N % n_fft == half that is the one sample N - 1), and is computable in the last window because that window holds them; below half it
    reads appended zeros only."""
    from audio_inpainting_diffusion_amd.spec_long import computable, rec_frames
    n_fft, hop, L = 64, 16, 1000
    for r, reads in ((0, False), (1, False), (31, False), (32, True), (33, True), (63, True)):
        N = 3008 + r
        T_rec = rec_frames(N, n_fft, hop)
        q = frame_positions(N, n_fft, hop)[T_rec - 1]
        assert bool((q < N).any()) == reads
        assert bool(computable([T_rec - 1], N, L, n_fft, hop, 2208)[0])             # the last window [2208, 3208) holds what it reads
        assert bool(computable([T_rec - 1], N, L, n_fft, hop, 0)[0]) == (not reads)  # the first window does not


def test_the_grid_refuses_an_aligned_overlap_below_four_times_the_frame_reach():
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.spec_long import spec_windows
    with pytest.raises(_lib.AidError, match=r"end = 248 must be >= 2 \(K - 1\) = 252"):
        spec_windows(5000, 1000, 240, 64, 16)                                       # end' = 240 + (760 % 16) = 248 < 4 * 63
    assert spec_windows(1000, 1000, 240, 64, 16) == [(0, 0, 0, 0, 1000)] and spec_windows(900, 1000, 240, 64, 16) == [(0, 0, 0, 0, 900)]
    assert len(spec_windows(5000, 1000, 252, 64, 16)) > 1                           # end' = 252 + (748 % 16) = 264 >= 252
    with pytest.raises(_lib.AidError, match="end"):
        spec_windows(5000, 1000, 500, 64, 16)                                       # 2 end' = L


# ---- exactness in float64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L,end,n_fft,hop", SPEC_CASES + TAIL_CASES[3:])
def test_computable_frames_are_the_recordings_exactly_and_state_0_samples_carry_the_recordings_operator(N, L, end, n_fft, hop):
    """In every window the frame input vector of every computable frame -- read from the window through the reflection rule, absent samples
    as 0 -- differs from the recording's by exactly 0.0 in float64; the window operator equals the recording's at every state-0 sample to
    1e-12 relative (the same arithmetic on the same numbers; only the order of the overlap-add differs), and the recording's operator is
    torch.stft / torch.istft's (oracle.sampler.spectral_mask_apply)."""
    from audio_inpainting_diffusion_amd.spec_long import rec_frames, spec_windows, window_state
    from oracle.sampler import spectral_mask_apply
    gen = torch.Generator().manual_seed(N + L + n_fft)
    x = torch.randn(N, generator=gen, dtype=torch.float64)
    T_rec = rec_frames(N, n_fft, hop)
    mask = (torch.rand(n_fft // 2 + 1, T_rec, generator=gen) > 0.3).double()
    y = rec_operator64(x, mask, n_fft, hop)
    ref = spectral_mask_apply(x[None, :], mask, n_fft, hop, n_fft)[0]                                 # (the exact Hann window: compared with the same)
    exact = rec_operator64(x, mask, n_fft, hop, torch.hann_window(n_fft, dtype=torch.float64))
    assert float((exact - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert float((y - ref).abs().max()) <= 1e-6 * float(ref.abs().max())                              # (the window rounded to fp32, as the kernels hold it)
    rec = rec_frames64(x, n_fft, hop)
    seen = set()
    for s, head, tail, lo, hi in spec_windows(N, L, end, n_fft, hop):
        st = torch.from_numpy(window_state(N, L, n_fft, hop, s, head, tail))
        seen |= set(st[L:].tolist())
        n_in = min(L, N - s)
        xw = torch.cat([x[s:s + n_in], torch.randn(L - n_in, generator=gen, dtype=torch.float64)])    # (what stands at absent samples must not matter)
        t, fr = window_frames64(xw, st[:L], st[L:], s, N, n_fft, hop)
        assert t.numel() and float((fr - rec[t]).abs().max()) == 0.0
        c = window_apply64(xw, st, s, N, mask, n_fft, hop)
        obs = torch.nonzero(st[:L] == 0).reshape(-1)
        assert obs.numel() >= hi - lo
        assert float((c[obs] - y[s + obs]).abs().max()) <= 1e-12 * float(y.abs().max())
        known = st[:L] > 0
        assert torch.equal(c[known], xw[known]) and bool((c[(st[:L] < 0)] == 0).all())
    if N > L:
        assert seen >= {-1.0, 0.0}


# ---- the job rule ------------------------------------------------------------------------------------------------------------------------
def test_a_window_is_a_job_when_its_owned_range_holds_a_sample_under_a_touched_frame():
    from audio_inpainting_diffusion_amd.spec_long import rec_frames, spec_plan, spec_windows, touched_frames
    N, L, end, n_fft, hop = 5000, 1200, 300, 64, 16
    half, T_rec = n_fft // 2, rec_frames(N, n_fft, hop)
    wins = spec_windows(N, L, end, n_fft, hop)
    assert len(wins) >= 4
    ones = torch.ones(n_fft // 2 + 1, T_rec)
    assert not bool(touched_frames(ones).any()) and spec_plan(touched_frames(ones), 2, N, L, end, n_fft, hop) == ([], [])
    # a rectangle whose frames cover samples of window 2's owned range only
    s, head, tail, lo, hi = wins[2]
    t_lo, t_hi = -(-(s + lo + half) // hop), (s + hi - half) // hop + 1              # frames [t_lo, t_hi) cover [t_lo hop - half, (t_hi - 1) hop + half) inside [s + lo, s + hi)
    assert t_lo * hop - half >= s + lo and (t_hi - 1) * hop + half <= s + hi and t_hi - t_lo > 3
    inside = rect_mask(N, n_fft, hop, t_lo, t_hi)
    tf = touched_frames(inside)
    assert tf.shape == (1, T_rec) and tf.dtype == torch.bool and torch.nonzero(tf[0]).reshape(-1).tolist() == list(range(t_lo, t_hi))
    assert spec_plan(tf, 2, N, L, end, n_fft, hop) == ([(r,) + wins[2] for r in range(2)], [])          # (a one-row mask repeats its jobs)
    # one frame further to the right reaches into window 3's owned range: both are jobs
    across = rect_mask(N, n_fft, hop, t_hi - 1, t_hi + 1)
    assert spec_plan(touched_frames(across), 1, N, L, end, n_fft, hop) == ([(0,) + wins[2]], [(0,) + wins[3]])
    # per-recording masks: each recording gets its own jobs; a bin that differs from 1 without being 0 touches its frame too
    soft = ones.clone()
    soft[5, (wins[1][0] + wins[1][3]) // hop + 3] = 0.5
    per = torch.stack([inside, soft])
    assert spec_plan(touched_frames(per), 2, N, L, end, n_fft, hop) == ([(0,) + wins[2]], [(1,) + wins[1]])
    # a frame that covers only positions at and past N affects no sample
    late = rect_mask(N, n_fft, hop, T_rec - 1, T_rec)
    assert (T_rec - 1) * hop - half >= N and spec_plan(touched_frames(late), 1, N, L, end, n_fft, hop) == ([], [])
    with pytest.raises(Exception, match="touched"):
        spec_plan(np.zeros((1, T_rec + 1), dtype=bool), 1, N, L, end, n_fft, hop)
    with pytest.raises(Exception, match="touched"):
        spec_plan(np.zeros((3, T_rec), dtype=bool), 2, N, L, end, n_fft, hop)


def test_an_unaffected_sample_of_the_masked_recording_is_the_signal():
    """what the job rule rests on: where no touched frame covers n, A(x)[n] = x[n] (to rounding)"""
    from audio_inpainting_diffusion_amd.spec_long import rec_frames
    N, n_fft, hop = 3777, 64, 16
    x = torch.randn(N, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    mask = rect_mask(N, n_fft, hop, 60, 90)
    y = rec_operator64(x, mask.double(), n_fft, hop)
    affected = torch.zeros(N, dtype=torch.bool)
    affected[60 * hop - n_fft // 2:89 * hop + n_fft // 2] = True
    assert rec_frames(N, n_fft, hop) == mask.shape[1]
    assert float((y - x)[~affected].abs().max()) <= 1e-13 and float((y - x)[affected].abs().max()) > 1e-3


# ---- the pass loop: seeds ----------------------------------------------------------------------------------------------------------------
def test_the_seed_rule_of_run_passes_holds_with_the_aligned_step(monkeypatch):
    from audio_inpainting_diffusion_amd import restore, spec_long
    from audio_inpainting_diffusion_amd.restore import aligned_end
    N, L, end, n_fft, hop = 5000, 1200, 300, 64, 16
    step = L - aligned_end(L, end, hop)
    wins = spec_long.spec_windows(N, L, end, n_fft, hop)
    A = [(r,) + w for r in range(2) for w in wins[0::2]]
    B = [(r,) + w for r in range(2) for w in wins[1::2]]
    monkeypatch.setattr(restore, "job_table", lambda jobs, device: list(jobs))
    monkeypatch.setattr(restore, "window_scatter", lambda x, out, table: None)

    class Stub:
        seeds = "untouched"
    stub, seen = Stub(), []

    def predict(win, c0, c1):
        seen.append(stub.seeds)
        return torch.zeros(c1 - c0, L)
    for seeds in ([7, 9], None):
        seen.clear()
        restore.run_passes(stub, torch.zeros(2, N), (A, B), step, 3, seeds, lambda table: None, predict)
        flat = [s for chunk in seen for s in (chunk if chunk is not None else [None])]
        if seeds is None:
            assert all(s is None for s in flat)
        else:
            assert flat == [seeds[r] * restore.SEED_STRIDE + wins.index(tuple(w)) for r, *w in A + B]
        assert stub.seeds == "untouched"


# ---- refusals that need no GPU, the harness wrapper --------------------------------------------------------------------------------------
def _stub_sampler(rid=False, overlap=0.25, dc=None, n_fft=256, hop=64, window="hann", win_length=None):
    from test_bwe_long_host import _Fused
    from audio_inpainting_diffusion_amd.config import small_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.sampler import Sampler
    args = small_args(xi=0.25)
    args.tester.autoregressive.overlap = overlap
    args.tester.data_consistency.use = dc is not None
    if dc is not None:
        args.tester.data_consistency.type = dc
    st = args.tester.spectrogram_inpainting.stft
    st.n_fft, st.hop_length, st.win_length, st.window = n_fft, hop, n_fft if win_length is None else win_length, window
    return Sampler(model=_Fused(), diff_params=EDM(args), args=args, rid=rid), int(args.exp.audio_len)


def test_every_refusal_is_raised_before_any_launch(monkeypatch):
    from audio_inpainting_diffusion_amd import _lib, spec_long
    launched = []
    monkeypatch.setattr(_lib, "call", lambda name, p: launched.append(name))
    monkeypatch.setattr(spec_long, "spec_plan", lambda *a, **k: launched.append("plan"))
    monkeypatch.setattr(spec_long, "touched_frames", lambda *a, **k: launched.append("touched"))
    smp, L = _stub_sampler()
    smp.seeds = [5]
    end = L // 4
    n_fft, hop = 256, 64
    F, N = n_fft // 2 + 1, 3 * L
    T = spec_long.rec_frames(N, n_fft, hop)
    y, mask = torch.zeros(2, N), torch.ones(F, T)                              # (on the host: a valid call is refused for that, every other one for its own reason)
    sentences = []

    def refused(match, call, exc=_lib.AidError):
        with pytest.raises(exc, match=match) as e:
            call()
        sentences.append(str(e.value))

    call = smp.predict_spectrogram_inpainting_long
    refused("GPU only", lambda: call(y, mask, max_batch=1, seeds=[1, 2]))
    refused("GPU only", lambda: call(y, mask.expand(2, F, T)))
    refused("GPU only", lambda: spec_long.spec_passes(smp, y, mask, n_fft, hop, L, end))
    for dc in ("always", "end"):
        refused("GPU only", lambda: _stub_sampler(dc=dc)[0].predict_spectrogram_inpainting_long(y, mask))    # (data consistency is served, not refused)
    refused("rid", lambda: _stub_sampler(rid=True)[0].predict_spectrogram_inpainting_long(y, mask))
    refused("hann", lambda: _stub_sampler(window="hamming")[0].predict_spectrogram_inpainting_long(y, mask), NotImplementedError)
    for nf, h in ((250, 50), (8, 4), (16384, 64)):
        refused("n_fft must be a power of two", lambda: _stub_sampler(n_fft=nf, hop=h)[0].predict_spectrogram_inpainting_long(y, mask))
    for h in (0, -64, 96, 60, 512, 2.0):
        refused("hop_length must divide n_fft", lambda: _stub_sampler(hop=h)[0].predict_spectrogram_inpainting_long(y, mask))
    for wl in (0, 257, 2.5):
        refused("win_length", lambda: _stub_sampler(win_length=wl)[0].predict_spectrogram_inpainting_long(y, mask))
    for bad in (torch.ones(F, T + 1), torch.ones(F, T - 1), torch.ones(F + 1, T), torch.ones(3, F, T), torch.ones(T), torch.ones(1, 1, F, T), None, mask.numpy(),
                torch.ones(F, 1 + N // hop)):
        refused(rf"must be \[{F}, {T}\]", lambda: call(y, bad))
    for bad in ([1], [1, 2, 3]):
        refused("seeds", lambda: call(y, mask, seeds=bad))
    for bad in (0, -2, 2.5, "two", None, True):
        refused("max_batch", lambda: call(y, mask, max_batch=bad))
    for bad in (y.double(), y.half(), y.long(), y[0], y[:, None, :], y.numpy(), y[:, :0], y[:0], y[:, ::2]):
        refused("float32 recordings", lambda: call(bad, mask))
    for ov in (0.5, 0.75, 0.0):
        refused("end", lambda: _stub_sampler(overlap=ov)[0].predict_spectrogram_inpainting_long(y, mask))
    assert int(0.2 * L) + (L - int(0.2 * L)) % hop < 4 * (n_fft - 1)
    refused(r"2 \(K - 1\) = 1020", lambda: _stub_sampler(overlap=0.2)[0].predict_spectrogram_inpainting_long(y, mask))     # end' < 1020, more than one window
    one = torch.ones(F, spec_long.rec_frames(L, n_fft, hop))
    refused("GPU only", lambda: _stub_sampler(overlap=0.2)[0].predict_spectrogram_inpainting_long(y[:, :L], one))           # one window: any n_fft (refused for the device alone)
    # the device of y is judged last: a host y with any other fault is refused for that fault
    refused("seeds", lambda: spec_long.check_spec_args(y, mask, n_fft, hop, None, "hann", L, end, 8, [1]))
    refused("GPU only", lambda: spec_long.check_spec_args(y, mask, n_fft, hop, None, "hann", L, end, 8, [1, 2]))
    assert all(s.count(". ") == 0 and not s.rstrip().endswith(".") for s in sentences), [s for s in sentences if s.count(". ")]    # one sentence each
    assert launched == [] and smp.seeds == [5] and smp.y is None and smp.spectral is None and smp.n_evals == 0


def test_spectrogram_inpainting_long_groups_equal_lengths_and_checks_its_arguments():
    from audio_inpainting_diffusion_amd.harness import spectrogram_inpainting_long

    class Rec:
        def __init__(self):
            self.calls = []

        def predict_spectrogram_inpainting_long(self, y, mask, max_batch=8, seeds=None):
            self.calls.append((tuple(y.shape), tuple(mask.shape), max_batch, seeds))
            return y + mask[:, 0, :1]

    files = [torch.full((n,), float(k)) for k, n in enumerate((70, 30, 70, 31, 30, 70))]
    masks = [torch.full((5, 3 + f.numel() // 10), float(10 * k)) for k, f in enumerate(files)]
    rec = Rec()
    out = spectrogram_inpainting_long(rec, files, masks, seeds=[10, 11, 12, 13, 14, 15], max_batch=4, device="cpu")
    assert [c[:2] for c in rec.calls] == [((3, 70), (3, 5, 10)), ((2, 30), (2, 5, 6)), ((1, 31), (1, 5, 6))]
    assert all(c[2] == 4 for c in rec.calls) and [c[3] for c in rec.calls] == [[10, 12, 15], [11, 14], [13]]
    assert all(torch.equal(o, f + 10 * k) for k, (o, f) in enumerate(zip(out, files)))     # in the order of the files, each under its own mask
    rec = Rec()
    spectrogram_inpainting_long(rec, files, masks, device="cpu")
    assert all(c[2] == 8 and c[3] is None for c in rec.calls)
    with pytest.raises(ValueError):
        spectrogram_inpainting_long(rec, files, masks, seeds=[1], device="cpu")
    with pytest.raises(ValueError):
        spectrogram_inpainting_long(rec, files, masks[:2], device="cpu")
    with pytest.raises(ValueError):
        spectrogram_inpainting_long(rec, files[:1], [torch.ones(5)], device="cpu")
