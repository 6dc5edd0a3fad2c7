"""CPU tests (no GPU) of phase retrieval of whole recordings (phase_long.py, include/aid_phase_long.h, Sampler.predict_pr_long,
harness.pr_long): the hop-aligned window grid (every start a multiple of hop; ownership tiles the recording),
the exactness of the observed frames of a window in float64, the lengths, and the refusals, all raised before anything touches a GPU."""

import numpy as np
import pytest
import torch


# (N, L, end, n_fft, hop)
PR_CASES = [(4096, 4096, 1024, 256, 64), (9000, 4096, 1024, 256, 64), (9000, 4096, 1024, 256, 60), (9557, 4096, 1024, 256, 256),
            (12288, 4096, 1024, 512, 128), (1000, 4096, 1024, 256, 64), (20000, 4096, 1024, 256, 37)]


# ---- the grid ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L,end,n_fft,hop", PR_CASES)
def test_window_starts_are_multiples_of_hop_and_owned_ranges_tile_the_recording(N, L, end, n_fft, hop):
    from audio_inpainting_diffusion_amd.bwe_long import bwe_windows
    from audio_inpainting_diffusion_amd.restore import aligned_end
    from audio_inpainting_diffusion_amd.phase_long import frames_of, pr_plan, pr_windows, window_state
    end2 = aligned_end(L, end, hop)
    assert end2 == end + ((L - end) % hop) and end <= end2 < end + hop and (L - end2) % hop == 0
    if hop == 60:
        assert end2 == 1036
    step, m, Tw = L - end2, n_fft - 1, frames_of(L, hop)
    assert Tw == 1 + L // hop and frames_of(N, hop) == 1 + N // hop
    wins = pr_windows(N, L, end, n_fft, hop)
    assert wins == bwe_windows(N, L, end2, n_fft) and (len(wins) > 1) == (N > L)
    assert [w[0] for w in wins] == [w * step for w in range(len(wins))] and all(w[0] % hop == 0 for w in wins)
    count = np.zeros(N, dtype=np.int64)
    for w, (s, head, tail, lo, hi) in enumerate(wins):
        assert 0 <= lo < hi <= min(L, N - s), (w, lo, hi)
        count[s + lo:s + hi] += 1
        if w % 2 == 0:
            assert (head, tail) == (0, 0)
        else:
            assert head == end2 - m and tail == (0 if w == len(wins) - 1 else end2 - m)
        k = window_state(N, L, n_fft, hop, s, head, tail)
        assert k.dtype == np.float32 and k.shape == (L + Tw,)
        kh, kf = k[:L], k[L:]
        assert set(np.unique(kh)) <= {-2.0, -1.0, 1.0} and set(np.unique(kf)) <= {-2.0, -1.0, 0.0}
        assert bool((kh[N - s:] == -2).all()) and bool((kh[:min(L, N - s)] != -2).all())
        assert bool((kh[:head] == 1).all()) and bool((kh[L - tail:] == 1).all() if tail else True) and int((kh == 1).sum()) == head + tail
        # an observed frame lies in the window, or the recording ends in the window; it is a frame of the recording
        j = np.arange(Tw)[kf == 0]
        assert j.size and bool(((j * hop + n_fft <= L) | (s + L >= N)).all()) and bool((s // hop + j < frames_of(N, hop)).all())
    assert bool((count == 1).all())                                              # [0, N) exactly once
    A, B = pr_plan(2, N, L, end, n_fft, hop)
    assert A == [(r,) + w for r in range(2) for w in wins[0::2]] and B == [(r,) + w for r in range(2) for w in wins[1::2]]
    with pytest.raises(Exception, match="no multiple of hop_size"):
        window_state(N, L, n_fft, hop, 1, 0, 0)


def test_the_grid_refuses_an_aligned_overlap_below_twice_the_frame_reach():
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.phase_long import pr_windows
    # end' = 500 + (3596 % 64) = 512 < 2 * 511
    with pytest.raises(_lib.AidError, match=r"end = 512 must be >= 2 \(K - 1\) = 1022"):
        pr_windows(9000, 4096, 500, 512, 64)
    assert pr_windows(4096, 4096, 500, 512, 64) == [(0, 0, 0, 0, 4096)] and pr_windows(1000, 4096, 500, 512, 64) == [(0, 0, 0, 0, 1000)]     # one window: any n_fft
    assert len(pr_windows(9000, 4096, 1022, 512, 1)) > 1                        # end' = end = 2 (n_fft - 1) exactly
    with pytest.raises(_lib.AidError, match="end"):
        pr_windows(9000, 4096, 2040, 256, 64)                                   # end' = 2040 + (2056 % 64) = 2048: 2 end' = L


# ---- the observed frames ---------------------------------------------------------------------------------------------------------------
def _frames64(x, n_fft, hop, T):
    """the windowed frame vectors [T, n_fft] of x with zeros past its end (what the FFT of frame t reads), float64"""
    from audio_inpainting_diffusion_amd.phase import hamming_tables
    w = hamming_tables(n_fft)[0]
    xp = np.concatenate([x, np.zeros(T * hop + n_fft)])
    return np.stack([xp[t * hop:t * hop + n_fft] * w for t in range(T)])


def test_every_observed_frame_of_a_window_is_the_recordings_frame_exactly_and_every_owned_sample_lies_under_one():
    """In every window, the windowed frame vector of every frame with state 0 -- taken from the window with its absent samples as 0 -- equals the
    recording's (difference exactly 0.0 in float64: the same samples times the same window), so any transform of it is the recording's column;
    every sample a window owns is covered by at least one of its observed frames; all three frame states occur."""
    from audio_inpainting_diffusion_amd.phase_long import frames_of, pr_windows, window_state
    states = set()
    for N, L, end, n_fft, hop in PR_CASES:
        rng = np.random.default_rng(N + L + n_fft + hop)
        x = rng.standard_normal(N)
        T_rec, Tw = frames_of(N, hop), frames_of(L, hop)
        rec = _frames64(x, n_fft, hop, T_rec)
        for s, head, tail, lo, hi in pr_windows(N, L, end, n_fft, hop):
            st = window_state(N, L, n_fft, hop, s, head, tail)
            kh, kf = st[:L], st[L:]
            states |= set(np.unique(kf).tolist())
            n_in = min(L, N - s)
            xw = np.concatenate([x[s:s + n_in], rng.standard_normal(L - n_in)])      # (what stands at absent samples must not matter)
            got = _frames64(np.where(kh == -2, 0.0, xw), n_fft, hop, Tw)
            obs = np.arange(Tw)[kf == 0]
            assert obs.size and s // hop + obs.max() < T_rec
            assert float(np.abs(got[obs] - rec[s // hop + obs]).max()) == 0.0
            covered = np.zeros(L + n_fft, dtype=bool)
            for j in obs:
                covered[j * hop:j * hop + n_fft] = True
            assert bool(covered[lo:hi].all()), (N, L, hop, s)
    assert states == {-2.0, -1.0, 0.0}


# ---- lengths ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [1, 37, 64, 256])
def test_the_default_length_is_the_largest_consistent_one_and_an_inconsistent_one_is_refused(hop):
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.phase_long import check_length, default_length, frames_of
    for T in (2, 3, 7, 100, 1001):
        N = default_length(T, hop)
        assert N == T * hop - 1 and frames_of(N, hop) == T and frames_of(N + 1, hop) == T + 1 and check_length(T, None, hop) == N
        consistent = [q for q in range(max(1, N - 2 * hop), N + 2) if frames_of(q, hop) == T]
        assert consistent[-1] == N and len(consistent) == hop and all(check_length(T, q, hop) == q for q in consistent)
        for bad in (N + 1, consistent[0] - 1, 0, -5, N + 0.5):
            with pytest.raises(_lib.AidError, match="not consistent") as e:
                check_length(T, bad, hop)
            assert str(e.value).count(". ") == 0
    with pytest.raises(_lib.AidError, match=r"length = 1400 is not consistent with the 10 frames .* has 22 frames"):
        check_length(10, 1400, 64)                                                  # both numbers in the message
    if hop == 1:
        with pytest.raises(_lib.AidError, match="no sample"):
            check_length(1, None, 1)
    else:
        assert check_length(1, None, hop) == hop - 1


# ---- refusals that need no GPU, the harness wrapper --------------------------------------------------------------------------------------
def _stub_sampler(rid=False, overlap=0.25, dc=None, xi=0.25, win=256, hop=64):
    from test_bwe_long_host import _Fused
    from audio_inpainting_diffusion_amd.config import small_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.sampler import Sampler
    args = small_args(xi=xi)
    args.tester.autoregressive.overlap = overlap
    args.tester.data_consistency.use = dc is not None
    if dc is not None:
        args.tester.data_consistency.type = dc
    args.tester.phase_retrieval.win_size = win
    args.tester.phase_retrieval.hop_size = hop
    return Sampler(model=_Fused(), diff_params=EDM(args), args=args, rid=rid), int(args.exp.audio_len)


def test_every_refusal_is_raised_before_any_launch(monkeypatch):
    from audio_inpainting_diffusion_amd import _lib, phase_long
    launched = []
    monkeypatch.setattr(_lib, "call", lambda name, p: launched.append(name))
    monkeypatch.setattr(phase_long, "pr_plan", lambda *a, **k: launched.append("plan"))
    smp, L = _stub_sampler()
    smp.seeds = [5]
    end = L // 4
    win, hop = 256, 64
    F = win // 2 + 1
    T = 1 + (3 * L) // hop
    y = torch.zeros(2, F, T)                                                 # (on the host: a valid call is refused for that, every other one for its own reason)
    sentences = []

    def refused(match, call, exc=_lib.AidError):
        with pytest.raises(exc, match=match) as e:
            call()
        sentences.append(str(e.value))

    refused("GPU only", lambda: smp.predict_pr_long(y, max_batch=1, seeds=[1, 2]))
    refused("GPU only", lambda: smp.predict_pr_long(y, length=3 * L))
    refused("GPU only", lambda: phase_long.pr_passes(smp, y, win, hop, L, end))
    refused("GPU only", lambda: smp.predict_pr_long(y.transpose(1, 2).contiguous().transpose(1, 2)))       # (torch.stft's layout: frames strided)
    for dc in ("always", "end"):
        refused("data consistency", lambda: _stub_sampler(dc=dc)[0].predict_pr_long(y))
    refused("rid", lambda: _stub_sampler(rid=True)[0].predict_pr_long(y))
    for xi in (0, 0.0, -1.0):
        refused("xi must be > 0", lambda: _stub_sampler(xi=xi)[0].predict_pr_long(y))
    for bad in (torch.zeros(2, F + 1, T), torch.zeros(2, F - 1, T), torch.zeros(2, win, T)):
        refused(f"F = {F}", lambda: smp.predict_pr_long(bad))
    for bad in (T * hop, (T - 1) * hop - 1, 0, -3, T * hop - 1.5):
        refused("not consistent", lambda: smp.predict_pr_long(y, length=bad))
    for bad in ([1], [1, 2, 3]):
        refused("seeds", lambda: smp.predict_pr_long(y, seeds=bad))
    for bad in (0, -2, 2.5, "two", None, True):
        refused("max_batch", lambda: smp.predict_pr_long(y, max_batch=bad))
    for bad in (y.double(), y.half(), y.long(), y[0], y[:, :, 0], y.numpy(), y[:, :, :0], y[:0]):
        refused("float32 magnitude spectrograms", lambda: smp.predict_pr_long(bad))
    for w, h in ((250, 64), (8, 4), (16384, 64)):
        refused("win_size", lambda: _stub_sampler(win=w, hop=h)[0].predict_pr_long(y))
    for h in (0, 257, -1):
        refused("hop_size", lambda: _stub_sampler(hop=h)[0].predict_pr_long(y))
    for ov in (0.5, 0.75, 0.0):
        refused("end", lambda: _stub_sampler(overlap=ov)[0].predict_pr_long(y))
    assert int(0.1 * L) + (L - int(0.1 * L)) % hop < 2 * (win - 1)
    refused(r"2 \(K - 1\) = 510", lambda: _stub_sampler(overlap=0.1)[0].predict_pr_long(y))                 # end' < 510, more than one window
    refused("GPU only", lambda: _stub_sampler(overlap=0.1)[0].predict_pr_long(y[:, :, :1 + L // hop], length=L))      # one window: any n_fft (refused for the device alone)
    # the device of y is judged last: a host y with any other fault is refused for that fault
    refused("seeds", lambda: phase_long.check_pr_args(y, None, phase_long.phase.check_sizes(win, hop), L, end, 8, [1]))
    refused("GPU only", lambda: phase_long.check_pr_args(y, None, phase_long.phase.check_sizes(win, hop), L, end, 8, [1, 2]))
    assert all(s.count(". ") == 0 and not s.rstrip().endswith(".") for s in sentences), [s for s in sentences if s.count(". ")]    # one sentence each
    assert launched == [] and smp.seeds == [5] and smp.y is None and smp.spectral is None and smp.n_evals == 0


def test_pr_long_groups_equal_shapes_and_lengths_and_checks_its_arguments():
    from audio_inpainting_diffusion_amd.harness import pr_long

    class Rec:
        def __init__(self):
            self.calls = []

        def predict_pr_long(self, y, length=None, max_batch=8, seeds=None):
            self.calls.append((tuple(y.shape), length, max_batch, seeds))
            return y[:, 0, :] + 1

    files = [torch.full((5, n), float(k)) for k, n in enumerate((70, 30, 70, 31, 30, 70))]
    rec = Rec()
    out = pr_long(rec, files, lengths=[4479, None, 4479, 1983, None, 4470], seeds=[10, 11, 12, 13, 14, 15], max_batch=4, device="cpu")
    assert [(c[0], c[1]) for c in rec.calls] == [((2, 5, 70), 4479), ((2, 5, 30), None), ((1, 5, 31), 1983), ((1, 5, 70), 4470)]
    assert all(c[2] == 4 for c in rec.calls)
    assert [c[3] for c in rec.calls] == [[10, 12], [11, 14], [13], [15]]
    assert all(torch.equal(o, f[0] + 1) for o, f in zip(out, files))                     # in the order of the files
    rec = Rec()
    pr_long(rec, files, device="cpu")                                                    # default lengths, the global generator
    assert [c[0] for c in rec.calls] == [(3, 5, 70), (2, 5, 30), (1, 5, 31)] and all(c[1] is None and c[2] == 8 and c[3] is None for c in rec.calls)
    with pytest.raises(ValueError):
        pr_long(rec, files, seeds=[1], device="cpu")
    with pytest.raises(ValueError):
        pr_long(rec, files, lengths=[1400], device="cpu")
    with pytest.raises(ValueError):
        pr_long(rec, [torch.zeros(70)], device="cpu")
