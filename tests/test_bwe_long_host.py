"""CPU tests (no GPU) of bandwidth extension of whole recordings (bwe_long.py, include/aid_bwe_long.h, Sampler.predict_bwe_long,
harness.bwe_long): the window plan (ownership tiles the recording; every owned sample is observed with its
whole filter support), the exactness of the window operator in float64, and the refusals, all raised before anything touches a GPU."""

import numpy as np
import pytest
import torch


# (N, L, end, K): odd and even tap counts, K = 1, end = 2 (K - 1) + 1 and end = 2 (K - 1) + 1 with an even K, one window shorter than, equal
# to and one sample longer than L, and a last odd window
BWE_CASES = [(1000, 256, 64, 9), (1000, 256, 64, 8), (1001, 256, 1, 1), (2500, 256, 127, 33), (2500, 256, 127, 64), (100, 256, 64, 9),
             (256, 256, 64, 9), (257, 256, 64, 33), (449, 256, 64, 32)]


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L,end,K", BWE_CASES)
def test_owned_ranges_tile_the_recording_and_every_owned_sample_is_filtered(N, L, end, K):
    from audio_inpainting_diffusion_amd.bwe_long import bwe_plan, bwe_windows, window_state
    from audio_inpainting_diffusion_amd.restore import restore_windows
    wins = bwe_windows(N, L, end, K)
    grid = restore_windows(N, L, end)
    m, step = K - 1, L - end
    assert [w[0] for w in wins] == [g[0] for g in grid] == [w * step for w in range(len(wins))]
    count = np.zeros(N, dtype=np.int64)
    for w, (s, head, tail, lo, hi) in enumerate(wins):
        assert 0 <= lo < hi <= min(L, N - s), (w, lo, hi)
        count[s + lo:s + hi] += 1
        if w % 2 == 0:
            assert (head, tail) == (0, 0)
        else:
            assert head == end - m and tail == (0 if w == len(wins) - 1 else end - m)
        k = window_state(N, L, K, s, head, tail)
        assert k.dtype == np.float32 and k.shape == (L,) and set(np.unique(k)) <= {-2.0, -1.0, 0.0, 1.0}
        assert bool((k[lo:hi] == 0).all()), w                                  # every owned sample: filtered, in its own window
        assert bool((k[N - s:] == -2).all()) and bool((k[:min(L, N - s)] != -2).all())
        if w % 2:
            assert not bool((k == -1).any())                                     # only even windows (pass A) have unobserved samples
            assert bool((k[:head] == 1).all()) and bool((k[L - tail:] == 1).all() if tail else True)
    assert bool((count == 1).all())                                              # [0, N) exactly once
    A, B = bwe_plan(2, N, L, end, K)
    assert A == [(r,) + w for r in range(2) for w in wins[0::2]] and B == [(r,) + w for r in range(2) for w in wins[1::2]]


def _fir_same(x, h):
    """"same" correlation in float64, taps in ascending order per output: out[i] = sum_k h[k] x[i + k - P], zeros outside"""
    K, n = h.size, x.size
    P = (K - 1) // 2
    xp = np.concatenate([np.zeros(P), x, np.zeros(K - 1 - P)])
    acc = np.zeros(n)
    for k in range(K):
        acc = acc + h[k] * xp[k:k + n]
    return acc


def fir_observed_host(x, h, k, mode="apply", y=None):
    """float64 numpy model of FIRObserved on one window: x, k [L]"""
    xin = np.where(k == -2, 0.0, x)
    if mode == "adjoint":
        K = h.size
        P = (K - 1) // 2
        gin = np.where(k == 0, x, 0.0)
        gp = np.concatenate([np.zeros(K - 1 - P), gin, np.zeros(P)])
        a = np.zeros(x.size)
        for j in range(K):
            a = a + h[j] * gp[K - 1 - j:K - 1 - j + x.size]                     # a[i] = sum_j h[j] gin[i - j + P]
        return np.where(k == -2, 0.0, np.where(k == 1, a + x, a))
    c = _fir_same(xin, h)
    if mode == "apply":
        return np.where(k == 1, x, np.where(k == 0, c, 0.0))
    return np.where(k == 1, y, np.where(k == 0, (-c + y) + x, x))


@pytest.mark.parametrize("N,L,end,K", BWE_CASES)
def test_the_window_operator_on_the_true_signal_reproduces_the_filtered_recording_exactly(N, L, end, K):
    """rec = FIR_same(x) over the whole recording.  In every window, the operator applied to the true window equals rec wherever the state is
    0, with difference exactly 0.0 in float64: the same dot product over the same samples (zeros beyond the ends of the recording)."""
    from audio_inpainting_diffusion_amd.bwe_long import bwe_windows, window_state
    rng = np.random.default_rng(N + K)
    x, h = rng.standard_normal(N), rng.standard_normal(K)
    rec = _fir_same(x, h)
    seen = np.zeros(N, dtype=bool)
    for s, head, tail, lo, hi in bwe_windows(N, L, end, K):
        n_in = min(L, N - s)
        xw = np.concatenate([x[s:s + n_in], rng.standard_normal(L - n_in)])      # (what stands at absent samples must not matter)
        k = window_state(N, L, K, s, head, tail)
        got = fir_observed_host(xw, h, k)
        obs = k == 0
        assert not bool(obs[n_in:].any()) and bool(obs.any())
        assert float(np.abs(got[:n_in][obs[:n_in]] - rec[s:s + n_in][obs[:n_in]]).max()) == 0.0
        assert bool((got[k == 1] == xw[k == 1]).all()) and bool((got[k < 0] == 0).all())
        # the adjoint of the host model is the transpose of its apply
        g = rng.standard_normal(L)
        lhs, rhs = float(np.dot(fir_observed_host(xw, h, k), g)), float(np.dot(xw, fir_observed_host(g, h, k, "adjoint")))
        assert abs(lhs - rhs) <= 1e-12 * (np.abs(xw).sum() * np.abs(h).sum() * np.abs(g).max() + 1)
        seen[s + lo:s + hi] |= obs[lo:hi]
    assert bool(seen.all())


# ---- refusals that need no GPU, the harness wrapper --------------------------------------------------------------------------------------
class _Fused:                                                                # (stands for the MI355X network: never evaluated here)
    denoise = denoise_guided = None


def _stub_sampler(rid=False, overlap=0.25):
    from audio_inpainting_diffusion_amd.config import small_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.sampler import Sampler
    args = small_args(xi=0.25)
    args.tester.autoregressive.overlap = overlap
    return Sampler(model=_Fused(), diff_params=EDM(args), args=args, rid=rid), int(args.exp.audio_len)


def test_windows_refuse_an_overlap_below_twice_the_filter_reach_only_with_more_than_one_window():
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.bwe_long import bwe_windows
    assert len(bwe_windows(1000, 256, 64, 33)) > 1                           # end = 2 (K - 1): allowed
    for K in (34, 64, 501):
        with pytest.raises(_lib.AidError, match=r"2 \(K - 1\)"):
            bwe_windows(1000, 256, 64, K)
        assert bwe_windows(256, 256, 64, K) == [(0, 0, 0, 0, 256)] and bwe_windows(100, 256, 64, K) == [(0, 0, 0, 0, 100)]     # one window: any K
    for bad in (0, -1):
        with pytest.raises(_lib.AidError, match="K ="):
            bwe_windows(1000, 256, 64, bad)
    for end in (0, 128, 256):
        with pytest.raises(_lib.AidError, match="end"):
            bwe_windows(1000, 256, end, 1)


def test_every_refusal_is_raised_before_any_launch(monkeypatch):
    from audio_inpainting_diffusion_amd import _lib, bwe_long
    launched = []
    monkeypatch.setattr(_lib, "call", lambda name, p: launched.append(name))
    monkeypatch.setattr(bwe_long, "bwe_plan", lambda *a, **k: launched.append("plan"))
    smp, L = _stub_sampler()
    smp.seeds = [5]
    N, end = 3 * L, L // 4
    taps = torch.ones(33) / 33
    y = torch.zeros(2, N)                                                    # (on the host: a valid call is refused for that, every other one for its own reason)
    with pytest.raises(_lib.AidError, match="GPU only"):
        smp.predict_bwe_long(y, taps, "firwin", max_batch=1, seeds=[1, 2])
    with pytest.raises(_lib.AidError, match="GPU only"):
        smp.predict_bwe_long(y, taps[None, None, :], "firwin_hpf")
    with pytest.raises(_lib.AidError, match="GPU only"):
        bwe_long.bwe_passes(smp, y, taps, "firwin", L, end)
    for ftype, why in (("cheby1", "IIR filter carries state"), ("biquad", "IIR filter carries state"), ("decimate", "phase depends on the window start"),
                       ("resample", "phase depends on the window start")):
        with pytest.raises(_lib.AidError, match=why) as e:
            smp.predict_bwe_long(y, 2, ftype)
        assert ftype in str(e.value) and str(e.value).count(". ") == 0       # one sentence
    with pytest.raises(NotImplementedError):
        smp.predict_bwe_long(y, taps, "butterworth")
    with pytest.raises(_lib.AidError, match=r"2 \(K - 1\)"):
        smp.predict_bwe_long(y, torch.ones(end // 2 + 2), "firwin")          # end < 2 (K - 1), three windows
    with pytest.raises(_lib.AidError, match="GPU only"):
        smp.predict_bwe_long(y[:, :L], torch.ones(end // 2 + 2), "firwin")   # one window: any K (refused for the device alone)
    for bad in (torch.ones(2, 33), torch.ones(0), torch.tensor(1.0)):
        with pytest.raises(_lib.AidError, match="taps"):
            smp.predict_bwe_long(y, bad, "firwin")
    for bad in ([1], [1, 2, 3]):
        with pytest.raises(_lib.AidError, match="seeds"):
            smp.predict_bwe_long(y, taps, "firwin", seeds=bad)
    for bad in (0, -2):
        with pytest.raises(_lib.AidError, match="max_batch"):
            smp.predict_bwe_long(y, taps, "firwin", max_batch=bad)
    for bad in (y.double(), y.half(), y.long(), y[0], y.numpy()):
        with pytest.raises(_lib.AidError, match="float32 recordings"):
            smp.predict_bwe_long(bad, taps, "firwin")
    with pytest.raises(_lib.AidError, match="rid"):
        _stub_sampler(rid=True)[0].predict_bwe_long(y, taps, "firwin")
    for ov in (0.5, 0.75, 0.0):
        with pytest.raises(_lib.AidError, match="end"):
            _stub_sampler(overlap=ov)[0].predict_bwe_long(y, taps, "firwin")
    # the device of y is judged last: a host y with any other fault is refused for that fault
    with pytest.raises(_lib.AidError, match="seeds"):
        bwe_long.check_bwe_args(y, bwe_long.bwe_prepare(None, taps, "firwin"), L, end, 8, [1])
    with pytest.raises(_lib.AidError, match="GPU only"):
        bwe_long.check_bwe_args(y, bwe_long.bwe_prepare(None, taps, "firwin"), L, end, 8, [1, 2])
    assert launched == [] and smp.seeds == [5] and smp.y is None and smp.spectral is None and smp.n_evals == 0


def test_bwe_long_groups_equal_lengths_and_checks_its_arguments():
    from audio_inpainting_diffusion_amd.harness import bwe_long

    class Rec:
        def __init__(self):
            self.calls = []

        def predict_bwe_long(self, y, filt, filt_type, max_batch=8, seeds=None):
            self.calls.append((tuple(y.shape), filt, filt_type, max_batch, seeds))
            return y + 1

    files = [torch.full((n,), float(k)) for k, n in enumerate((700, 300, 700, 301, 300))]
    taps = torch.ones(9) / 9
    rec = Rec()
    out = bwe_long(rec, files, taps, "firwin_hpf", seeds=[10, 11, 12, 13, 14], max_batch=4, device="cpu")
    assert [c[0] for c in rec.calls] == [(2, 700), (2, 300), (1, 301)] and all(c[3] == 4 and c[2] == "firwin_hpf" and c[1] is taps for c in rec.calls)
    assert [c[4] for c in rec.calls] == [[10, 12], [11, 14], [13]]
    assert all(torch.equal(o, f + 1) for o, f in zip(out, files))        # full length, in the order of the files
    rec = Rec()
    bwe_long(rec, files, taps, device="cpu")                             # "firwin", the global generator
    assert all(c[2] == "firwin" and c[4] is None for c in rec.calls)
    with pytest.raises(ValueError):
        bwe_long(rec, files, taps, seeds=[1], device="cpu")
