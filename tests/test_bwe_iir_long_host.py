"""CPU tests (no GPU) of bandwidth extension of whole recordings through an IIR filter (bwe_iir_long.py, include/aid_bwe_long.h,
Sampler.predict_bwe_iir_long, harness.bwe_iir_long): seeding a window's recursion from the recording reproduces the recording (float64, scipy),
the window states, the plan, and the refusals, all raised before anything touches a GPU."""

import numpy as np
import pytest
import scipy.signal
import torch

L_HOST, END_HOST = 1000, 250
N_HOST = 3 * L_HOST + 17


def iir_filters():
    """name -> (filt, filt_type) of the filters of the issue: three Chebyshev low-passes and a biquad"""
    bq = scipy.signal.butter(2, 4000, fs=22050)
    return {"cheby1_4_1k_22k": (scipy.signal.cheby1(4, 0.05, 1000, fs=22050), "cheby1"),
            "cheby1_8_4k_22k": (scipy.signal.cheby1(8, 0.05, 4000, fs=22050), "cheby1"),
            "cheby1_6_1k_16k": (scipy.signal.cheby1(6, 0.05, 1000, fs=16000), "cheby1"),
            "biquad": (tuple(float(v) for v in (*bq[0], *bq[1])), "biquad")}


FILTERS = sorted(iir_filters())


def _run(k):
    """S: the length of the leading run of -3 states"""
    nz = np.nonzero(k != -3)[0]
    return int(nz[0]) if nz.size else k.size


def iir_observed_host(x, b, a, k, mode="apply", y=None):
    """float64 scipy model of IIRObserved on one window: x, k [L] (the definitions of include/aid_bwe_long.h, aid_iir_observed)"""
    L, S = x.size, _run(k)
    absent, known, filt = (k <= -2) & (k != -3), k > 0, k == 0
    if mode == "adjoint":
        g0 = np.where(filt, x, 0.0)
        w = np.zeros(L)
        w[S:] = scipy.signal.lfilter([1.0], a, g0[S:][::-1])[::-1]
        c = scipy.signal.lfilter(b, [1.0], w[::-1])[::-1]
        return np.where(absent, 0.0, np.where(known, c + x, c))
    if mode == "prepare":
        r = x.copy()
        for i in range(S, L):
            r[i] = -sum(a[j] * r[i - j] for j in range(1, a.size) if i - j >= 0)
        return np.where(known, x, np.where(filt, x - r, 0.0))
    u = scipy.signal.lfilter(b, [1.0], np.where(absent, 0.0, x))
    yh = np.zeros(L)
    yh[S:] = scipy.signal.lfilter([1.0], a, u[S:])
    if mode == "apply":
        return np.where(known, x, np.where(filt, yh, 0.0))
    return np.where(known, y, np.where(filt, (y - yh) + x, x))


def _conv64(v, h):
    """causal convolution of the rows of v [B, L] with h [L] over L samples, float64 (FFT: differentiable)"""
    n = 2 * v.shape[-1]
    return torch.fft.irfft(torch.fft.rfft(v, n) * torch.fft.rfft(h, n), n)[..., :v.shape[-1]]


def iir_observed_torch(x, b, a, k, mode="apply", y=None):
    """The same operator, vectorised over rows and differentiable: x, k [B, L] float64 torch (k may be [1, L]).  An all-pole recursion from a zero
    state is the causal convolution with its impulse response over the L samples, and gating its INPUT at S is the recursion started at S."""
    B, L = x.shape
    k = k.expand(B, L)
    i = torch.arange(L)[None, :]
    S = torch.tensor([_run(row.numpy()) for row in k])[:, None]
    imp = np.zeros(L)
    imp[0] = 1.0
    hp = torch.from_numpy(scipy.signal.lfilter([1.0], a, imp))
    hb, ha = torch.zeros(L, dtype=torch.float64), torch.zeros(L, dtype=torch.float64)
    hb[:min(L, b.size)], ha[:min(L, a.size)] = torch.from_numpy(b[:L]), torch.from_numpy(a[:L])
    absent, known, filt, zero = (k <= -2) & (k != -3), k > 0, k == 0, torch.zeros_like(x)
    if mode == "adjoint":
        flip = lambda v: v.flip(-1)                                                                                  # noqa: E731
        w = torch.where(i >= S, flip(_conv64(flip(torch.where(filt, x, zero)), hp)), zero)
        c = flip(_conv64(flip(w), hb))
        return torch.where(absent, zero, torch.where(known, c + x, c))
    if mode == "prepare":
        r = _conv64(torch.where(i < S, _conv64(torch.where(i < S, x, zero), ha), zero), hp)
        return torch.where(known, x, torch.where(filt, x - r, zero))
    yh = _conv64(torch.where(i >= S, _conv64(torch.where(absent, zero, x), hb), zero), hp)
    if mode == "apply":
        return torch.where(known, x, torch.where(filt, yh, zero))
    return torch.where(known, y, torch.where(filt, (y - yh) + x, x))


def _table(name):
    from audio_inpainting_diffusion_amd.bwe_iir_long import IIRTable
    return IIRTable(*iir_filters()[name])


def window_case(name, seed=0):
    """(table, x [N] float64, rec = lfilter(b, a, x) float64, the windows of the grid) of the host case"""
    from audio_inpainting_diffusion_amd.bwe_iir_long import iir_windows
    table = _table(name)
    x = np.random.default_rng(seed + table.order).standard_normal(N_HOST) * 0.1
    return table, x, scipy.signal.lfilter(table.b, table.a, x), iir_windows(N_HOST, L_HOST, END_HOST, table.order)


def raw_row(rec, known_from, k, s, L):
    """the raw row aid_iir_gather builds: rec at seed and filtered samples, ``known_from`` at known ones, 0 elsewhere"""
    n_in = min(L, rec.size - s)
    pad = lambda v: np.concatenate([v[s:s + n_in], np.zeros(L - n_in)])                                              # noqa: E731
    return np.where((k == -3) | (k == 0), pad(rec), np.where(k == 1, pad(known_from), 0.0))


# ---- seeding is exact --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FILTERS)
def test_seeding_from_the_recording_reproduces_the_recording_in_every_window(name):
    """rec = lfilter(b, a, x) over the whole recording, float64.  In every window of the grid the recursion seeded with rec[s .. s + order)
    gives rec at every state-0 sample to <= 1e-9 max|rec|: yh + r = rec, i.e. apply(x_w) = prepare(raw).  With the seeds rounded to float32 the
    deviation stays within seed_error_bound * max|rec|."""
    from audio_inpainting_diffusion_amd.bwe_iir_long import window_state
    table, x, rec, wins = window_case(name)
    assert len(wins) == 4
    top = np.abs(rec).max()
    rec32 = rec.astype(np.float32).astype(np.float64)
    rng = np.random.default_rng(1)
    worst = worst32 = 0.0
    seen = np.zeros(N_HOST, dtype=bool)
    for s, head, tail, lo, hi in wins:
        n_in = min(L_HOST, N_HOST - s)
        xw = np.concatenate([x[s:s + n_in], rng.standard_normal(L_HOST - n_in)])     # (what stands at absent samples must not matter)
        k = window_state(N_HOST, L_HOST, table.order, s, head, tail)
        obs = k == 0
        assert bool(obs[lo:hi].all()) and not bool(obs[n_in:].any())
        got = iir_observed_host(xw, table.b, table.a, k)
        want = iir_observed_host(raw_row(rec, x, k, s, L_HOST), table.b, table.a, k, "prepare")
        worst = max(worst, float(np.abs(got - want)[obs].max()))
        assert bool((got[k == 1] == xw[k == 1]).all()) and bool((got[k < 0] == 0).all()) and bool((want[k < 0] == 0).all())
        # float32 seeds, exact observations: the bound of the seed rounding alone
        seeded = np.where(k == -3, raw_row(rec32, x, k, s, L_HOST), raw_row(rec, x, k, s, L_HOST))
        worst32 = max(worst32, float(np.abs(got - iir_observed_host(seeded, table.b, table.a, k, "prepare"))[obs].max()))
        # the adjoint of the host model is the transpose of its apply
        g = rng.standard_normal(L_HOST)
        lhs, rhs = float(np.dot(got, g)), float(np.dot(xw, iir_observed_host(g, table.b, table.a, k, "adjoint")))
        assert abs(lhs - rhs) <= 1e-10 * np.linalg.norm(got) * np.linalg.norm(g) * table.amplification
        seen[s + lo:s + hi] |= obs[lo:hi]
    print(f"{name}: order {table.order}, amplification {table.amplification:.3g}, seed_error_bound {table.seed_error_bound:.2e}; worst deviation "
          f"{worst / top:.2e} (exact rec), {worst32 / top:.2e} (float32 seeds)")
    assert bool(seen.all())
    assert worst <= 1e-9 * top
    assert worst32 <= table.seed_error_bound * top
    assert table.seed_error_bound == table.order * table.amplification * 2.0 ** -24


@pytest.mark.parametrize("name", ["cheby1_4_1k_22k", "cheby1_8_4k_22k"])
def test_window_state_on_every_window_shape(name):
    from audio_inpainting_diffusion_amd.bwe_iir_long import iir_plan, window_state
    table, _, _, wins = window_case(name)
    o, L, step = table.order, L_HOST, L_HOST - END_HOST
    e = END_HOST - o
    assert wins == [(0, 0, 0, 0, L - o), (step, e, e, e, L - e), (2 * step, 0, 0, o, L - o), (3 * step, e, 0, e, N_HOST - 3 * step)]
    want = [np.zeros(L),                                                                                   # the first window
            np.concatenate([np.full(o, -3.0), np.ones(e - o), np.zeros(L - 2 * e), np.ones(e)]),           # odd inner: seeds before the known head
            np.concatenate([np.full(o, -3.0), np.zeros(L - o)]),                                           # even inner
            np.concatenate([np.full(o, -3.0), np.ones(e - o), np.zeros(N_HOST - 3 * step - e), np.full(L - (N_HOST - 3 * step), -2.0)])]   # odd last, cut
    for (s, head, tail, lo, hi), k_ref in zip(wins, want):
        k = window_state(N_HOST, L, o, s, head, tail)
        assert k.dtype == np.float32 and np.array_equal(k, k_ref.astype(np.float32)), s
        assert s == 0 or lo >= o                                                  # a seed sample is never owned
    A, B = iir_plan(2, N_HOST, L, END_HOST, o)
    assert A == [(r,) + w for r in range(2) for w in wins[0::2]] and B == [(r,) + w for r in range(2) for w in wins[1::2]]
    # a recording that ends inside the seeds: absent comes first
    assert np.array_equal(window_state(step + 2, L, o, step, 0, 0)[:4], np.array([-3, -3, -2, -2], np.float32))


def test_the_torch_model_is_the_scipy_model():
    """the vectorised float64 model the GPU tests compare against equals the per-row scipy model, in every mode, with seed runs of every kind"""
    table = _table("cheby1_8_4k_22k")
    rng = np.random.default_rng(5)
    B, L, o = 5, 257, table.order
    k = rng.integers(-3, 2, (B, L)).astype(np.float64)
    for r, S in enumerate((0, o, o - 1, o + 3, L)):
        k[r, :S] = -3
        if S < L:
            k[r, S] = 0
    x, y = rng.standard_normal((B, L)), rng.standard_normal((B, L))
    for mode in ("apply", "adjoint", "project", "prepare"):
        got = iir_observed_torch(torch.from_numpy(x), table.b, table.a, torch.from_numpy(k), mode, torch.from_numpy(y)).numpy()
        want = np.stack([iir_observed_host(x[r], table.b, table.a, k[r], mode, y[r]) for r in range(B)])
        assert np.abs(got - want).max() <= 1e-11 * table.amplification * np.abs(want).max(), mode


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L,end,order", [(3017, 1000, 250, 4), (3017, 1000, 250, 16), (1000, 256, 64, 8), (2500, 256, 127, 1), (100, 256, 64, 16),
                                           (256, 256, 64, 8), (257, 256, 64, 2), (449, 256, 32, 16)])
def test_owned_ranges_tile_the_recording(N, L, end, order):
    from audio_inpainting_diffusion_amd.bwe_iir_long import iir_windows, window_state
    from audio_inpainting_diffusion_amd.restore import trimmed_windows
    wins = iir_windows(N, L, end, order)
    assert wins == trimmed_windows(N, L, end, order + 1)
    count = np.zeros(N, dtype=np.int64)
    for s, head, tail, lo, hi in wins:
        count[s + lo:s + hi] += 1
        k = window_state(N, L, order, s, head, tail)
        assert bool((k[lo:hi] == 0).all()) and not bool((k == -1).any())
        assert _run(k) == (min(order, N - s) if s else 0)
    assert bool((count == 1).all())


def test_windows_refuse_an_overlap_below_twice_the_order_only_with_more_than_one_window():
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.bwe_iir_long import iir_windows
    assert len(iir_windows(1000, 256, 32, 16)) > 1                           # end = 2 order: allowed
    with pytest.raises(_lib.AidError, match=r"2 \(K - 1\)"):
        iir_windows(1000, 256, 31, 16)
    assert iir_windows(256, 256, 3, 16) == [(0, 0, 0, 0, 256)] and iir_windows(100, 256, 3, 16) == [(0, 0, 0, 0, 100)]     # one window: any order


# ---- refusals, the pooled task, the ABI --------------------------------------------------------------------------------------------------
def test_every_refusal_is_raised_before_any_launch_and_in_order(monkeypatch):
    from test_bwe_long_host import _stub_sampler
    from audio_inpainting_diffusion_amd import _lib, bwe_iir_long
    launched = []
    monkeypatch.setattr(_lib, "call", lambda name, p: launched.append(name))
    monkeypatch.setattr(bwe_iir_long, "iir_plan", lambda *a, **k: launched.append("plan"))
    smp, L = _stub_sampler()
    smp.seeds = [5]
    N, end = 3 * L, L // 4
    filt = scipy.signal.cheby1(4, 0.05, 1000, fs=22050)
    biq = iir_filters()["biquad"][0]
    y = torch.zeros(2, N)                                                    # (on the host: a valid call is refused for that, every other one for its own reason)
    for f, ft, kw in ((filt, "cheby1", dict(max_batch=1, seeds=[1, 2])), (biq, "biquad", {}), ((torch.tensor(filt[0]), torch.tensor(filt[1])), "cheby1", {})):
        with pytest.raises(_lib.AidError, match="GPU only"):
            smp.predict_bwe_iir_long(y, f, ft, **kw)
    with pytest.raises(_lib.AidError, match="GPU only"):
        bwe_iir_long.bwe_iir_passes(smp, y, filt, "cheby1", L, end)
    # 1. the other degradations of predict_bwe, each with the method that takes it -- before y or the coefficients are looked at
    for ft, where in (("firwin", "predict_bwe_long"), ("firwin_hpf", "predict_bwe_long"), ("decimate", "predict_bwe_lowrate_long"), ("resample", "predict_bwe_lowrate_long")):
        with pytest.raises(_lib.AidError, match=where + "$"):
            smp.predict_bwe_iir_long("no tensor", None, ft)
    # 2. an unknown type
    with pytest.raises(NotImplementedError):
        smp.predict_bwe_iir_long("no tensor", None, "butterworth")
    # 3. the recordings, before the coefficients
    for bad in (y.double(), y.half(), y.long(), y[0], y.numpy()):
        with pytest.raises(_lib.AidError, match="float32 recordings"):
            smp.predict_bwe_iir_long(bad, None, "cheby1")
    # 4. the coefficients, before the grid
    unstable, order17 = ([1.0], [1.0, -1.01]), (np.ones(18), np.r_[1.0, np.zeros(17)])
    sharp = scipy.signal.cheby1(8, 0.05, 2000, fs=44100)                     # (stable, but too ill-conditioned: IIRFilter's refusal)
    for bad, ft, why in ((unstable, "cheby1", "unstable"), (order17, "cheby1", "order 17"), (([1.0], [0.0, 1.0]), "cheby1", r"a\[0\]"), (([], [1.0]), "cheby1", "empty"),
                         (sharp, "cheby1", "ill-conditioned"), (3.0, "cheby1", r"\(b, a\)"), (biq[:5], "biquad", "six"), (filt, "biquad", "six"),
                         ((1.0, 0.0, 0.0, 1.0, -1.01, 0.0), "biquad", "unstable")):
        with pytest.raises(_lib.AidError, match=why):
            smp.predict_bwe_iir_long(y[:, :3], bad, ft, max_batch=0)
    # 5. the grid: end < 2 order with more than one window; one window takes any order
    f16 = np.poly(0.8 * np.exp(2j * np.pi * np.arange(16) / 16)).real
    narrow = _stub_sampler(overlap=20.5 / L)[0]                              # end = 20 < 2 * 16
    with pytest.raises(_lib.AidError, match=r"2 \(K - 1\)"):
        narrow.predict_bwe_iir_long(y, ([1.0], f16), "cheby1", max_batch=0)
    with pytest.raises(_lib.AidError, match="GPU only"):
        narrow.predict_bwe_iir_long(y[:, :L], ([1.0], f16), "cheby1")
    with pytest.raises(_lib.AidError, match="GPU only"):
        narrow.predict_bwe_iir_long(y, filt, "cheby1")                       # (order 4: end = 20 >= 8)
    # 6. max_batch, the seeds and, last, the device
    for bad in (0, -2, 1.5, True):
        with pytest.raises(_lib.AidError, match="max_batch"):
            smp.predict_bwe_iir_long(y, filt, "cheby1", max_batch=bad, seeds=[1])
    for bad in ([1], [1, 2, 3]):
        with pytest.raises(_lib.AidError, match="seeds"):
            smp.predict_bwe_iir_long(y, filt, "cheby1", seeds=bad)
    with pytest.raises(_lib.AidError, match="rid"):
        _stub_sampler(rid=True)[0].predict_bwe_iir_long(y, filt, "cheby1")
    with pytest.raises(_lib.AidError, match="seeds"):
        bwe_iir_long.check_bwe_iir_args(y, bwe_iir_long.bwe_iir_prepare(None, filt, "cheby1"), L, end, 8, [1])
    with pytest.raises(_lib.AidError, match="GPU only"):
        bwe_iir_long.check_bwe_iir_args(y, bwe_iir_long.bwe_iir_prepare(None, filt, "cheby1"), L, end, 8, [1, 2])
    assert launched == [] and smp.seeds == [5] and smp.y is None and smp.spectral is None and smp.n_evals == 0
    # the FIR mode still refuses an IIR filter, in one sentence that names the new method
    with pytest.raises(_lib.AidError, match="IIR filter carries state") as e:
        smp.predict_bwe_long(y, filt, "cheby1")
    assert str(e.value).count(". ") == 0 and "predict_bwe_iir_long" in str(e.value)


def test_the_pooled_task_and_the_harness_wrapper():
    from test_bwe_long_host import _stub_sampler
    from audio_inpainting_diffusion_amd import _lib, harness
    smp, L = _stub_sampler()
    filt = scipy.signal.cheby1(4, 0.05, 1000, fs=22050)
    assert "bwe_iir" in smp.POOLED_TASKS
    y = torch.zeros(1, 2 * L)
    for bad in (dict(), dict(filt=filt), dict(filt=filt, filt_type="cheby1", factor=2), dict(factor=2)):
        with pytest.raises(TypeError, match="filt, filt_type"):
            smp.predict_long_pooled("bwe_iir", [y], **bad)
    with pytest.raises(_lib.AidError, match="predict_bwe_long$"):
        smp.predict_long_pooled("bwe_iir", [y], filt=torch.ones(9), filt_type="firwin")
    with pytest.raises(_lib.AidError, match="GPU only"):
        smp.predict_long_pooled("bwe_iir", [y, torch.zeros(2, 3 * L)], filt=filt, filt_type="cheby1", seeds=[1, 2, 3])

    class Rec:
        def __init__(self):
            self.calls = []

        def predict_bwe_iir_long(self, y, filt, filt_type, max_batch=8, seeds=None):
            self.calls.append((tuple(y.shape), filt, filt_type, max_batch, seeds))
            return y + 1

    files = [torch.full((n,), float(k)) for k, n in enumerate((700, 300, 700, 301, 300))]
    rec = Rec()
    out = harness.bwe_iir_long(rec, files, filt, seeds=[10, 11, 12, 13, 14], max_batch=4, device="cpu")
    assert [c[0] for c in rec.calls] == [(2, 700), (2, 300), (1, 301)] and all(c[3] == 4 and c[2] == "cheby1" and c[1] is filt for c in rec.calls)
    assert [c[4] for c in rec.calls] == [[10, 12], [11, 14], [13]] and all(torch.equal(o, f + 1) for o, f in zip(out, files))
    with pytest.raises(ValueError):
        harness.bwe_iir_long(rec, files, filt, seeds=[1], device="cpu")


def test_the_new_entries_ride_on_the_existing_structs():
    from audio_inpainting_diffusion_amd import _lib
    abi = next(a for a in _lib.ABIS if a.header == "aid_bwe_long.h")
    assert abi.version == 1 and set(abi.structs.values()) == {_lib.FirObservedParams, _lib.BweGatherParams}
    assert abi.launches["aid_iir_observed"] is _lib.FirObservedParams and abi.launches["aid_iir_gather"] is _lib.BweGatherParams
    assert abi.launches["aid_fir_observed"] is _lib.FirObservedParams and abi.launches["aid_bwe_gather"] is _lib.BweGatherParams
    assert all(hasattr(_lib.lib(), name) for name in ("aid_iir_observed", "aid_iir_gather"))
