"""Host tests (no GPU) of declicking (audio_inpainting_diffusion_amd/declick.py): the refusals of the settings, the float64 restatements
against cases worked by hand, the run rules, the dilation, the report, add_clicks, and -- through the stub sampler of
test_long_tasks_host.py -- that predict_declicking_long is a front end of predict_inpainting_long and registers nothing."""
import numpy as np
import pytest
import torch


def _dk():
    from audio_inpainting_diffusion_amd import declick
    return declick


def signal(N, seed, R=1):
    """four partials plus coloured noise, float32 [R, N]: what a clean recording looks like to the detector"""
    rng = np.random.default_rng(seed)
    t = np.arange(N)
    out = []
    for _ in range(R):
        x = sum(a * np.sin(2 * np.pi * f * t / 22050 + rng.uniform(0, 6.28)) for a, f in ((0.3, 220.0), (0.2, 440.0), (0.1, 1330.0), (0.05, 3100.0)))
        w = rng.standard_normal(N + 2)
        out.append(x + 0.005 * (w[2:] + 0.9 * w[1:-1] + 0.4 * w[:-2]))
    return np.stack(out).astype(np.float32)


# ---- settings ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad, word", [
    (dict(block=1000), "block"), (dict(block=8192), "block"), (dict(block=True), "block"), (dict(order=0), "order"), (dict(order=33), "order"),
    (dict(order=2.5), "order"), (dict(block=256, order=33), "order"), (dict(threshold=0), "threshold"),
    (dict(threshold=-1.0), "threshold"), (dict(threshold=float("nan")), "threshold"), (dict(threshold=float("inf")), "threshold"),
    (dict(pad=-1), "pad"), (dict(pad=257), "pad"), (dict(pad=1.5), "pad"), (dict(min_run=1), "min_run"), (dict(min_run=-2), "min_run"),
    (dict(min_run=9, max_run=8), "min_run"), (dict(max_run=1025), "max_run"), (dict(max_run=0), "max_run"), (dict(ridge=-1e-9), "ridge"),
    (dict(ridge=float("inf")), "ridge"), (dict(sigma_floor=0), "sigma_floor"), (dict(sigma_floor=1e-60), "sigma_floor"),
    (dict(max_fraction=-0.1), "max_fraction"), (dict(max_fraction=1.5), "max_fraction"), (dict(blok=256), "unknown setting blok")])
def test_every_setting_outside_its_range_is_refused_by_name(bad, word):
    from audio_inpainting_diffusion_amd import _lib
    with pytest.raises(_lib.AidError, match=word):
        _dk().make_settings(**bad)


def test_defaults_and_settings_of_read_the_config_node():
    from audio_inpainting_diffusion_amd.config import small_args
    dk = _dk()
    s = dk.make_settings()
    assert (s.block, s.order, s.threshold, s.pad, s.min_run, s.max_run, s.max_fraction) == (2048, 16, 8.0, 16, 8, 1024, 0.2)
    assert s.ridge == float(np.float32(1e-6)) == s.sigma_floor                    # (rounded to float32 once: the kernels take floats)
    assert dk.make_settings(block=256, order=32).order == 32 and dk.make_settings(min_run=0).min_run == 0 and dk.make_settings(pad=256).pad == 256
    args = small_args()
    assert dk.settings_of(args) == s
    assert dk.settings_of(args, pad=3).pad == 3
    args.tester.declicking = {"block": 512, "threshold": 6.0, "pad": None}
    got = dk.settings_of(args)
    assert (got.block, got.threshold, got.pad) == (512, 6.0, 16) and dk.settings_of(args, block=1024).block == 1024
    args.tester.declicking = {"order": 40}
    from audio_inpainting_diffusion_amd import _lib
    with pytest.raises(_lib.AidError, match="order"):
        dk.settings_of(args)


# ---- the score -----------------------------------------------------------------------------------------------------------------------------------
def test_order_one_has_the_closed_form():
    dk = _dk()
    y = signal(256, 1)
    x = y[0].astype(np.float64)
    r0, r1 = float(np.cumsum(x * x)[-1]) * (1.0 + float(np.float32(1e-6))), float(np.cumsum(x[1:] * x[:-1])[-1])
    a1 = -r1 / r0
    assert np.array_equal(dk.levinson_host([r0, r1], 1), np.array([1.0, a1]))
    e = np.abs(x + a1 * np.concatenate([[0.0], x[:-1]]))
    med = np.sort(e[1:])[255 // 2]
    s, sigma = dk.score_host(y, block=256, order=1)
    assert float(sigma[0, 0]) == med / 0.6745 and s[0, 0] == 0
    assert np.array_equal(s.numpy()[0, 1:], (e[1:] / (med / 0.6745)).astype(np.float32))


def test_an_exact_ar2_sequence_leaves_sigma_at_the_floor_and_flags_the_one_outlier():
    dk = _dk()
    # the impulse response of 1 / (1 - 1.5 z^-1 + 0.5625 z^-2), from the first sample of the recording (zeros before it) and decayed to
    # nothing inside the block: the sums of the block are the sums over all time, so the fit is the recursion itself, up to the float32
    # rounding of the samples
    x = np.zeros(256)
    x[0], x[1] = 1.0, 1.5
    for i in range(2, 256):
        x[i] = 1.5 * x[i - 1] - 0.5625 * x[i - 2]
    y = x.astype(np.float32).reshape(1, -1)
    r = [float(np.cumsum(x[m:] * x[:256 - m])[-1]) for m in range(3)]
    assert np.allclose(dk.levinson_host(r, 2), [1.0, -1.5, 0.5625], atol=1e-12)
    s, sigma = dk.score_host(y, block=256, order=2, ridge=0.0, sigma_floor=1e-3)
    assert sigma.shape == (1, 1) and float(sigma[0, 0]) == float(np.float32(1e-3))                           # residual ~1e-7: the floor holds
    assert float(s.max()) < 1e-2
    y[0, 100] += 0.25
    s, sigma = dk.score_host(y, block=256, order=2, ridge=0.0, sigma_floor=1e-3)
    hit = np.flatnonzero(s.numpy()[0] > 8)
    assert {100, 101, 102} <= set(hit.tolist()) and s[0, 100] > 100 and float(sigma[0, 0]) == float(np.float32(1e-3))


def test_silent_short_and_first_samples():
    dk = _dk()
    y = signal(1000, 2)
    y[0, 256:512] = 0.0                                                              # a silent block: r[0] = 0
    s, sigma = dk.score_host(y, block=256, order=8)
    assert sigma.shape == (1, 4) and sigma[0, 1] == 0 and not s[0, 256:512].any()
    assert sigma[0, 0] > 0 and sigma[0, 2] > 0 and sigma[0, 3] > 0                   # the tail of 232 >= 64 samples is scored
    assert not s[0, :8].any() and s[0, 8] > 0                                        # the first ``order`` samples of the recording are not
    assert s[0, 512] > 0                                                             # ... those of a later block are
    s, sigma = dk.score_host(y[:, :300], block=256, order=8)                         # a tail of 44 < 64: not scored
    assert sigma[0, 1] == 0 and not s[0, 256:].any() and sigma[0, 0] > 0
    s, sigma = dk.score_host(y[:, :200], block=256, order=8)                         # N < block
    assert sigma.shape == (1, 1) and sigma[0, 0] > 0 and s[0, 8:].min() >= 0 and s[0, 100] > 0
    s, sigma = dk.score_host(y[:, :63], block=256, order=8)                          # N < 8 order: nothing is scored
    assert sigma[0, 0] == 0 and not s.any()


def test_history_comes_from_the_previous_block_and_the_median_has_rank_n_half():
    dk = _dk()
    y = signal(512, 3)
    s, sigma = dk.score_host(y, block=256, order=8)
    # block 1 alone, as a recording of its own, has zeros for history and leaves its first 8 samples unscored: the scores differ there
    s1, sigma1 = dk.score_host(y[:, 256:], block=256, order=8)
    assert not np.array_equal(s.numpy()[0, 256:264], s1.numpy()[0, :8]) and (s.numpy()[0, 256:264] > 0).all()
    # the median: rank n' // 2 of the scored |e|; score * sigma gives |e| back
    e = s.numpy()[0, 256:].astype(np.float64) * float(sigma[0, 1])
    assert abs(np.sort(e)[128] / 0.6745 / float(sigma[0, 1]) - 1) < 1e-6
    e0 = s.numpy()[0, 8:256].astype(np.float64) * float(sigma[0, 0])
    assert abs(np.sort(e0)[248 // 2] / 0.6745 / float(sigma[0, 0]) - 1) < 1e-6
    # a clean signal stays far below the threshold, a click does not
    assert float(s.max()) < 6
    y[0, 400] += 0.3
    assert dk.score_host(y, block=256, order=8)[0][0, 400] > 8


def test_the_two_summation_orders_agree_to_rounding():
    dk = _dk()
    y = signal(1000, 4)
    a, b = dk.score_host(y, block=256, order=8)[0].double(), dk.score_host(y, block=256, order=8, autocorr="pairwise")[0].double()
    big = a >= 1
    assert float(((a - b).abs() / a)[big].max()) < 1e-6 and not torch.equal(dk.score_host(y, block=256, order=8)[1],
                                                                            dk.score_host(y, block=256, order=8, autocorr="pairwise")[1])


# ---- the flags and the mask ----------------------------------------------------------------------------------------------------------------------
def _ramp(N):
    """no two neighbours equal"""
    return (np.arange(N, dtype=np.float32) % 7 + 1).reshape(1, -1) * np.float32(0.01) + (np.arange(N, dtype=np.float32).reshape(1, -1) % 2)


def test_run_rules():
    dk = _dk()
    N = 3000
    zero = np.zeros((1, N), dtype=np.float32)
    for length, want in ((3, False), (4, True), (1024, True), (1025, False)):          # min_run - 1, min_run, max_run, max_run + 1
        y = _ramp(N)
        y[0, 500:500 + length] = 0.125
        f = dk.flags_host(y, zero, threshold=8.0, min_run=4, max_run=1024)
        assert f[0, 500:500 + length].all() == want and f.sum() == (length if want else 0), length
    y = _ramp(N)
    y[0, :10] = 0.5                                                                    # touches the start
    y[0, N - 10:] = 0.25                                                               # touches the end
    y[0, 100:110] = -0.0                                                               # bits, not values: -0.0 and +0.0 are two runs
    y[0, 110:120] = 0.0
    f = dk.flags_host(y, zero, threshold=8.0, min_run=8, max_run=1024)
    assert not f[0, :10].any() and not f[0, N - 10:].any() and f[0, 100:120].all() and f.sum() == 20
    assert dk.flags_host(y, zero, threshold=8.0, min_run=11, max_run=1024).sum() == 0
    assert dk.flags_host(y, zero, threshold=8.0, min_run=0, max_run=1024).sum() == 0   # no run rule
    one = np.full((1, 1), 0.5, dtype=np.float32)
    assert dk.mask_host(one, np.zeros((1, 1), dtype=np.float32)).tolist() == [[1.0]]   # N = 1: a run at both ends


def test_the_threshold_compares_float32_with_float32():
    dk = _dk()
    y = _ramp(8)
    thr = np.float32(8.0)
    s = np.array([[0, thr, np.nextafter(thr, np.float32(9)), 0, 0, 0, 0, 0]], dtype=np.float32)
    assert dk.flags_host(y, s, threshold=8.0, min_run=0)[0].tolist() == [False, False, True, False, False, False, False, False]


def test_dilation():
    dk = _dk()
    N, pad = 200, 5
    y = _ramp(N)

    def m(at, pad=pad):
        s = np.zeros((1, N), dtype=np.float32)
        s[0, list(at)] = 9.0
        return dk.mask_host(y, s, threshold=8.0, pad=pad, min_run=0).numpy()[0]
    assert np.flatnonzero(m([0]) == 0).tolist() == list(range(0, 6))                    # clamped at q = 0
    assert np.flatnonzero(m([N - 1]) == 0).tolist() == list(range(N - 6, N))            # ... and at q = N - 1
    assert np.flatnonzero(m([50], pad=0) == 0).tolist() == [50]                         # pad 0
    assert np.flatnonzero(m([50]) == 0).tolist() == list(range(45, 56))                 # the pad edge is inside: |q - 50| <= pad
    two = m([50, 50 + 2 * pad])                                                         # 2 pad apart: one gap
    assert np.flatnonzero(two == 0).tolist() == list(range(45, 66))
    two = m([50, 50 + 2 * pad + 1])                                                     # 2 pad + 1 apart: the gaps touch, still one
    assert np.flatnonzero(two == 0).tolist() == list(range(45, 67))
    two = m([50, 50 + 2 * pad + 2])                                                     # 2 pad + 2 apart: one observed sample between
    assert np.flatnonzero(two == 0).tolist() == list(range(45, 56)) + list(range(57, 68)) and two[56] == 1
    assert dk.mask_host(y, np.zeros((1, N), dtype=np.float32)).dtype == torch.float32


def test_report_counts():
    dk = _dk()
    m = torch.ones(3, 50)
    m[0, 0:3] = 0
    m[0, 10:11] = 0
    m[0, 40:50] = 0
    m[2, :] = 0
    n, g, lg = dk.report_of(m)
    assert n.tolist() == [14, 0, 50] and g.tolist() == [3, 0, 1] and lg.tolist() == [10, 0, 50] and n.dtype == torch.int64


def test_detect_host_on_damaged_signal_finds_all_of_it():
    dk = _dk()
    x = signal(5000, 5, R=2)
    clean = dk.detect_host(x)
    assert clean.n_flagged.tolist() == [0, 0] and bool((clean.mask == 1).all())
    y, truth = dk.add_clicks(x, 12, seed=7, dropouts=1)
    det = dk.detect_host(y)
    sc = dk.detection_scores(det.mask, truth, pad=16)
    # (a click rings on in the residual for ``order`` samples after it, and those are flagged and padded too: precision stays below 1)
    assert sc["recall"] == 1.0 and 0.85 < sc["precision"] <= 1.0
    assert (det.n_gaps >= 1).all() and (det.n_flagged.numpy() == (det.mask.numpy() == 0).sum(axis=1)).all() and float(det.n_flagged.sum()) / y.size < 0.2


def test_add_clicks_is_reproducible_by_seed_and_marks_what_it_touched():
    dk = _dk()
    x = signal(4000, 6, R=2)
    y1, t1 = dk.add_clicks(x, 20, seed=3, dropouts=2)
    y2, t2 = dk.add_clicks(x, 20, seed=3, dropouts=2)
    y3, t3 = dk.add_clicks(x, 20, seed=4, dropouts=2)
    assert np.array_equal(y1, y2) and np.array_equal(t1, t2) and not np.array_equal(t1, t3)
    assert y1.dtype == np.float32 and t1.dtype == bool and y1.shape == x.shape and np.array_equal(y1[~t1], x[~t1]) and (y1[t1] != x[t1]).mean() > 0.9
    assert not t1[:, 0].any() and not t1[:, -1].any() and 20 <= t1[0].sum() <= 20 * 5 + 2 * 64
    yt, tt = dk.add_clicks(torch.from_numpy(x[0]), 20, seed=3)
    assert torch.is_tensor(yt) and yt.shape == (4000,) and tt.dtype == torch.bool


# ---- the front end ---------------------------------------------------------------------------------------------------------------------------------
def _stubbed(monkeypatch):
    """the stub sampler with declick.detect restated on the host and predict_inpainting_long recording its calls"""
    from test_long_tasks_host import _sampler
    from audio_inpainting_diffusion_amd import _lib
    dk = _dk()
    launched, calls = [], []
    monkeypatch.setattr(_lib, "call", lambda name, p: launched.append(name))
    monkeypatch.setattr(dk, "detect", lambda y, **kw: dk.detect_host(y, **kw))
    smp, L = _sampler()
    monkeypatch.setattr(smp, "predict_inpainting_long", lambda y, mask, max_batch=8, seeds=None: (calls.append((y, mask, max_batch, seeds)), y.clone())[1])
    return smp, L, launched, calls


def test_predict_declicking_long_calls_predict_inpainting_long_once_with_the_combined_mask(monkeypatch):
    dk = _dk()
    smp, L, launched, calls = _stubbed(monkeypatch)
    y, truth = dk.add_clicks(torch.from_numpy(signal(5000, 5, R=2)), 12, seed=7)
    out = smp.predict_declicking_long(y, max_batch=3, seeds=[4, 5])
    det = dk.detect_host(y)
    assert len(calls) == 1 and calls[0][0] is y and torch.equal(calls[0][1], det.mask) and calls[0][2:] == (3, [4, 5]) and torch.equal(out, y)
    rep = smp.declick_report
    assert rep.score is None and torch.equal(rep.mask, det.mask) and rep.n_flagged.tolist() == det.n_flagged.tolist() and torch.equal(rep.sigma, det.sigma)
    known = torch.ones(5000)
    known[1000:1100] = 0
    smp.predict_declicking_long(y, mask=known, pad=4)
    want = dk.detect_host(y, pad=4).mask * known
    assert len(calls) == 2 and torch.equal(calls[1][1], want) and torch.equal(smp.declick_report.mask, want) and calls[1][2:] == (8, None)
    assert [c.tolist() for c in smp.declick_report[3:]] == [c.tolist() for c in dk.report_of(want)]     # the counts are the combined mask's
    assert smp.declick_report.longest_gap.min() >= 100
    assert launched == []


def test_predict_declicking_long_launches_nothing_when_nothing_is_flagged(monkeypatch):
    smp, L, launched, calls = _stubbed(monkeypatch)
    y = torch.from_numpy(signal(3000, 8))
    monkeypatch.undo()                                                                   # the real predict_inpainting_long from here on ...
    from audio_inpainting_diffusion_amd import _lib, restore
    dk = _dk()
    monkeypatch.setattr(_lib, "call", lambda name, p: launched.append(name))
    monkeypatch.setattr(dk, "detect", lambda y, **kw: dk.detect_host(y, **kw))
    monkeypatch.setattr(restore, "check_batch", lambda *a, **k: None)                    # ... but for its refusal of host tensors
    monkeypatch.setattr(smp, "_check_model", lambda: None)
    n = smp.n_evals
    out = smp.predict_declicking_long(y)
    assert torch.equal(out, y) and out.data_ptr() != y.data_ptr() and smp.n_evals == n and launched == []
    assert smp.declick_report.n_flagged.tolist() == [0]


def test_predict_declicking_long_refuses_on_max_fraction_before_anything_else(monkeypatch):
    from audio_inpainting_diffusion_amd import _lib
    dk = _dk()
    smp, L, launched, calls = _stubbed(monkeypatch)
    y, _ = dk.add_clicks(torch.from_numpy(signal(5000, 5, R=2)), 12, seed=7)
    y[1], _ = dk.add_clicks(y[1], 300, seed=9)
    smp.rid = True                                                                       # (what predict_inpainting_long would refuse first)
    with pytest.raises(_lib.AidError, match=r"recording 1: \d+ of 5000 samples .* max_fraction = 0.2"):
        smp.predict_declicking_long(y)
    known = torch.ones(2, 5000)
    known[0, :1500] = 0
    with pytest.raises(_lib.AidError, match=r"recording 0: \d+ of 5000"):
        smp.predict_declicking_long(y, mask=known, max_fraction=0.25)
    with pytest.raises(_lib.AidError, match="unknown setting"):
        smp.predict_declicking_long(y, treshold=3)
    assert calls == [] and launched == []
    smp.predict_declicking_long(y, max_fraction=1.0)
    assert len(calls) == 1


def test_the_device_front_end_refuses_host_tensors_and_bad_settings_before_any_launch(monkeypatch):
    from audio_inpainting_diffusion_amd import _lib
    dk = _dk()
    launched = []
    monkeypatch.setattr(_lib, "call", lambda name, p: launched.append(name))
    y = torch.zeros(1, 100)
    for call in (lambda: dk.score(y), lambda: dk.mask(y, y), lambda: dk.detect(y)):
        with pytest.raises(_lib.AidError, match="on the GPU"):
            call()
    with pytest.raises(_lib.AidError, match="block"):
        dk.detect(y, block=100)
    assert launched == []


def test_declicking_registers_no_task():
    from audio_inpainting_diffusion_amd import metrics, restore
    from audio_inpainting_diffusion_amd.sampler import Sampler
    before = (tuple(restore.LONG_TASKS), Sampler.POOLED_TASKS, metrics.TASKS)
    import audio_inpainting_diffusion_amd.declick  # noqa: F401
    assert (tuple(restore.LONG_TASKS), Sampler.POOLED_TASKS, metrics.TASKS) == before
    assert "declicking" not in restore.LONG_TASKS and hasattr(Sampler, "predict_declicking_long")
    from audio_inpainting_diffusion_amd import _lib
    bwe = next(a for a in _lib.ABIS if a.header == "aid_bwe_long.h")
    assert bwe.launches["aid_ar_score"] is _lib.BweGatherParams and bwe.launches["aid_click_mask"] is _lib.FirObservedParams
