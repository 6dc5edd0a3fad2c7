"""CPU tests (no GPU) of the restoration metrics (metrics.py, harness.evaluate_long): the float64 restatements against closed forms, the
counted-frame rule, band -> bins, the refusals that need no GPU, evaluate_long over a stub, and the two entry points in the ABI table.
Also the shapes, inputs, regions and bands that tests/test_gpu_metrics.py runs the kernels on, and the yardstick it holds them to."""
import math

import numpy as np
import pytest
import torch

FS = 22050
# (n_fft, hop, L, B): one frame that is also the trailing-frame case; hop 1; three items in rows of a wider buffer; L < n_fft; hop | L; the
# default sizes; the largest n_fft (the 146-KB LDS launch)
SHAPES = [(16, 16, 16, 1), (16, 1, 40, 2), (64, 16, 1000, 3), (64, 48, 63, 1), (256, 64, 2048, 2), (2048, 512, 5000, 2), (8192, 2048, 9000, 1)]
REGIONS = ("none", "run", "one", "empty")
BANDS = ("all", "one", "low", "high")


def signals(n_fft, hop, L, B):
    """(ref, est) float32 [B, L]: seeded white noise and ref + 0.1 * noise.  Every bin of every frame then sits within a few tens of dB of the
    frame's peak, so the logarithm does not magnify the fp32 rounding of an FFT at empty bins: a condition on the INPUTS of these tests, not on
    the kernel (an fp32 FFT leaves a rounding floor some 140 dB under the frame's peak, whatever code computes it)."""
    g = torch.Generator().manual_seed(1000 * n_fft + L)
    ref = torch.randn(B, L, generator=g)
    return ref, ref + 0.1 * torch.randn(B, L, generator=g)


def region(kind, n_fft, hop, L, B):
    """none: no weights; run: one run of samples that starts and ends inside frames (off the hop grid where there is one); one: one sample;
    empty: the run, but no sample at all for item 0"""
    if kind == "none":
        return None
    off = lambda q: q + 1 if hop > 1 and q % hop == 0 else q                                # noqa: E731
    w = torch.zeros(B, L)
    if kind == "one":
        w[:, off(L // 2)] = 1.0
    else:
        w[:, off(L // 3 + 1):off(2 * L // 3 + 2)] = 1.0
        if kind == "empty":
            w[0] = 0.0
    return w


def band(kind, n_fft):
    """(k_lo, k_hi): every bin; one bin; from bin 0; up to bin n_fft / 2"""
    return {"all": (0, n_fft // 2), "one": (n_fft // 4 + 1,) * 2, "low": (0, n_fft // 4), "high": (n_fft // 4 + 1, n_fft // 2)}[kind]


# The yardstick of the frame distances in tests/test_gpu_metrics.py.  FP32_REL[band] is the largest relative distance, over all SHAPES and all
# counted frames, between metrics.logspec_dist_host(dtype=numpy.float32) -- the same formula in single precision through torch.stft on the CPU
# -- and the float64 restatement, on ``signals``; measured by ``fp32_yardstick`` below and rounded up to two digits.  The kernel is another
# fp32 FFT with another order of operations and has no claim to be closer: it gets KERNEL_FACTOR times that, relative to the float64 value.
# (Measured: all 4.524e-5, one 2.054e-4, low 1.714e-5, high 4.558e-5.  The one-bin band has the widest bar: a single |log10 R - log10 E| can be
# small by chance, and the same absolute error is then a larger share of it.  The figures are set by the few frames in which a bin of white
# noise happens to be nearly empty.)  Never derived from the kernel's output.
FP32_REL = {"all": 4.6e-5, "one": 2.1e-4, "low": 1.8e-5, "high": 4.6e-5}
KERNEL_FACTOR = 4.0


def fp32_yardstick(kind):
    from audio_inpainting_diffusion_amd import metrics
    worst = 0.0
    for n_fft, hop, L, B in SHAPES:
        ref, est = signals(n_fft, hop, L, B)
        k_lo, k_hi = band(kind, n_fft)
        want = metrics.logspec_dist_host(ref, est, n_fft=n_fft, hop=hop, k_lo=k_lo, k_hi=k_hi)
        got = metrics.logspec_dist_host(ref, est, n_fft=n_fft, hop=hop, k_lo=k_lo, k_hi=k_hi, dtype=np.float32)
        m = want > 0
        assert np.array_equal(got < 0, want < 0)
        worst = max(worst, float((np.abs(got - want)[m] / want[m]).max()))
    return worst


@pytest.mark.parametrize("kind", BANDS)
def test_the_fp32_restatement_lies_inside_the_bar_the_kernel_gets(kind):
    """the bar is not out of reach of an fp32 evaluation: the one it was measured on passes it (on another FFT library the figure moves a little,
    hence the kernel's bar and not the pinned figure itself)"""
    worst = fp32_yardstick(kind)
    print(f"fp32 torch.stft restatement against float64, band {kind}: largest relative difference {worst:.3e} (pinned {FP32_REL[kind]:.1e})")
    assert worst <= KERNEL_FACTOR * FP32_REL[kind]


def _noise(B, L, seed):
    return torch.randn(B, L, generator=torch.Generator().manual_seed(seed)).double()


# ---- closed forms ----------------------------------------------------------------------------------------------------------------------------
def test_an_estimate_equal_to_the_reference():
    from audio_inpainting_diffusion_amd import metrics
    x = _noise(2, 700, 1)
    m = metrics.evaluate_host(x, x.clone(), sample_rate=FS, n_fft=64, hop=16)
    assert m["lsd"].tolist() == [0.0, 0.0] and m["max_abs_err"].tolist() == [0.0, 0.0]
    assert m["snr_db"].tolist() == [math.inf] * 2 and m["si_sdr_db"].tolist() == [math.inf] * 2
    assert m["n_samples"].tolist() == [700.0] * 2 and m["n_frames"].tolist() == [44.0] * 2        # t * 16 < 700: t = 0 .. 43
    assert all(v.dtype == torch.float64 for v in m.values())


@pytest.mark.parametrize("a", [0.5, 0.25, -2.0])
def test_a_scaled_reference(a):
    """a power of two, so that est = a * ref holds exactly in floating point (3 * x is rounded: see the next test)"""
    from audio_inpainting_diffusion_amd import metrics
    x = _noise(1, 1000, 2)
    m = metrics.evaluate_host(x, a * x, sample_rate=FS, n_fft=128, hop=32, floor=0.0)
    fr = m["lsd_frames"][0]
    assert bool((fr[fr >= 0] - abs(2 * math.log10(abs(a)))).abs().max() <= 1e-12) and int((fr >= 0).sum()) == 32
    assert abs(float(m["lsd"]) - abs(2 * math.log10(abs(a)))) <= 1e-12
    assert float(m["si_sdr_db"]) > 250                                           # +inf, or the float64 rounding of a zero denominator
    assert abs(float(m["snr_db"]) + 20 * math.log10(abs(1 - a))) <= 1e-9
    assert abs(float(m["max_abs_err"]) - abs(1 - a) * float(x.abs().max())) <= 1e-12


def test_si_sdr_from_the_sums_has_a_ceiling_near_150_dB():
    """est = fl(3 x) is a * ref up to one rounding per sample (a true SI-SDR near 320 dB), but sum r^2 sum e^2 - (sum r e)^2 cancels to the last
    bits of float64: the formula cannot tell anything above 2^-52 of the product, about 156 dB, from a perfect match.  Stated, not hidden: lsd,
    snr and max_abs_err are exact to their usual precision here."""
    from audio_inpainting_diffusion_amd import metrics
    x = _noise(1, 1000, 2)
    m = metrics.evaluate_host(x, 3.0 * x, sample_rate=FS, n_fft=128, hop=32, floor=0.0)
    assert float(m["si_sdr_db"]) > 140
    assert abs(float(m["lsd"]) - 2 * math.log10(3.0)) <= 1e-12 and abs(float(m["snr_db"]) + 20 * math.log10(2.0)) <= 1e-9


def test_si_sdr_does_not_change_with_the_scale_of_the_estimate_and_snr_does():
    from audio_inpainting_diffusion_amd import metrics
    x, n = _noise(2, 900, 3), _noise(2, 900, 4)
    e = x + 0.3 * n
    one, two = (metrics.evaluate_host(x, s * e, sample_rate=FS, n_fft=64, hop=32) for s in (1.0, 0.37))
    assert bool((one["si_sdr_db"] - two["si_sdr_db"]).abs().max() <= 1e-9)
    assert bool((one["snr_db"] - two["snr_db"]).abs().min() > 1.0)
    # against the definition through the projection onto the reference: s = <e, x> x / <x, x>, 10 log10(|s|^2 / |e - s|^2)
    s = (e * x).sum(1, keepdim=True) / (x * x).sum(1, keepdim=True) * x
    want = 10 * torch.log10((s * s).sum(1) / ((e - s) ** 2).sum(1))
    assert bool((one["si_sdr_db"] - want).abs().max() <= 1e-9)


def test_sums_over_a_region_are_the_sums_over_its_samples():
    from audio_inpainting_diffusion_amd import metrics
    x, e = _noise(2, 300, 5), _noise(2, 300, 6)
    w = torch.zeros(2, 300)
    w[0, 10:50], w[1, 299], w[0, 200] = 1.0, 2.5, -1.0                           # (any non-zero weight counts, and counts once)
    s = metrics.eval_sums_host(x, e, w, frames=np.array([[-1.0, 0.5, 0.25], [-1.0, -1.0, -1.0]]))
    keep = [list(range(10, 50)) + [200], [299]]
    for b in range(2):
        r, v = x[b, keep[b]].numpy(), e[b, keep[b]].numpy()
        want = [len(keep[b]), (r * r).sum(), (v * v).sum(), (r * v).sum(), ((r - v) ** 2).sum(), np.abs(r - v).max()]
        assert np.allclose(s[b, :6], want, rtol=1e-13, atol=0)
    assert s[:, 6:].tolist() == [[2.0, 0.75], [0.0, 0.0]]
    m = metrics.from_sums(s)
    assert m["lsd"][0] == 0.375 and math.isnan(m["lsd"][1]) and m["n_samples"].tolist() == [41.0, 1.0]


# ---- the counted frames ------------------------------------------------------------------------------------------------------------------
def test_the_trailing_frame_is_dropped_when_hop_divides_the_length():
    from audio_inpainting_diffusion_amd import metrics
    x = _noise(1, 256, 7)
    fr = metrics.logspec_dist_host(x, 0.5 * x, n_fft=64, hop=64)
    assert fr.shape == (1, 5) and (fr[0, :4] > 0).all() and fr[0, 4] == -1.0                      # T = 1 + 256 / 64; frame 4 starts at L
    fr = metrics.logspec_dist_host(x[:, :255], 0.5 * x[:, :255], n_fft=64, hop=64)
    assert fr.shape == (1, 4) and (fr > 0).all()                                                 # 255 = 3 * 64 + 63: every frame holds a sample
    assert metrics.counted_frames_host(None, 1, 16, 16, 16).tolist() == [[True, False]]


def test_a_recording_shorter_than_one_frame_is_one_partly_zero_frame():
    from audio_inpainting_diffusion_amd import metrics
    x = _noise(1, 40, 8)
    fr = metrics.logspec_dist_host(x, 2 * x, n_fft=64, hop=48, floor=0.0)
    assert fr.shape == (1, 1) and abs(fr[0, 0] - 2 * math.log10(2)) <= 1e-12
    m = metrics.evaluate_host(x, 2 * x, sample_rate=FS, n_fft=64, hop=48)
    assert m["n_frames"].tolist() == [1.0] and m["n_samples"].tolist() == [40.0]


@pytest.mark.parametrize("q,want", [(0, [0]), (15, [0]), (16, [0, 1]), (63, [0, 1, 2, 3]), (64, [1, 2, 3, 4]), (100, [3, 4, 5, 6]), (199, [9, 10, 11, 12])])
def test_a_region_of_one_sample_counts_exactly_the_frames_that_cover_it(q, want):
    """n_fft 64, hop 16, L 200: frame t covers [16 t, 16 t + 64), t <= 12"""
    from audio_inpainting_diffusion_amd import metrics
    w = torch.zeros(200)
    w[q] = 1.0
    x = _noise(1, 200, 9)
    fr = metrics.logspec_dist_host(x, x + 0.1 * _noise(1, 200, 10), w, n_fft=64, hop=16)
    assert np.nonzero(fr[0] >= 0)[0].tolist() == want == [t for t in range(13) if 16 * t <= q < 16 * t + 64]
    assert (fr[0][fr[0] < 0] == -1.0).all()


def test_an_empty_region_is_an_answer():
    from audio_inpainting_diffusion_amd import metrics
    x = _noise(2, 200, 11)
    w = torch.zeros(2, 200)
    w[1, 50:60] = 1.0
    m = metrics.evaluate_host(x, x + 0.1, w, sample_rate=FS, n_fft=64, hop=16)
    assert m["n_frames"].tolist() == [0.0, 4.0] and m["n_samples"].tolist() == [0.0, 10.0]
    assert math.isnan(m["lsd"][0]) and math.isnan(m["snr_db"][0]) and math.isnan(m["si_sdr_db"][0]) and math.isnan(m["max_abs_err"][0])
    assert math.isfinite(m["lsd"][1]) and abs(float(m["max_abs_err"][1]) - 0.1) < 1e-14
    assert bool((m["lsd_frames"][0] == -1).all())


# ---- band -> bins ----------------------------------------------------------------------------------------------------------------------------
def test_band_to_bins_at_the_edges():
    from audio_inpainting_diffusion_amd import metrics
    bb = lambda lo, hi, n=2048, fs=FS: metrics.band_bins((lo, hi), fs, n)                         # noqa: E731
    assert metrics.band_bins(None, FS, 2048) == (0, 1024) and metrics.band_bins(None, None, 16) == (0, 8)
    assert bb(0, FS / 2) == (0, 1024) and bb(0, 0) == (0, 0) and bb(FS / 2, FS / 2) == (1024, 1024)
    hz = FS / 2048                                                                               # the distance of two bin centres
    assert bb(3 * hz, 3 * hz) == (3, 3)                                                          # k_lo == k_hi: a centre is inside its own band
    assert bb(3 * hz, 7 * hz) == (3, 7) and bb(3 * hz + 1e-6, 7 * hz - 1e-6) == (4, 6) and bb(2.5 * hz, 3.5 * hz) == (3, 3)
    assert bb(3000, FS / 2) == (279, 1024)                                                       # 3000 / 10.7666 = 278.6
    assert bb(1000, 2000, 16, 16000) == (1, 2) and bb(1000, 1000, 16, 16000) == (1, 1)           # bins 1000 Hz apart
    assert metrics.region_of("bwe", cutoff_hz=3000, sample_rate=FS) == (None, (3000.0, FS / 2))


def test_bands_and_sizes_that_are_refused_say_why():
    from audio_inpainting_diffusion_amd import _lib, metrics
    for bad, why in (((-1, 100), "inside"), ((0, FS / 2 + 1), "inside"), ((200, 100), "lo_hz above"), ((1, 2), "no bin centre"),
                     ((float("nan"), 5), "inside"), ("ab", "band must be"), ((1, 2, 3), "band must be")):
        with pytest.raises(_lib.AidError, match=why):
            metrics.band_bins(bad, FS, 2048)
    with pytest.raises(_lib.AidError, match="sample_rate"):
        metrics.band_bins((0, 1), 0, 2048)
    x = _noise(1, 100, 12)
    for kw, why in ((dict(n_fft=48), "power of two"), (dict(n_fft=16384), "power of two"), (dict(n_fft=64, hop=65), "hop"), (dict(n_fft=64, hop=0), "hop"),
                    (dict(floor=-1.0), "floor"), (dict(floor=float("inf")), "floor"), (dict(window="hamming"), "hann"), (dict(band=(0, FS)), "inside")):
        with pytest.raises(_lib.AidError, match=why):
            metrics.evaluate_host(x, x, **dict(dict(sample_rate=FS, n_fft=64, hop=16), **kw))
    with pytest.raises(_lib.AidError, match="differ in shape"):
        metrics.evaluate_host(x, x[:, :99], sample_rate=FS, n_fft=64, hop=16)
    with pytest.raises(_lib.AidError, match="region must be"):
        metrics.evaluate_host(x, x, torch.ones(2, 100), sample_rate=FS, n_fft=64, hop=16)
    with pytest.raises(_lib.AidError, match="k_lo <= k_hi"):
        metrics.logspec_dist_host(x, x, n_fft=64, hop=16, k_lo=3, k_hi=33)


def test_evaluate_refuses_what_is_not_on_the_gpu_or_does_not_match_before_anything_is_launched():
    from audio_inpainting_diffusion_amd import _lib, metrics
    x = _noise(2, 100, 13).float()
    with pytest.raises(_lib.AidError, match="on the GPU"):
        metrics.evaluate(x, x, sample_rate=FS)
    with pytest.raises(_lib.AidError, match="on the GPU"):
        metrics.evaluate(x.numpy(), x, sample_rate=FS)
    with pytest.raises(_lib.AidError, match="inside"):                                           # (the settings are checked first)
        metrics.evaluate(x, x, sample_rate=FS, band=(0, FS))
    with pytest.raises(_lib.AidError, match="power of two"):
        metrics.evaluate(x, x, sample_rate=FS, n_fft=100)


def test_the_region_of_every_mode():
    from audio_inpainting_diffusion_amd import _lib, metrics
    mask = torch.ones(1, 10)
    mask[0, 3:6] = 0
    w, b = metrics.region_of("inpainting", mask=mask)
    assert b is None and w.tolist() == [[0, 0, 0, 1, 1, 1, 0, 0, 0, 0]]
    y = torch.tensor([[0.1, -0.5, 0.5, 0.49], [0.2, 0.1, -0.3, 0.0]])
    w, b = metrics.region_of("declipping", y=y, clip_value=0.5)
    assert b is None and w.tolist() == [[0, 1, 1, 0], [0, 0, 0, 0]]
    w, _ = metrics.region_of("declipping", y=y, clip_value=[0.5, 0.2])
    assert w.tolist() == [[0, 1, 1, 0], [1, 0, 1, 0]]
    for task in ("spectrogram_inpainting", "pr", "compsens"):
        assert metrics.region_of(task) == (None, None)
    for task, kw, why in (("bwe_declip", {}, "out of scope"), ("inpainting", {}, "mask="), ("bwe", dict(cutoff_hz=1), "sample_rate="),
                          ("pr", dict(mask=mask), "no keyword"), ("declipping", dict(y=y, clip_value=[1, 2, 3]), "one per recording"),
                          ("declipping", dict(y=y, clip_value=0.0), "above 0")):
        with pytest.raises(_lib.AidError, match=why):
            metrics.region_of(task, **kw)


# ---- evaluate_long over a stub -----------------------------------------------------------------------------------------------------------------
def test_evaluate_long_groups_by_length_keeps_the_order_and_counts_what_is_not_finite():
    from audio_inpainting_diffusion_amd import harness, metrics
    lengths = [300, 500, 300, 40, 500, 300]
    refs = [_noise(1, n, 20 + i).float().reshape(-1) for i, n in enumerate(lengths)]
    ests = [r + 0.05 * (i + 1) for i, r in enumerate(refs)]
    ests[3] = refs[3].clone()                                                                    # snr and si_sdr +inf
    regions = [None, None, torch.zeros(300), None, None, None]                                   # file 2: an empty region: every metric nan
    regions[5] = torch.zeros(300)
    regions[5][7] = 3.0
    calls = []

    def stub(r, e, w, **kw):
        calls.append((tuple(r.shape), None if w is None else w.sum(1).tolist(), kw))
        return metrics.evaluate_host(r, e, w, **kw)
    rows, summary = harness.evaluate_long(refs, ests, regions, device="cpu", evaluate=stub, sample_rate=FS, n_fft=64, hop=16)
    # one call per length, in the order the lengths first appear; a missing region in a group with one is all ones, a group without any passes None
    assert [(c[0], c[1]) for c in calls] == [((3, 300), [300.0, 0.0, 1.0]), ((2, 500), None), ((1, 40), None)]
    assert all(c[2] == dict(sample_rate=FS, n_fft=64, hop=16) for c in calls)
    assert [row["index"] for row in rows] == list(range(6)) and [row["n"] for row in rows] == lengths
    for i, row in enumerate(rows):                                                               # each row is that file evaluated alone
        alone = metrics.evaluate_host(refs[i], ests[i], regions[i], sample_rate=FS, n_fft=64, hop=16)
        for k in ("lsd", "snr_db", "si_sdr_db", "max_abs_err", "n_samples", "n_frames"):
            a, b = row[k], float(alone[k][0])
            assert (math.isnan(a) and math.isnan(b)) or a == b, (i, k, a, b)
    assert rows[5]["n_samples"] == 1.0 and abs(rows[5]["max_abs_err"] - 0.3) < 1e-6 and rows[2]["n_samples"] == 0.0
    assert summary["n_files"] == 6
    assert summary["lsd"]["n_not_finite"] == 1 and summary["max_abs_err"]["n_not_finite"] == 1   # file 2
    assert summary["snr_db"]["n_not_finite"] == 2                                                # files 2 (nan) and 3 (+inf)
    # file 5 is one sample: est = a * ref over it, so si_sdr is +inf there as well
    assert summary["si_sdr_db"]["n_not_finite"] in (2, 3)                                        # (or the float64 rounding of a zero denominator)
    finite = sorted(rows[i]["snr_db"] for i in (0, 1, 4, 5))
    assert abs(summary["snr_db"]["mean"] - sum(finite) / 4) < 1e-12 and abs(summary["snr_db"]["median"] - (finite[1] + finite[2]) / 2) < 1e-12
    with pytest.raises(ValueError, match="file 1 "):
        harness.evaluate_long(refs, ests[:1] + [ests[0]] + ests[2:], device="cpu", evaluate=stub, sample_rate=FS)
    with pytest.raises(ValueError, match="5 estimates"):
        harness.evaluate_long(refs, ests[:5], device="cpu", evaluate=stub, sample_rate=FS)


# ---- the ABI table ---------------------------------------------------------------------------------------------------------------------------
def test_the_two_entry_points_ride_on_existing_parameter_blocks():
    from audio_inpainting_diffusion_amd import _lib
    abi = {a.header: a for a in _lib.ABIS}
    assert abi["aid_phase_long.h"].launches["aid_stft_logspec_dist"] is _lib.StftMagObservedParams
    assert abi["aid_bwe_long.h"].launches["aid_eval_sums"] is _lib.FirObservedParams
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in ("aid_stft_logspec_dist", "aid_eval_sums"))
