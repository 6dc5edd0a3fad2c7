"""CPU tests (no GPU) of blind bandwidth extension (blind.py, Sampler.predict_blind_bwe): the float64 restatements of the statistics, the fit
and the tap design -- recovery of a model filter, the tie rule, empty inputs, two windowed-sinc low-passes and a Chebyshev on a noise-free
signal -- the refusals, all raised before anything touches a GPU, and the three entry points in the ABI table."""
import functools

import numpy as np
import pytest
import scipy.signal
import torch

FS = 22050
SMALL = dict(n_fft=256, hop=64, K=127)                      # the settings of the signal cases: integer-bin cut-offs from k_lo to F - 1


def small_settings(**kw):
    from audio_inpainting_diffusion_amd import blind
    cfg = dict(SMALL, cutoffs=np.arange(2, SMALL["n_fft"] // 2 + 1))
    cfg.update(kw)
    return blind.make_settings(**cfg)


def source(L=8192, seed=0):
    """Gaussian noise through [1, 0.9], times 0.05: a spectrum that falls towards Nyquist, as music does"""
    e = np.random.default_rng(seed).standard_normal(L + 1)
    return 0.05 * (e[1:] + 0.9 * e[:-1])


def same_filter(x, h):
    """sum_k h[k] x[i + k - P], P = (K - 1) // 2, zeros outside (conv1d padding="same"), float64"""
    K = len(h)
    P = (K - 1) // 2
    return np.correlate(np.concatenate([np.zeros(P), x, np.zeros(K - 1 - P)]), h, mode="valid")


@functools.lru_cache(maxsize=None)
def sinc_case(fc, seed=0):
    """(x, y): the source and its low-passed copy through a 101-tap Hamming windowed sinc at fc Hz"""
    x = source(seed=seed)
    return x, same_filter(x, scipy.signal.firwin(101, fc, fs=FS))


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b))


# ---- recovery, ties, empty inputs ----------------------------------------------------------------------------------------------------------
def test_fit_recovers_a_model_filter_on_the_grid_with_cost_zero():
    from audio_inpainting_diffusion_amd import blind
    cfg = blind.make_settings(n_fft=256, hop=64, K=127)
    F = cfg.F
    c, A = float(cfg.cutoffs[37]), float(cfg.slopes[9])       # 20.5 bins, -6 * 2^(9/4) dB per octave
    H = blind.gain_host(np.arange(F), c, A, cfg.floor_dB)
    sxx = np.where(np.arange(F) % 2 == 0, 1.0, 4.0)           # (powers of two: Sxy / Sxx is H itself)
    fit, index = blind.fit_host(np.stack([sxx, H * sxx])[None], cfg.cutoffs, cfg.slopes, cfg.floor_dB, cfg.eps, cfg.k_lo)
    assert tuple(index[0]) == (37, 9) and fit[0, 0] == c and fit[0, 1] == A and fit[0, 2] == 0.0 and fit[0, 3] == F - cfg.k_lo
    cost = blind.costs_host(np.stack([sxx, H * sxx]), cfg.cutoffs, cfg.slopes, cfg.floor_dB, cfg.eps, cfg.k_lo)
    assert cost.shape == (cfg.cutoffs.size, cfg.slopes.size) and np.sort(cost.reshape(-1))[1] > 0       # no second pair explains it


def test_gain_is_one_up_to_the_knee_falls_by_the_slope_and_stops_at_the_floor():
    from audio_inpainting_diffusion_amd import blind
    H = blind.gain_host(np.array([0, 1, 10, 20, 40, 80, 1 << 20]), 10.0, -12.0, -30.0)
    want = [1, 1, 1, 10 ** (-12 / 20), 10 ** (-24 / 20), 10 ** (-30 / 20), 10 ** (-30 / 20)]
    assert np.allclose(H, want, rtol=1e-14, atol=0) and H[0] == H[2] == 1.0


def test_without_a_valid_bin_every_cost_is_zero_and_the_first_pair_wins():
    from audio_inpainting_diffusion_amd import blind
    cfg = small_settings()
    fit, index = blind.fit_host(np.zeros((2, 2, cfg.F)), cfg.cutoffs, cfg.slopes, cfg.floor_dB, cfg.eps, cfg.k_lo)
    assert np.all(index == 0) and np.all(fit[:, 2:] == 0) and np.all(fit[:, 0] == cfg.cutoffs[0]) and np.all(fit[:, 1] == cfg.slopes[0])
    # bins below k_lo and bins below eps * max do not count
    stats = np.zeros((1, 2, cfg.F))
    stats[0, :, 0] = 1.0
    stats[0, :, 5] = 1e-12
    fit, index = blind.fit_host(stats, cfg.cutoffs, cfg.slopes, cfg.floor_dB, cfg.eps, cfg.k_lo)
    assert tuple(index[0]) == (0, 0) and fit[0, 3] == 0


def test_a_duplicated_candidate_ties_and_the_lower_index_wins():
    from audio_inpainting_diffusion_amd import blind
    cfg = small_settings(cutoffs=[30, 20, 20, 25], slopes=[-6, -48, -48])
    H = blind.gain_host(np.arange(cfg.F), 20.0, -48.0, cfg.floor_dB)
    stats = np.stack([np.ones(cfg.F), H])
    cost = blind.costs_host(stats, cfg.cutoffs, cfg.slopes, cfg.floor_dB, cfg.eps, cfg.k_lo)
    assert cost[1, 1] == cost[1, 2] == cost[2, 1] == cost[2, 2] == 0.0
    fit, index = blind.fit_host(stats[None], cfg.cutoffs, cfg.slopes, cfg.floor_dB, cfg.eps, cfg.k_lo)
    assert tuple(index[0]) == (1, 1)


# ---- noise-free signals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fc", [3000, 5000])
def test_a_windowed_sinc_is_found_within_three_bins_and_its_taps_reproduce_the_observation(fc):
    """Measured with this restatement: knees at bins 33 and 56 against 34.8 and 58.0, rel-L2 of taps * x against y 0.027 and 0.022; the runner-up cost is
    26 % and 13 % above the lowest."""
    from audio_inpainting_diffusion_amd import blind
    cfg = small_settings()
    x, y = sinc_case(fc)
    stats = blind.band_stats_host(x[None], blind.stft_mag_host(y, cfg.n_fft, cfg.hop), cfg.n_fft, cfg.hop)
    assert stats.shape == (1, 2, cfg.F)
    fit, _ = blind.fit_host(stats, cfg.cutoffs, cfg.slopes, cfg.floor_dB, cfg.eps, cfg.k_lo)
    c, A = fit[0, :2]
    taps = blind.design_taps_host(c, A, cfg.n_fft, cfg.K, cfg.floor_dB)
    e = rel(same_filter(x, taps), y)
    costs = np.sort(blind.costs_host(stats[0], cfg.cutoffs, cfg.slopes, cfg.floor_dB, cfg.eps, cfg.k_lo).reshape(-1))[:3]
    print(f"fc = {fc} Hz: knee at bin {c:g} (true {fc * cfg.n_fft / FS:.1f}), slope {A:.1f} dB/oct, rel-L2 = {e:.3f}, three lowest costs {costs}")
    assert abs(c - fc * cfg.n_fft / FS) <= 3
    assert taps.shape == (cfg.K,) and np.array_equal(taps, taps[::-1]) and e <= 0.06


def test_a_longer_transform_finds_the_same_filter():
    """n_fft 512, hop 128, K 255 at 3 kHz.  Measured with this restatement: knee at bin 66 of 69.7, rel-L2 0.026."""
    from audio_inpainting_diffusion_amd import blind
    cfg = small_settings(n_fft=512, hop=128, K=255, cutoffs=np.arange(2, 257))
    x, y = sinc_case(3000)
    stats = blind.band_stats_host(x[None], blind.stft_mag_host(y, cfg.n_fft, cfg.hop), cfg.n_fft, cfg.hop)
    fit, _ = blind.fit_host(stats, cfg.cutoffs, cfg.slopes, cfg.floor_dB, cfg.eps, cfg.k_lo)
    e = rel(same_filter(x, blind.design_taps_host(fit[0, 0], fit[0, 1], cfg.n_fft, cfg.K, cfg.floor_dB)), y)
    print(f"n_fft 512: knee at bin {fit[0, 0]:g} (true {3000 * 512 / FS:.1f}), rel-L2 = {e:.3f}")
    assert abs(fit[0, 0] - 3000 * 512 / FS) <= 6 and e <= 0.06


def test_a_chebyshev_low_pass_is_found_at_its_edge():
    """A sixth-order Chebyshev (1 dB ripple) at 3 kHz is no zero-phase filter; the magnitudes do not see its phase.  Measured: bin 34 of 34.8."""
    from audio_inpainting_diffusion_amd import blind
    cfg = small_settings()
    x = source()
    y = scipy.signal.lfilter(*scipy.signal.cheby1(6, 1, 3000, fs=FS), x)
    stats = blind.band_stats_host(x[None], blind.stft_mag_host(y, cfg.n_fft, cfg.hop), cfg.n_fft, cfg.hop)
    fit, _ = blind.fit_host(stats, cfg.cutoffs, cfg.slopes, cfg.floor_dB, cfg.eps, cfg.k_lo)
    print(f"cheby1: knee at bin {fit[0, 0]:g}, slope {fit[0, 1]:.1f} dB/oct")
    assert abs(fit[0, 0] - 3000 * cfg.n_fft / FS) <= 3


def test_the_taps_have_the_gain_of_the_model_on_the_grid():
    """Without a tap window and with K = n_fft - 1 frequency sampling interpolates H on the grid: the DFT of the taps is H there, but for the one
    missing tap."""
    from audio_inpainting_diffusion_amd import blind
    N, c, A = 64, 9.5, -24.0
    taps = blind.design_taps_host(c, A, N, N - 1, -60.0, window=np.ones(N - 1))
    H = blind.gain_host(np.arange(N // 2 + 1), c, A, -60.0)
    full = np.fft.irfft(H, N)                                              # the N-point zero-phase response, centred at 0
    assert np.allclose(taps, np.roll(full, (N - 2) // 2)[:N - 1], rtol=0, atol=1e-15)
    one = blind.design_taps_host(c, A, N, 1, -60.0)
    assert one.shape == (1,) and np.isclose(one[0], full[0], rtol=1e-14)


def test_band_stats_host_uses_the_framing_of_the_stft_magnitude_operator():
    """n_fft zeros appended, center=False, T = 1 + L // hop, periodic Hann: torch.stft's numbers"""
    from audio_inpainting_diffusion_amd import blind
    x = torch.randn(2, 100, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    want = torch.stft(torch.cat([x, torch.zeros(2, 64, dtype=torch.float64)], 1), 64, 16, window=torch.hann_window(64, dtype=torch.float64),
                      center=False, return_complex=True).abs().numpy()
    got = blind.stft_mag_host(x.numpy(), 64, 16)
    assert got.shape == (2, 33, 1 + 100 // 16) and np.allclose(got, want, rtol=0, atol=1e-12)
    stats = blind.band_stats_host(x.numpy(), 2 * want, 64, 16)
    assert np.allclose(stats[:, 1], 2 * stats[:, 0], rtol=1e-12) and np.allclose(stats[:, 0], (want ** 2).sum(2), rtol=1e-12)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [dict(K=126), dict(K=256), dict(K=257), dict(cutoffs=[]), dict(slopes=[]), dict(slopes=[-6, 3]), dict(slopes=[0]),
                                 dict(cutoffs=[0.0, 4]), dict(n_fft=300), dict(n_fft=4096), dict(hop=0), dict(hop=257), dict(floor_dB=0), dict(k_lo=-1)])
def test_settings_are_refused_on_the_host(bad):
    from audio_inpainting_diffusion_amd import _lib
    with pytest.raises(_lib.AidError):
        small_settings(**bad)


def test_defaults_and_settings_read_from_the_config():
    from audio_inpainting_diffusion_amd import blind
    from audio_inpainting_diffusion_amd.config import small_args
    args = small_args(xi=0.25)
    assert "blind_bwe" not in args.tester                                  # (make_args builds no such key: the defaults apply)
    cfg = blind.settings_of(args)
    assert (cfg.n_fft, cfg.hop, cfg.K, cfg.floor_dB, cfg.k_lo, cfg.eps) == (1024, 256, 501, -80.0, 2, 1e-10)
    assert cfg.cutoffs.size == 2 * (512 - 2) + 1 and cfg.cutoffs[0] == 2 and cfg.cutoffs[1] == 2.5 and cfg.cutoffs[-1] == 512
    assert cfg.slopes.size == 25 and cfg.slopes[0] == -6 and np.isclose(cfg.slopes[-1], -384)
    args.tester.blind_bwe = dict(n_fft=256, hop=64, K=127, cutoffs=[4, 8])
    cfg = blind.settings_of(args)
    assert (cfg.n_fft, cfg.hop, cfg.K, cfg.floor_dB) == (256, 64, 127, -80.0) and list(cfg.cutoffs) == [4, 8] and cfg.slopes.size == 25


class _Fused:                                                              # (stands for the MI355X network: never evaluated here)
    denoise = denoise_guided = None


def _sampler(xi=0.25, dc=None, rid=False):
    from audio_inpainting_diffusion_amd.config import small_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.sampler import Sampler
    args = small_args(xi=xi)
    args.tester.data_consistency.use = dc is not None
    if dc is not None:
        args.tester.data_consistency.type = dc
    args.tester.blind_bwe = dict(SMALL)
    return Sampler(model=_Fused(), diff_params=EDM(args), args=args, rid=rid), int(args.exp.audio_len)


@pytest.mark.parametrize("kw,y_len,taps,text", [
    (dict(dc="always"), 0, None, "data consistency"), (dict(dc="end"), 0, None, "data consistency"), (dict(rid=True), 0, None, "rid"),
    (dict(xi=0.0), 0, None, "xi"), (dict(), 1, None, "audio_len"), (dict(), -1, None, "audio_len"),
    (dict(), 0, torch.zeros(2, 125), "frozen taps"), (dict(), 0, torch.zeros(3, 127), "frozen taps"), (dict(), 0, None, "GPU only")])
def test_predict_blind_bwe_refuses_before_anything_is_installed(kw, y_len, taps, text):
    from audio_inpainting_diffusion_amd import _lib
    smp, L = _sampler(**kw)
    with pytest.raises(_lib.AidError, match=text):
        smp.predict_blind_bwe(torch.zeros(2, L + y_len), frozen_taps=taps)       # (a host tensor: the device is judged last)
    assert smp.y is None and smp.spectral is None and smp.blind_operator is None and smp.blind_fit is None and smp.blind_taps is None


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------
def test_the_three_entry_points_are_bound_under_the_headers_that_declare_them():
    from audio_inpainting_diffusion_amd import _lib
    abi = {a.header: a for a in _lib.ABIS}
    assert abi["aid_phase.h"].launches["aid_stft_band_stats"] is _lib.StftMagParams
    assert abi["aid_phase.h"].launches["aid_lowpass_fit"] is _lib.MatrixNormParams
    assert abi["aid_bwe_long.h"].launches["aid_fir_observed_items"] is _lib.FirObservedParams
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in ("aid_stft_band_stats", "aid_lowpass_fit", "aid_fir_observed_items"))
