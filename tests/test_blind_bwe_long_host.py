"""CPU tests (no GPU) of blind bandwidth extension of whole recordings (blind_long.py, Sampler.predict_blind_bwe_long): the choice of the probe
windows, the chunks of whole recordings, the probe seeds, the pooled statistics and their fit in the float64 restatement, one robustness case
-- a probe whose estimate is unrelated noise does not decide the pooled filter -- the refusals, all raised before anything touches a GPU, and
the two entry points in the ABI table."""
import numpy as np
import pytest
import scipy.signal
import torch

from test_blind_bwe_host import FS, SMALL, _sampler, same_filter, small_settings


# ---- the probe windows ---------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_window_and_the_probes_come_back_ordered_by_start():
    from audio_inpainting_diffusion_amd import blind_long
    E = np.array([[1.0, 3.0, 3.0, 2.0, 3.0], [5.0, 1.0, 0.0, 4.0, 4.5]])
    assert blind_long.choose_probes(E, 2, 8) == [[1, 2], [0, 4]]
    assert blind_long.choose_probes(E, 3, 8) == [[1, 2, 4], [0, 3, 4]]
    assert blind_long.choose_probes(E, 1, 1) == [[1], [0]]
    assert blind_long.choose_probes(np.ones((1, 4)), 2, 2) == [[0, 1]]


def test_more_probes_than_candidates_takes_every_candidate():
    from audio_inpainting_diffusion_amd import blind_long
    assert blind_long.choose_probes(np.array([[2.0, 1.0, 3.0]]), 8, 8) == [[0, 1, 2]]
    assert blind_long.choose_probes(np.array([[0.5]]), 4, 8) == [[0]]


@pytest.mark.parametrize("N,want", [(700, [0]), (1000, [0]), (1001, [0]), (1000 + 750 - 1, [0]), (1000 + 750, [0, 750]), (1000 + 2 * 750 + 3, [0, 750, 1500])])
def test_the_candidates_are_the_windows_wholly_inside_the_recording(N, want):
    """L = 1000, end = 250, K = 33: N < L gives window 0 alone; N = L, N = L + 1 and N one short of a second full window give window 0 (the grid
    has a second window there, which reaches beyond the recording); from N = step + L on the second window counts."""
    from audio_inpainting_diffusion_amd import blind_long, bwe_long
    L, end, K = 1000, 250, 33
    got = blind_long.candidate_starts(N, L, end, K)
    assert got == want
    grid = [s for s, *_ in bwe_long.bwe_windows(N, L, end, K)]
    assert got == grid[:len(got)] and all(s + L <= N for s in got if N >= L)
    y = np.random.default_rng(N).standard_normal((2, N))
    E = blind_long.window_energy_host(y, got, L)
    assert E.shape == (2, len(got)) and np.allclose(E[:, 0], (y[:, :L] ** 2).sum(1), rtol=1e-14)
    assert blind_long.choose_probes(E, 4, 8) == [list(range(len(got)))] * 2


def test_an_all_zero_recording_is_refused_by_name_and_so_are_bad_probe_counts():
    from audio_inpainting_diffusion_amd import _lib, blind_long
    E = np.array([[1.0, 2.0], [3.0, 1.0], [0.0, 0.0], [1.0, 1.0]])
    with pytest.raises(_lib.AidError, match="recording 2 "):
        blind_long.choose_probes(E, 2, 8)
    with pytest.raises(_lib.AidError, match="recording 0 "):
        blind_long.choose_probes(np.array([[np.nan, 1.0]]), 2, 8)
    for probes, max_batch in ((0, 8), (-1, 8), (9, 8), (2, 1), (True, 8), (2.0, 8)):
        with pytest.raises(_lib.AidError, match="probes"):
            blind_long.choose_probes(E[:2], probes, max_batch)


@pytest.mark.parametrize("counts,max_batch", [([4, 4, 4], 8), ([3, 3, 3, 3], 8), ([1, 2, 3, 4, 1, 1, 8, 1], 8), ([2, 2], 2), ([1] * 9, 4), ([4], 4), ([], 8)])
def test_chunks_hold_whole_recordings_and_never_exceed_max_batch(counts, max_batch):
    from audio_inpainting_diffusion_amd import blind_long
    chunks = blind_long.probe_chunks(counts, max_batch)
    assert [r for r0, r1 in chunks for r in range(r0, r1)] == list(range(len(counts)))            # every recording once, in order, never split
    assert all(r1 > r0 and sum(counts[r0:r1]) <= max_batch for r0, r1 in chunks)
    for (r0, r1), nxt in zip(chunks, chunks[1:]):                                                  # greedy: the next recording did not fit
        assert sum(counts[r0:r1]) + counts[nxt[0]] > max_batch
    # a share of the recordings (a rank's) is chunked the same way
    if len(counts) >= 3:
        part = blind_long.probe_chunks(counts, max_batch, 1, len(counts) - 1)
        assert [r for r0, r1 in part for r in range(r0, r1)] == list(range(1, len(counts) - 1))
    with pytest.raises(Exception):
        blind_long.probe_chunks([max_batch + 1], max_batch)


def test_the_probe_seeds_never_meet_the_window_seeds():
    from audio_inpainting_diffusion_amd import _lib, blind_long, restore
    S = restore.SEED_STRIDE
    seeds, W, P = [0, 1, 7, 8], 500, 8
    window = {s * S + w for s in seeds for w in range(W)}
    probe = [blind_long.probe_seed(s, p) for s in seeds for p in range(P)]
    assert len(set(probe)) == len(probe) and not window & set(probe)
    assert blind_long.probe_seed(3, 0) == 3 * S + S - 1 and blind_long.probe_seed(3, 2) == 3 * S + S - 3
    blind_long.check_probe_seeds(S - 4, 4)                                                         # (window S - 5 and probe 3 are neighbours)
    assert blind_long.probe_seed(1, 3) == 1 * S + (S - 5) + 1
    with pytest.raises(_lib.AidError, match="seeds"):
        blind_long.check_probe_seeds(S - 3, 4)


# ---- the pooled statistics -------------------------------------------------------------------------------------------------------------------
def _stats(x, y, cfg):
    from audio_inpainting_diffusion_amd import blind
    return blind.band_stats_host(x[None], blind.stft_mag_host(y, cfg.n_fft, cfg.hop), cfg.n_fft, cfg.hop)[0]


def test_pooling_one_item_is_the_identity_and_copies_of_the_same_statistics_leave_the_choice_unchanged():
    from audio_inpainting_diffusion_amd import blind, blind_long
    cfg = small_settings()
    rng = np.random.default_rng(3)
    x = rng.standard_normal(4096) * 0.05
    one = _stats(x, same_filter(x, scipy.signal.firwin(101, 3000, fs=FS)), cfg).astype(np.float32).astype(np.float64)
    other = _stats(x, same_filter(x, scipy.signal.firwin(101, 5000, fs=FS)), cfg)
    assert np.array_equal(blind_long.pooled_stats_host(one[None], [0]), one[None])
    assert np.array_equal(blind_long.pooled_stats_host(np.stack([one, other]), [0, 1]), np.stack([one, other]))       # every item its own group
    fit1, idx1 = blind.fit_host(one[None], cfg.cutoffs, cfg.slopes, cfg.floor_dB, cfg.eps, cfg.k_lo)
    for n in (2, 4):
        pooled = blind_long.pooled_stats_host(np.stack([one] * n), [0] * n)
        assert np.array_equal(pooled, np.stack([one * n] * n))                                     # (n = 2, 4: exact in floating point)
        fit, idx = blind.fit_host(pooled, cfg.cutoffs, cfg.slopes, cfg.floor_dB, cfg.eps, cfg.k_lo)
        assert np.array_equal(idx, np.repeat(idx1, n, axis=0)) and np.array_equal(fit[:, :2], np.repeat(fit1[:, :2], n, axis=0))


def test_the_pooled_fit_is_the_fit_of_the_float64_sum_in_item_order():
    from audio_inpainting_diffusion_amd import _lib, blind, blind_long
    cfg = small_settings()
    rng = np.random.default_rng(4)
    stats = rng.random((6, 2, cfg.F)).astype(np.float32)
    groups = [0, 1, 0, 3, 3, 3]
    pooled = blind_long.pooled_stats_host(stats, groups)
    s64 = stats.astype(np.float64)
    want = {0: s64[0] + s64[2], 1: s64[1], 3: (s64[3] + s64[4]) + s64[5]}
    for b, g in enumerate(groups):
        assert np.array_equal(pooled[b], want[g]), b
    fit, idx = blind.fit_host(pooled, cfg.cutoffs, cfg.slopes, cfg.floor_dB, cfg.eps, cfg.k_lo)
    for g, rows in ((0, [0, 2]), (3, [3, 4, 5])):
        ref = blind.fit_host(want[g][None], cfg.cutoffs, cfg.slopes, cfg.floor_dB, cfg.eps, cfg.k_lo)
        for b in rows:
            assert np.array_equal(fit[b], ref[0][0]) and np.array_equal(idx[b], ref[1][0])
    with pytest.raises(_lib.AidError):
        blind_long.pooled_stats_host(stats, groups[:-1])


def test_a_probe_whose_estimate_is_unrelated_noise_does_not_decide_the_pooled_filter():
    """White noise (sigma 0.05) through a 101-tap Hamming windowed sinc at 3 kHz (true knee: bin 34.8 of n_fft 256), four probe windows of 4096
    samples.  In three the estimate is the clean window; in window 2 it is unrelated white noise of the same level: the magnitudes of
    independent signals still correlate through |Y|, so g[k] of that window keeps a knee, but scaled by E|X| E|Y| / E|X|^2 = pi / 4 and noisy.
    Measured with this restatement: the windows alone find bins 33, 33, 29, 33; pooled over the four windows bin 33 (the fit of each clean
    window).  Asserted, and no more: the pooled cut-off lies nearer the true bin than window 2's own fit (1.8 against 5.8 bins)."""
    from audio_inpainting_diffusion_amd import blind, blind_long
    cfg = small_settings()
    Lw, true_bin = 4096, 3000 * cfg.n_fft / FS
    rng = np.random.default_rng(11)
    x = rng.standard_normal(4 * Lw) * 0.05
    y = same_filter(x, scipy.signal.firwin(101, 3000, fs=FS))
    est = x.copy()
    est[2 * Lw:3 * Lw] = rng.standard_normal(Lw) * 0.05
    stats = np.stack([_stats(est[w * Lw:(w + 1) * Lw], y[w * Lw:(w + 1) * Lw], cfg) for w in range(4)])
    own, _ = blind.fit_host(stats, cfg.cutoffs, cfg.slopes, cfg.floor_dB, cfg.eps, cfg.k_lo)
    pooled, _ = blind.fit_host(blind_long.pooled_stats_host(stats, [0, 0, 0, 0]), cfg.cutoffs, cfg.slopes, cfg.floor_dB, cfg.eps, cfg.k_lo)
    print(f"true bin {true_bin:.1f}: the windows alone {list(own[:, 0])}, pooled {pooled[0, 0]:g}")
    assert np.all(pooled[:, 0] == pooled[0, 0])
    assert abs(pooled[0, 0] - true_bin) < abs(own[2, 0] - true_bin)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,call,text", [
    (dict(rid=True), {}, "rid"), (dict(xi=0.0), {}, "xi"), (dict(xi=-1.0), {}, "xi"),
    (dict(dc="always"), {}, "runs without data consistency"), (dict(dc="end"), {}, "estimated filter"),
    (dict(), dict(frozen_taps=torch.zeros(125)), "frozen taps"), (dict(), dict(frozen_taps=torch.zeros(3, 127)), "frozen taps"),
    (dict(), dict(probes=0), "probes"), (dict(), dict(probes=9), "probes"), (dict(), dict(probes=3, max_batch=2), "probes"),
    (dict(), dict(seeds=[1]), "seeds"), (dict(), dict(max_batch=0), "max_batch"), (dict(), {}, "GPU only")])
def test_predict_blind_bwe_long_refuses_before_anything_is_launched(kw, call, text):
    from audio_inpainting_diffusion_amd import _lib
    smp, L = _sampler(**kw)
    with pytest.raises(_lib.AidError, match=text):
        smp.predict_blind_bwe_long(torch.zeros(2, 2 * L + L // 3), **call)                  # (a host tensor: the device is judged last)
    assert smp.y is None and smp.spectral is None and smp.blind_fit is None and smp.blind_taps is None and smp.blind_probes is None


def test_an_overlap_shorter_than_twice_the_reach_is_refused_with_more_than_one_window_only():
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.sampler import autoregressive_overlap
    smp, L = _sampler()
    end = int(autoregressive_overlap(smp.args) * L)
    smp.args.tester.blind_bwe = dict(n_fft=2048, hop=512, K=1025)
    assert end < 2 * (1025 - 1)
    with pytest.raises(_lib.AidError, match=r"2 \(K - 1\)"):
        smp.predict_blind_bwe_long(torch.zeros(1, L + 1))
    with pytest.raises(_lib.AidError, match="GPU only"):                                     # one window: no overlap is needed
        smp.predict_blind_bwe_long(torch.zeros(1, L))
    smp.args.tester.blind_bwe = dict(SMALL)
    with pytest.raises(_lib.AidError, match="float32"):
        smp.predict_blind_bwe_long(torch.zeros(2 * L))


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_the_two_entry_points_are_bound_under_the_headers_that_declare_them():
    from audio_inpainting_diffusion_amd import _lib
    abi = {a.header: a for a in _lib.ABIS}
    assert abi["aid_bwe_long.h"].launches["aid_window_energy"] is _lib.BweGatherParams
    assert abi["aid_phase.h"].launches["aid_lowpass_fit_groups"] is _lib.MatrixNormParams
    assert "AID_LOWPASS_FIT_MAX_ITEMS" in abi["aid_phase.h"].macros and _lib.AID_LOWPASS_FIT_MAX_ITEMS == 256
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in ("aid_window_energy", "aid_lowpass_fit_groups"))
