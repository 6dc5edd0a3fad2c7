"""GPU tests of blind bandwidth extension (csrc/aid_blind_bwe.hip, blind.py, Sampler.predict_blind_bwe): the band statistics, the fit and the tap
design against their float64 restatements, the filter with one tap row per item bit for bit against aid_fir_observed, and the sampler on the
reduced HIP network -- frozen taps against predict_bwe, a logged run against its playback, two streams against one.  Small shapes only."""
import functools

import numpy as np
import pytest
import scipy.signal
import torch

from conftest import rel_l2
from test_blind_bwe_host import FS, SMALL, same_filter, sinc_case, small_settings, source

pytestmark = pytest.mark.gpu
DEV = "cuda"
# The cost of the pair the kernel chose, re-evaluated in float64 on the kernel's own fp32 statistics, may exceed the float64 minimum by this
# relative margin.  Measured over the cases below on one MI355X: 0.0 in every case (the kernel chose the float64 pair), so 4 x the largest
# value seen is 0; what remains is that the kernel adds the same fp64 terms in another order (pass band and floor as prefix sums), which moves
# a cost by at most F * 2^-53 = 1.1e-13 at F = 1025 and can swap two candidates closer than that
FIT_MARGIN = 1e-12
# rel-L2 of the taps against design_taps_host: 4 x the largest value measured over the cases below (4.62e-08 at K = 1; 2.7e-08 ... 3.7e-08 elsewhere),
# the rounding of the result to fp32
TAPS_BAR = 4 * 4.62e-8
# rel-L2 of Sxx and Sxy against band_stats_host: an fp32 radix-2 FFT of N points leaves about eps log2(N) = 6e-8 * 11 on |X|, twice that on a product
# of two magnitudes; the sums over t are fp64.  1e-5 is the bar the FFT kernels of this project are held to (tests/test_gpu_phase.py)
STATS_BAR = 1e-5


def _noise(B, L, seed, scale=0.05):
    return torch.randn(B, L, generator=torch.Generator().manual_seed(seed)) * scale


# ---- band statistics ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,n_fft,hop", [(1, 100, 64, 16), (3, 4133, 256, 64), (2, 2085, 1024, 256)])
def test_band_stats_against_the_float64_restatement_item_by_item_and_twice(B, L, n_fft, hop):
    from audio_inpainting_diffusion_amd import _lib, blind
    cfg = blind.make_settings(n_fft=n_fft, hop=hop, K=15)
    x, y = _noise(B, L, 1 + L), _noise(B, L, 2 + L)
    xd = x.to(DEV)
    y_mag = blind.stft_mag(y.to(DEV), cfg)
    assert y_mag.shape == (B, cfg.F, 1 + L // hop)
    stats = blind.band_stats(xd, y_mag, cfg)
    want = blind.band_stats_host(x.numpy(), y_mag.cpu().numpy(), n_fft, hop)
    errs = [rel_l2(stats[:, s].cpu(), want[:, s]) for s in (0, 1)]
    print(f"band stats B={B} L={L} n_fft={n_fft} hop={hop}: rel-L2 Sxx {errs[0]:.2e}, Sxy {errs[1]:.2e}")
    assert stats.shape == (B, 2, cfg.F) and max(errs) <= STATS_BAR
    assert torch.equal(blind.band_stats(xd, y_mag, cfg), stats)                       # deterministic
    for b in range(B):                                                                 # an item does not depend on the others
        assert torch.equal(blind.band_stats(xd[b:b + 1], y_mag[b:b + 1].contiguous(), cfg), stats[b:b + 1]), b
    # a strided x_hat (rows of a wider buffer) gives the same bits
    wide = torch.full((B, L + 5), 3.0, device=DEV)
    wide[:, 2:2 + L] = xd
    assert torch.equal(blind.band_stats(wide[:, 2:2 + L], y_mag, cfg), stats)
    # refusals of the launcher: checked on the host, nothing is launched
    out = torch.zeros_like(stats)
    scratch = torch.zeros(B, 1 + L // hop, 2, cfg.F, device=DEV)
    window, twiddle, _, _ = blind.tables(cfg, DEV)
    for bad in (dict(adjoint=1), dict(n_frames=L // hop), dict(hop=0), dict(n_fft=n_fft + 1), dict(x_ld=L - 1), dict(g=None), dict(frames=None)):
        kw = dict(g=y_mag.data_ptr(), frames=scratch.data_ptr(), n_fft=n_fft, hop=hop, n_frames=1 + L // hop, adjoint=0, x_ld=L)
        kw.update(bad)
        with pytest.raises(_lib.AidError):
            _lib.call("aid_stft_band_stats", _lib.StftMagParams(xd.data_ptr(), kw["g"], out.data_ptr(), kw["frames"], window.data_ptr(), twiddle.data_ptr(),
                                                                B, kw["n_fft"], kw["hop"], kw["n_frames"], kw["adjoint"], L, kw["x_ld"], L))
    assert bool((out == 0).all())


# ---- the fit -----------------------------------------------------------------------------------------------------------------------------
def _check_fit(stats, cfg, what):
    """fit and taps of the kernel on ``stats`` [B, 2, F] (GPU) against fit_host / design_taps_host on the same numbers -> the largest relative
    excess of the chosen pair's float64 cost over the float64 minimum, and the largest rel-L2 of the taps"""
    from audio_inpainting_diffusion_amd import blind
    fit, taps = blind.lowpass_fit(stats, cfg)
    fit2, taps2 = blind.lowpass_fit(stats, cfg)
    assert torch.equal(fit, fit2) and torch.equal(taps, taps2)
    fit, taps, host = fit.cpu().double().numpy(), taps.cpu().numpy(), stats.cpu().double().numpy()
    want, index = blind.fit_host(host, cfg.cutoffs, cfg.slopes, cfg.floor_dB, cfg.eps, cfg.k_lo)
    wtap = blind.tables(cfg, DEV)[3].cpu().double().numpy()
    excess, terr = 0.0, 0.0
    for b in range(host.shape[0]):
        cost = blind.costs_host(host[b], cfg.cutoffs, cfg.slopes, cfg.floor_dB, cfg.eps, cfg.k_lo)
        j, i = np.nonzero(cfg.cutoffs == np.float32(fit[b, 0]))[0][0], np.nonzero(cfg.slopes == np.float32(fit[b, 1]))[0][0]    # (the first: the tie rule)
        low = np.sort(cost.reshape(-1))[:2]
        ex = (cost[j, i] - low[0]) / low[0] if low[0] > 0 else float(cost[j, i] > 0)
        excess = max(excess, ex)
        assert fit[b, 3] == want[b, 3], (what, b, fit[b], want[b])                                        # the valid bins are counted exactly
        assert abs(fit[b, 2] - cost[j, i]) <= 1e-6 * cost[j, i] + 1e-30, (what, b, fit[b, 2], cost[j, i])   # the cost it reports is that pair's
        if cost.size == 1 or low[0] == 0 or low[1] >= 1.09 * low[0]:                                      # a runner-up 9 % away: the very pair
            assert (j, i) == tuple(index[b]), (what, b, (j, i), tuple(index[b]))
        ref = blind.design_taps_host(fit[b, 0], fit[b, 1], cfg.n_fft, cfg.K, cfg.floor_dB, window=wtap)
        terr = max(terr, rel_l2(taps[b], ref))
    print(f"fit {what}: chosen (bins, dB/oct) {[tuple(np.round(f[:2], 2)) for f in fit]}, excess over the float64 minimum {excess:.2e}, taps rel-L2 {terr:.2e}")
    assert excess <= FIT_MARGIN and terr <= TAPS_BAR, (what, excess, terr)
    return fit, taps


def _signal_stats(cfg, pairs):
    from audio_inpainting_diffusion_amd import blind
    x = torch.from_numpy(np.stack([p[0] for p in pairs])).float().to(DEV)
    y = torch.from_numpy(np.stack([p[1] for p in pairs])).float().to(DEV)
    return blind.band_stats(x, blind.stft_mag(y, cfg), cfg)


def test_fit_finds_three_different_filters_in_one_launch():
    """Items: windowed sincs at 3 kHz and 5 kHz, a sixth-order Chebyshev at 3 kHz -- the cases of tests/test_blind_bwe_host.py, whose two lowest costs
    are 26 % and 13 % apart for the sincs -- on the integer-bin grid of those tests and on the default half-bin grid."""
    x = source()
    cheb = scipy.signal.lfilter(*scipy.signal.cheby1(6, 1, 3000, fs=FS), x)
    pairs = [sinc_case(3000), sinc_case(5000), (x, cheb)]
    for what, cfg in (("integer bins", small_settings()), ("half bins", small_settings(cutoffs=None))):
        fit, taps = _check_fit(_signal_stats(cfg, pairs), cfg, what)
        assert abs(fit[0, 0] - 3000 * cfg.n_fft / FS) <= 3 and abs(fit[1, 0] - 5000 * cfg.n_fft / FS) <= 3 and abs(fit[2, 0] - 3000 * cfg.n_fft / FS) <= 3
        assert not np.array_equal(taps[0], taps[1])
        y0 = same_filter(x, taps[0].astype(np.float64))
        assert rel_l2(y0, pairs[0][1]) <= 0.06


def test_fit_on_unrelated_signals_one_candidate_and_an_all_zero_estimate():
    from audio_inpainting_diffusion_amd import blind
    # white noise against unrelated white noise: a flat g, many candidates close to one another
    cfg = small_settings(cutoffs=None)
    stats = blind.band_stats(_noise(2, 4133, 5).to(DEV), blind.stft_mag(_noise(2, 4133, 6).to(DEV), cfg), cfg)
    _check_fit(stats, cfg, "unrelated noise")
    # an even number of cut-offs (the kernel pairs cut-off q with NC - 1 - q) and of slopes, more cut-offs than one sweep of the workgroup
    even = small_settings(cutoffs=np.arange(8, 1210) / 10, slopes=[-12, -96])
    _check_fit(_signal_stats(even, [sinc_case(3000), sinc_case(5000)]), even, "1202 cut-offs, 2 slopes")
    # NC = NA = 1
    one = small_settings(cutoffs=[21.5], slopes=[-30])
    fit, _ = _check_fit(_signal_stats(one, [sinc_case(3000)]), one, "one candidate")
    assert fit[0, 0] == 21.5 and fit[0, 1] == -30
    # an all-zero x_hat: no valid bin, every cost 0, the first pair, and its taps
    stats = blind.band_stats(torch.zeros(2, 4133, device=DEV), blind.stft_mag(_noise(2, 4133, 7).to(DEV), cfg), cfg)
    assert bool((stats == 0).all())
    fit, taps = _check_fit(stats, cfg, "all-zero estimate")
    assert np.all(fit[:, 0] == cfg.cutoffs[0]) and np.all(fit[:, 1] == cfg.slopes[0]) and np.all(fit[:, 2:] == 0) and np.all(np.isfinite(taps))


@pytest.mark.parametrize("n_fft,K", [(64, 1), (256, 127), (2048, 1025)])
def test_taps_against_the_float64_design(n_fft, K):
    """K = 1025 at n_fft 2048 is more than one 1024-tap LDS chunk of the filter; model statistics put the knee where the test wants it."""
    from audio_inpainting_diffusion_amd import blind
    cfg = blind.make_settings(n_fft=n_fft, hop=n_fft // 4, K=K)
    knees = [(cfg.cutoffs[cfg.cutoffs.size // 3], cfg.slopes[4]), (cfg.cutoffs[cfg.cutoffs.size // 2], cfg.slopes[20])]
    k = np.arange(cfg.F)
    stats = np.stack([np.stack([np.ones(cfg.F), blind.gain_host(k, float(c), float(A), cfg.floor_dB)]) for c, A in knees])
    fit, taps = _check_fit(torch.from_numpy(stats).float().to(DEV), cfg, f"model statistics n_fft={n_fft} K={K}")
    assert [tuple(f[:2]) for f in fit] == [(float(c), float(A)) for c, A in knees] and taps.shape == (2, K)
    assert np.array_equal(taps, taps[:, ::-1]) or rel_l2(taps, taps[:, ::-1].copy()) <= 1e-6            # zero phase


def test_lowpass_fit_refusals_of_the_launcher():
    from audio_inpainting_diffusion_amd import _lib, blind
    cfg = small_settings()
    B, F, K = 2, cfg.F, cfg.K
    stats = torch.ones(B, 2, F, device=DEV)
    _, _, cand, wtap = blind.tables(cfg, DEV)
    fit, taps, diag = torch.zeros(B, 4, device=DEV), torch.zeros(B, K, device=DEV), torch.zeros(B, 2, device=DEV)
    for bad in (dict(F=F + 1), dict(F=2049), dict(F=5), dict(NC=0), dict(NA=0), dict(K=K + 1), dict(K=cfg.n_fft + 1), dict(K=0), dict(eps=-1.0), dict(B=0),
                dict(diag=diag.data_ptr()), dict(r=None)):
        kw = dict(B=B, F=F, NC=cfg.cutoffs.size, NA=cfg.slopes.size, K=K, eps=cfg.eps, diag=None, r=wtap.data_ptr())
        kw.update(bad)
        with pytest.raises(_lib.AidError):
            _lib.call("aid_lowpass_fit", _lib.MatrixNormParams(stats.data_ptr(), cand.data_ptr(), taps.data_ptr(), fit.data_ptr(), kw["r"], kw["diag"],
                                                               kw["B"], kw["F"], kw["NC"], kw["NA"], kw["K"], kw["eps"]))
    assert bool((fit == 0).all()) and bool((taps == 0).all())


# ---- the filter with one tap row per item -------------------------------------------------------------------------------------------------
def _fir(name, x, y, state, h, K, mode):
    from audio_inpainting_diffusion_amd import _lib
    B, L = x.shape
    out = torch.full((B, L), -7.5, device=DEV)
    _lib.call(name, _lib.FirObservedParams(x.data_ptr(), y.data_ptr() if mode == 2 else None, state.data_ptr(), h.data_ptr(), out.data_ptr(),
                                           B, K, mode, L, L, L, 0 if state.shape[0] == 1 else L, L))
    return out


@pytest.mark.parametrize("L", [2049, 4100])
@pytest.mark.parametrize("K", [33, 1025])
@pytest.mark.parametrize("shared", [False, True])
def test_fir_observed_items_is_fir_observed_row_by_row(L, K, shared):
    """Equal tap rows: aid_fir_observed's bits in modes 0, 1 and 2.  Different rows: item b is aid_fir_observed with row b alone.  L crosses the
    2048-output tile, K = 1025 the 1024-tap LDS chunk."""
    from test_gpu_bwe_long import _signals
    B = 3
    x, y, gy, h, state = _signals(B, L, K, 3 + L + K)
    rows = torch.stack([h, h.flip(0) * 0.5, torch.randn(K, generator=torch.Generator().manual_seed(K)) / K ** 0.5])
    xd, yd, gd, hd, rd = x.to(DEV), y.to(DEV), gy.to(DEV), h.to(DEV), rows.to(DEV).contiguous()
    kd = (state[:1] if shared else state).to(DEV).contiguous()
    same = hd.expand(B, K).contiguous()
    for mode, src in ((0, xd), (1, gd), (2, xd)):
        want = _fir("aid_fir_observed", src, yd, kd, hd, K, mode)
        assert torch.equal(_fir("aid_fir_observed_items", src, yd, kd, same, K, mode), want), mode
        got = _fir("aid_fir_observed_items", src, yd, kd, rd, K, mode)
        assert torch.equal(got[0], want[0]) and not torch.equal(got[1], want[1])
        for b in range(B):
            alone = _fir("aid_fir_observed", src[b:b + 1].contiguous(), yd[b:b + 1].contiguous(), kd if shared else kd[b:b + 1].contiguous(), rd[b].contiguous(), K, mode)
            assert torch.equal(got[b:b + 1], alone), (mode, b)
    # <A x, g> = <x, A^T g> with per-item rows, to fp32 rounding
    ax, atg = _fir("aid_fir_observed_items", xd, yd, kd, rd, K, 0).cpu().double(), _fir("aid_fir_observed_items", gd, yd, kd, rd, K, 1).cpu().double()
    lhs, rhs = float((ax * gy.double()).sum()), float((x.double() * atg).sum())
    assert abs(lhs - rhs) <= 1e-6 * float(ax.norm() * gy.double().norm())


def test_with_every_state_filtered_and_equal_rows_the_operator_is_fir_filter_bit_for_bit_in_three_plus_one_launches():
    from audio_inpainting_diffusion_amd import _lib, blind
    from audio_inpainting_diffusion_amd.degrade import FIRFilter
    cfg = small_settings()
    B, L = 3, 4133
    x, gy = _noise(B, L, 11).to(DEV), _noise(B, L, 12).to(DEV)
    h = torch.from_numpy(scipy.signal.firwin(cfg.K, 3000, fs=FS).astype(np.float32))
    op, fir = blind.BlindLowpass(x, cfg, taps=h, frozen=True), FIRFilter(h, L, device=DEV)
    assert op.shared_mask is False and op.items_held == B
    assert torch.equal(op.apply(x), fir.apply(x)) and torch.equal(op.adjoint(gy), fir.adjoint(gy))
    with pytest.raises(AttributeError):
        op.project(x, x)
    # the launches of an evaluation: statistics, fit, filter -- and one for the adjoint; rows() hands out views
    live = blind.BlindLowpass(fir.apply(x), cfg)
    names, call = [], _lib.call
    _lib.call = lambda name, params: names.append(name) or call(name, params)
    try:
        out = live.apply(x)
        live.adjoint(gy)
    finally:
        _lib.call = call
    assert names == ["aid_stft_band_stats", "aid_lowpass_fit", "aid_fir_observed_items", "aid_fir_observed_items"]
    sub = live.rows(1, 3)
    assert live.rows(1, 3) is sub and sub.taps.data_ptr() == live.taps[1:].data_ptr() and sub.y_mag.data_ptr() == live.y_mag[1:].data_ptr()
    taps = live.taps.clone()
    assert torch.equal(sub.apply(x[1:3]), out[1:3]) and torch.equal(live.taps, taps)           # the fit of a sub-batch is the fit of its items
    assert abs(float(live.fit[0, 0]) - 3000 * cfg.n_fft / FS) <= 3


# ---- the sampler on the reduced HIP network -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _net():
    from test_gpu_bwe_long import _small_net
    smp, _, Ls = _small_net(xi=0.25)
    smp.args.tester.blind_bwe = dict(SMALL)
    return smp, Ls


def _observed(B, Ls, seed=80):
    taps = torch.from_numpy(scipy.signal.firwin(SMALL["K"], 3000, fs=FS).astype(np.float32))
    clean = torch.stack([torch.randn(Ls, generator=torch.Generator().manual_seed(seed + i)) for i in range(B)]) * 0.063
    return torch.nn.functional.conv1d(clean[:, None], taps[None, None], padding="same").squeeze(1).to(DEV), taps


def test_frozen_equal_rows_are_predict_bwe_bit_for_bit():
    smp, Ls = _net()
    y, taps = _observed(2, Ls)
    smp.seeds = [5, 6]
    out = smp.predict_blind_bwe(y, frozen_taps=taps)
    assert out.shape == (2, Ls) and torch.equal(smp.blind_taps.cpu(), taps.expand(2, -1)) and smp.blind_operator.frozen
    smp.seeds = [5, 6]
    assert torch.equal(out, smp.predict_bwe(y, taps, "firwin")) and not torch.equal(out, y)


class _Playback:
    """The operator of a logged run: evaluation n filters with the taps the log holds for it (a frozen BlindLowpass whose rows are replaced)."""
    shared_mask = False

    def __init__(self, op, log):
        self.op, self.log, self.n = op, log, 0

    def apply(self, x):
        self.op.taps.copy_(self.log[self.n][0])
        self.n += 1
        return self.op.apply(x)

    def adjoint(self, g):
        return self.op.adjoint(g)


def test_a_logged_run_equals_its_playback_and_leaves_the_last_fit():
    from audio_inpainting_diffusion_amd import blind
    smp, Ls = _net()
    cfg = blind.settings_of(smp.args)
    y, _ = _observed(2, Ls)
    smp.seeds, smp.blind_log = [7, 8], []
    try:
        n0 = smp.n_evals
        out = smp.predict_blind_bwe(y)
    finally:
        log, smp.blind_log = smp.blind_log, None
    evals = (smp.n_evals - n0) // 2
    assert len(log) == evals == 2 * smp.nb_steps - 1 and all(t.shape == (2, cfg.K) and f.shape == (2, 4) for t, f in log)
    assert torch.equal(smp.blind_taps, log[-1][0]) and torch.equal(smp.blind_fit[:, 0], log[-1][1][:, 0] * (FS / cfg.n_fft)) and torch.equal(smp.blind_fit[:, 1], log[-1][1][:, 1])
    assert smp.blind_fit.shape == (2, 2) and bool(torch.isfinite(out).all()) and int(smp.args.exp.sample_rate) == FS
    print("blind run, reduced network: fitted (Hz, dB/oct) per evaluation of item 0:", [(round(float(f[0, 0]) * FS / cfg.n_fft), round(float(f[0, 1]), 1)) for _, f in log])
    play = _Playback(blind.BlindLowpass(y, cfg, taps=log[0][0], frozen=True), log)
    smp.seeds = [7, 8]
    assert torch.equal(smp.predict_resample(y, (2, Ls), play), out) and play.n == evals


def test_a_batch_of_four_on_two_streams_equals_one_stream():
    smp, Ls = _net()
    net = smp.model
    y, _ = _observed(4, Ls, seed=90)
    calls, orig = [], net._split_plan
    net._split_plan = lambda B: calls.append(B) or orig(B)
    try:
        smp.seeds = [1, 2, 3, 4]
        two = smp.predict_blind_bwe(y)
        fit2, taps2 = smp.blind_fit.clone(), smp.blind_taps.clone()
        assert 4 in calls and sorted(smp.blind_operator._sub) == [(0, 2), (2, 4)]
        keep, net.split_streams = net.split_streams, 1
        try:
            smp.seeds = [1, 2, 3, 4]
            one = smp.predict_blind_bwe(y)
        finally:
            net.split_streams = keep
    finally:
        net._split_plan = orig
    assert not smp.blind_operator._sub
    assert torch.equal(two, one) and torch.equal(fit2, smp.blind_fit) and torch.equal(taps2, smp.blind_taps)
