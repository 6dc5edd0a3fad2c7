"""GPU tests of blind bandwidth extension of whole recordings (csrc/aid_blind_long.hip, blind_long.py, Sampler.predict_blind_bwe_long,
harness.blind_bwe_long): the window energies and the pooled fit against their float64 restatements and, one item per group, against
aid_lowpass_fit bit for bit; the two window operators against the operators they extend; the two stages on the reduced HIP network -- frozen
taps against predict_bwe_long bit for bit, recordings together against each alone, chunks of whole recordings, a recording shorter than a
window, the harness wrapper -- and three ranks on one GPU against the single process.  Small shapes only."""
import ast
import ctypes
import functools
import os
import queue
import sys
import traceback

import numpy as np
import pytest
import scipy.signal
import torch
import torch.multiprocessing as mp
import torch.utils._python_dispatch

from conftest import GOLDEN, ROOT, rel_l2
from test_blind_bwe_host import FS, sinc_case, small_settings

pytestmark = pytest.mark.gpu
DEV = "cuda"
# relative difference of a window energy against the float64 restatement: both are fp64 sums of the same exactly squared fp32 samples (a
# square of a 24-bit number is exact in fp64) in another order; n additions move a sum of positive terms by at most n * 2^-53 relative, and
# 2^-40 leaves room for 8192 of them.  The largest window below has 1000 samples.
ENERGY_BAR = 2.0 ** -40
BLIND = dict(n_fft=256, hop=64, K=33)                     # the settings on the reduced network: end = 1024 >= 2 (K - 1) = 64


def _noise(B, L, seed, scale=0.05):
    return torch.randn(B, L, generator=torch.Generator().manual_seed(seed)) * scale


class _Launches:
    """records the names of the launches that go through _lib.call"""

    def __enter__(self):
        from audio_inpainting_diffusion_amd import _lib
        self.names, self._call = [], _lib.call
        _lib.call = lambda name, params: self.names.append(name) or self._call(name, params)
        return self.names

    def __exit__(self, *exc):
        from audio_inpainting_diffusion_amd import _lib
        _lib.call = self._call


# ---- the window energies -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,N,L,end", [(2, 700, 1000, 250), (1, 1000, 1000, 250), (3, 2300, 1000, 250), (2, 37, 1, 0)])
def test_window_energy_against_the_float64_restatement_and_twice(R, N, L, end):
    """N < L (one window, 700 samples exist), N = L, three windows of which the last holds 800 samples, and windows of one sample"""
    from audio_inpainting_diffusion_amd import _lib, blind_long, restore
    step = L - end
    W = max(1, -(-(N - L) // step) + 1)
    y = _noise(R, N, 5 + N)
    wide = torch.full((R, N + 5), 3.0, device=DEV)
    wide[:, 2:2 + N] = y.to(DEV)
    yd = wide[:, 2:2 + N]                                                                # rows of a wider buffer
    E = blind_long.window_energy(yd, L, step, W)
    want = blind_long.window_energy_host(y.numpy(), [w * step for w in range(W)], L)
    err = np.abs(E.cpu().numpy() - want) / want
    print(f"window energy R={R} N={N} L={L} W={W}: largest relative difference {err.max():.2e} (2^{np.log2(max(err.max(), 1e-300)):.1f})")
    assert E.shape == (R, W) and E.dtype == torch.float64 and err.max() <= ENERGY_BAR
    assert torch.equal(blind_long.window_energy(yd, L, step, W), E)                      # a second launch gives the same bits
    assert torch.equal(blind_long.window_energy(y.to(DEV), L, step, W), E)               # and so do contiguous rows
    # a job that starts at or beyond the end of the recording, or names no recording, is skipped: energy 0
    table = restore.job_table([(0, 0, 0, 0, 0, L), (0, N, 0, 0, 0, L), (R, 0, 0, 0, 0, L), (-1, 0, 0, 0, 0, L), (R - 1, N - 1, 0, 0, 0, L)], DEV)
    out = torch.full((5,), -1.0, dtype=torch.float64, device=DEV)
    args = dict(rec=yd.data_ptr(), y=out.data_ptr(), jobs=table.data_ptr(), J=5, R=R, L=L, N=N, rec_ld=yd.stride(0))

    def launch(**kw):
        kw = dict(args, **kw)
        _lib.call("aid_window_energy", _lib.BweGatherParams(kw["rec"], None, kw["y"], None, kw["jobs"], kw["J"], kw["R"], 1, kw["L"], kw["N"], kw["rec_ld"], 0))
    launch()
    assert out[:4].tolist() == [float(E[0, 0]), 0.0, 0.0, 0.0] and float(out[4]) == float(y[R - 1, N - 1].double() ** 2)
    # refusals of the launcher: checked on the host, nothing is launched
    out.fill_(-1.0)
    for bad in (dict(rec=None), dict(y=None), dict(jobs=None), dict(J=0), dict(R=0), dict(L=0), dict(N=0), dict(rec_ld=N - 1), dict(y=out.data_ptr() + 4)):
        with pytest.raises(_lib.AidError):
            launch(**bad)
    assert bool((out == -1).all())


# ---- the pooled fit ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,K", [(64, 1), (256, 127), (2048, 1025)])
def test_with_every_item_in_its_own_group_the_pooled_fit_is_aid_lowpass_fit_bit_for_bit(n_fft, K):
    from audio_inpainting_diffusion_amd import blind, blind_long
    cfg = blind.make_settings(n_fft=n_fft, hop=n_fft // 4, K=K)
    k = np.arange(cfg.F)
    model = np.stack([np.ones(cfg.F), blind.gain_host(k, float(cfg.cutoffs[cfg.cutoffs.size // 3]), float(cfg.slopes[4]), cfg.floor_dB)])
    rng = np.random.default_rng(n_fft)
    sxx = rng.random((2, cfg.F)) + 0.1
    noisy = np.stack([np.stack([s, s * model[1] * (0.8 + 0.4 * rng.random(cfg.F))]) for s in sxx])
    stats = torch.from_numpy(np.concatenate([model[None], noisy])).float().to(DEV)
    fit, taps = blind.lowpass_fit(stats, cfg)
    for groups in ([0, 1, 2], [2, 0, 1]):                                                # (the ids are names: any distinct ones)
        gfit, gtaps = blind_long.lowpass_fit_groups(stats, groups, cfg)
        assert torch.equal(gfit, fit) and torch.equal(gtaps, taps), groups
    one, one_taps = blind_long.lowpass_fit_groups(stats[1:2].contiguous(), [0], cfg)     # B = 1
    assert torch.equal(one, fit[1:2]) and torch.equal(one_taps, taps[1:2])


def _check_group_fit(stats, groups, cfg, what):
    """fit and taps of aid_lowpass_fit_groups on ``stats`` [B, 2, F] (GPU) against fit_host / design_taps_host on pooled_stats_host of the same
    numbers, as tests/test_gpu_blind_bwe.py::_check_fit holds aid_lowpass_fit to them, with its margins"""
    from audio_inpainting_diffusion_amd import blind, blind_long
    from test_gpu_blind_bwe import FIT_MARGIN, TAPS_BAR
    fit, taps = blind_long.lowpass_fit_groups(stats, groups, cfg)
    fit2, taps2 = blind_long.lowpass_fit_groups(stats, groups, cfg)
    assert torch.equal(fit, fit2) and torch.equal(taps, taps2)
    for g in set(groups):                                                                # the rows of a group are bit-equal
        rows = [b for b, gb in enumerate(groups) if gb == g]
        for b in rows[1:]:
            assert torch.equal(fit[b], fit[rows[0]]) and torch.equal(taps[b], taps[rows[0]]), (what, g, b)
    fit, taps = fit.cpu().double().numpy(), taps.cpu().numpy()
    pooled = blind_long.pooled_stats_host(stats.cpu().numpy(), groups)
    want, index = blind.fit_host(pooled, cfg.cutoffs, cfg.slopes, cfg.floor_dB, cfg.eps, cfg.k_lo)
    wtap = blind.tables(cfg, DEV)[3].cpu().double().numpy()
    excess, terr = 0.0, 0.0
    for b in range(pooled.shape[0]):
        cost = blind.costs_host(pooled[b], cfg.cutoffs, cfg.slopes, cfg.floor_dB, cfg.eps, cfg.k_lo)
        j, i = np.nonzero(cfg.cutoffs == np.float32(fit[b, 0]))[0][0], np.nonzero(cfg.slopes == np.float32(fit[b, 1]))[0][0]
        low = cost.min()
        excess = max(excess, (cost[j, i] - low) / low if low > 0 else float(cost[j, i] > 0))
        assert fit[b, 3] == want[b, 3], (what, b, fit[b], want[b])
        assert abs(fit[b, 2] - cost[j, i]) <= 1e-6 * cost[j, i] + 1e-30, (what, b, fit[b, 2], cost[j, i])
        terr = max(terr, rel_l2(taps[b], blind.design_taps_host(fit[b, 0], fit[b, 1], cfg.n_fft, cfg.K, cfg.floor_dB, window=wtap)))
    print(f"pooled fit {what}: chosen (bins, dB/oct) {[tuple(np.round(f[:2], 2)) for f in fit]}, excess over the float64 minimum {excess:.2e}, taps rel-L2 {terr:.2e}")
    assert excess <= FIT_MARGIN and terr <= TAPS_BAR, (what, excess, terr)
    return fit, taps


def test_three_groups_with_interleaved_members_a_zero_group_and_one_item():
    """Items 0 and 2: a 3 kHz windowed sinc on two sources; item 1: 5 kHz; items 3, 4, 5: 5 kHz on three sources.  Ids are arbitrary names in
    [0, B).  Then a group whose pooled statistics are all zero beside one that is not."""
    from audio_inpainting_diffusion_amd import blind
    from test_gpu_blind_bwe import _signal_stats
    cfg = small_settings(cutoffs=None)
    pairs = [sinc_case(3000, 0), sinc_case(5000, 1), sinc_case(3000, 2), sinc_case(5000, 3), sinc_case(5000, 4), sinc_case(5000, 5)]
    stats = _signal_stats(cfg, pairs)
    groups = [4, 1, 4, 0, 0, 0]
    fit, taps = _check_group_fit(stats, groups, cfg, "groups {0, 2}, {1}, {3, 4, 5}")
    assert abs(fit[0, 0] - 3000 * cfg.n_fft / FS) <= 3 and abs(fit[1, 0] - 5000 * cfg.n_fft / FS) <= 3 and abs(fit[3, 0] - 5000 * cfg.n_fft / FS) <= 3
    assert not np.array_equal(taps[0], taps[3])
    own, _ = blind.lowpass_fit(stats, cfg)
    assert torch.equal(torch.from_numpy(fit[1]).float(), own[1].cpu())                   # a group of one is the item's own fit
    zero = stats.clone()
    zero[[0, 2]] = 0
    fit, taps = _check_group_fit(zero, groups, cfg, "an all-zero group")
    assert fit[0, 0] == cfg.cutoffs[0] and fit[0, 1] == cfg.slopes[0] and np.all(fit[[0, 2], 2:] == 0) and np.all(np.isfinite(taps)) and fit[3, 3] > 0
    _check_group_fit(stats[:1].contiguous(), [0], cfg, "B = 1")


def test_lowpass_fit_groups_refusals_of_the_launcher_leave_the_outputs_untouched():
    from audio_inpainting_diffusion_amd import _lib, blind, blind_long
    cfg = small_settings()
    B, F, K = 3, cfg.F, cfg.K
    stats = torch.ones(B, 2, F, device=DEV)
    _, _, cand, wtap = blind.tables(cfg, DEV)
    fit, taps = torch.zeros(B, 4, device=DEV), torch.zeros(B, K, device=DEV)
    for bad in (dict(groups=[0, 3, 1]), dict(groups=[0, -1, 1]), dict(groups=[0, 1, B]), dict(groups=None), dict(F=F + 1), dict(F=2049), dict(F=5), dict(NC=0),
                dict(NA=0), dict(K=K + 1), dict(K=cfg.n_fft + 1), dict(K=0), dict(eps=-1.0), dict(B=0), dict(B=_lib.AID_LOWPASS_FIT_MAX_ITEMS + 1),
                dict(stats=None), dict(cand=None), dict(wtap=None), dict(taps=None), dict(fit=None)):
        kw = dict(groups=[0, 0, 2], B=B, F=F, NC=cfg.cutoffs.size, NA=cfg.slopes.size, K=K, eps=cfg.eps, stats=stats.data_ptr(), cand=cand.data_ptr(),
                  wtap=wtap.data_ptr(), taps=taps.data_ptr(), fit=fit.data_ptr())
        kw.update(bad)
        ids = None if kw["groups"] is None else blind_long.group_array(kw["groups"])       # (host memory, read by the launcher)
        with pytest.raises(_lib.AidError):
            _lib.call("aid_lowpass_fit_groups", _lib.MatrixNormParams(kw["stats"], kw["cand"], kw["taps"], kw["fit"], kw["wtap"], None if ids is None else ctypes.addressof(ids),
                                                                       kw["B"], kw["F"], kw["NC"], kw["NA"], kw["K"], kw["eps"]))
    assert bool((fit == 0).all()) and bool((taps == 0).all())
    with pytest.raises(_lib.AidError):
        blind_long.lowpass_fit_groups(stats, [0, 1], cfg)                                # two ids for three items: refused in Python


# ---- the window operator of stage 2 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [33, 1025])
def test_fir_observed_rows_is_fir_observed_with_a_tap_row_per_item(K):
    """L = 2049 crosses the 2048-output tile, K = 1025 the 1024-tap LDS chunk"""
    from audio_inpainting_diffusion_amd.blind_long import FIRObservedRows
    from audio_inpainting_diffusion_amd.bwe_long import FIRObserved
    from test_gpu_bwe_long import _signals
    B, L = 3, 2049
    x, _, gy, h, state = _signals(B, L, K, 9 + K)
    xd, gd, hd, kd = x.to(DEV), gy.to(DEV), h.to(DEV), state.to(DEV).contiguous()
    same = FIRObservedRows(hd.expand(B, K).contiguous(), kd)
    ref = FIRObserved(hd, kd)
    assert same.shared_mask is False and same.items_held == B
    assert torch.equal(same.apply(xd), ref.apply(xd)) and torch.equal(same.adjoint(gd), ref.adjoint(gd))
    with pytest.raises(AttributeError):
        same.project(xd, xd)
    rows = torch.stack([h, h.flip(0) * 0.5, torch.randn(K, generator=torch.Generator().manual_seed(K)) / K ** 0.5]).to(DEV).contiguous()
    op = FIRObservedRows(rows, kd)
    ax, atg = op.apply(xd), op.adjoint(gd)
    for b in range(B):                                                                   # item b is FIRObserved with row b alone
        alone = FIRObserved(rows[b].contiguous(), kd[b:b + 1])
        assert torch.equal(ax[b:b + 1], alone.apply(xd[b:b + 1])) and torch.equal(atg[b:b + 1], alone.adjoint(gd[b:b + 1])), b
    sub = op.rows(1, 3)                                                                  # views, kept per range
    assert op.rows(1, 3) is sub and sub.taps.data_ptr() == rows[1:].data_ptr() and sub.state.data_ptr() == kd[1:].data_ptr() and sub.items_held == 2
    assert torch.equal(sub.apply(xd[1:3]), ax[1:3]) and torch.equal(sub.adjoint(gd[1:3]), atg[1:3])
    lhs, rhs = float((ax.cpu().double() * gy.double()).sum()), float((x.double() * atg.cpu().double()).sum())
    assert abs(lhs - rhs) <= 1e-6 * float(ax.cpu().double().norm() * gy.double().norm())  # <A x, g> = <x, A^T g>


# ---- the operator of stage 1 ---------------------------------------------------------------------------------------------------------------
class _Muls(torch.utils._python_dispatch.TorchDispatchMode):
    """counts the torch multiplications that run under it"""

    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += "mul" in func.__name__
        return func(*args, **(kwargs or {}))


def test_the_pooled_operator_launches_three_kernels_and_one_for_the_adjoint():
    from audio_inpainting_diffusion_amd import _lib, blind, blind_long, bwe_long, restore
    cfg = small_settings(K=33)
    L, N, R = 4133, 3 * 4133, 2
    h = torch.from_numpy(scipy.signal.firwin(101, 3000, fs=FS).astype(np.float32))
    clean = _noise(R, N, 21)
    rec = torch.nn.functional.conv1d(clean[:, None], h[None, None], padding="same").squeeze(1).to(DEV)
    jobs = [(0, 0), (0, 4000), (1, 2 * 4133), (0, 8000)]                                 # recording 0: items 0, 1, 3; recording 1: item 2
    groups = [0, 0, 2, 0]
    yw, kw = bwe_long.bwe_gather(rec, rec, restore.job_table([(r, s, 0, 0, 0, L) for r, s in jobs], DEV), L, cfg.K)
    P = (cfg.K - 1) // 2
    assert bool((kw[0, :P] == 0).all()) and bool((kw[1, :P] == -1).all()) and bool((kw[2, L - P:] == 0).all()) and not bool((kw == -2).any())
    raw = blind_long.raw_windows(rec, jobs, L)
    assert torch.equal(raw[1], rec[0, 4000:4000 + L]) and torch.equal(torch.where(kw == 0, raw, torch.zeros_like(raw)), yw)
    op = blind_long.PooledBlindLowpass(raw, kw, groups, cfg)
    assert not hasattr(op, "rows") and op.shared_mask is False and op.present is None
    x = torch.stack([clean[r, s:s + L] for r, s in jobs]).to(DEV)
    gy = _noise(4, L, 22).to(DEV)
    muls = _Muls()
    with _Launches() as names, muls:
        out = op.apply(x)
        adj = op.adjoint(gy)
    assert names == ["aid_stft_band_stats", "aid_lowpass_fit_groups", "aid_fir_observed_items", "aid_fir_observed_items"] and muls.n == 0
    with pytest.raises(AttributeError):
        op.project(x, x)
    # the statistics are each item's own, the fit is the pooled one, the filter runs over the states
    assert torch.equal(op.stats, blind.band_stats(x, blind.stft_mag(raw, cfg), cfg))
    fit, taps = blind_long.lowpass_fit_groups(op.stats, groups, cfg)
    assert torch.equal(op.fit, fit) and torch.equal(op.taps, taps) and torch.equal(taps[0], taps[1]) and torch.equal(taps[0], taps[3])
    ref = blind_long.FIRObservedRows(taps, kw)
    assert torch.equal(out, ref.apply(x)) and torch.equal(adj, ref.adjoint(gy))
    assert abs(float(fit[0, 0]) - 3000 * cfg.n_fft / FS) <= 3 and abs(float(fit[2, 0]) - 3000 * cfg.n_fft / FS) <= 3


def test_an_item_with_absent_samples_costs_one_multiplication_and_its_statistics_see_zeros_there():
    from audio_inpainting_diffusion_amd import blind, blind_long, bwe_long, restore
    from test_gpu_blind_bwe import STATS_BAR
    cfg = small_settings(K=33)
    L, N = 4133, 3000
    rec = _noise(1, N, 31).to(DEV)
    yw, kw = bwe_long.bwe_gather(rec, rec, restore.job_table([(0, 0, 0, 0, 0, L)], DEV), L, cfg.K)
    assert bool((kw[0, :N] == 0).all()) and bool((kw[0, N:] == -2).all())
    raw = blind_long.raw_windows(rec, [(0, 0)], L)
    assert torch.equal(raw[:, :N], rec) and bool((raw[:, N:] == 0).all())
    op = blind_long.PooledBlindLowpass(raw, kw, [0], cfg)                                # (absent = None: it looks at the state)
    assert op.present is not None and torch.equal(op.present, (kw > -2).float())
    x = _noise(1, L, 32).to(DEV)
    muls = _Muls()
    with _Launches() as names, muls:
        out = op.apply(x)
        op.adjoint(x)
    assert names == ["aid_stft_band_stats", "aid_lowpass_fit_groups", "aid_fir_observed_items", "aid_fir_observed_items"] and muls.n == 1
    zeroed = x.cpu().numpy().copy()
    zeroed[:, N:] = 0
    want = blind.band_stats_host(zeroed, op.y_mag.cpu().numpy(), cfg.n_fft, cfg.hop)
    errs = [rel_l2(op.stats[:, s].cpu(), want[:, s]) for s in (0, 1)]
    unzeroed = blind.band_stats_host(x.cpu().numpy(), op.y_mag.cpu().numpy(), cfg.n_fft, cfg.hop)
    print(f"statistics of an item with absent samples: rel-L2 Sxx {errs[0]:.2e}, Sxy {errs[1]:.2e} (against the statistics of the unzeroed x_hat: {rel_l2(op.stats[:, 0].cpu(), unzeroed[:, 0]):.2e})")
    assert max(errs) <= STATS_BAR and rel_l2(op.stats[:, 0].cpu(), unzeroed[:, 0]) > 100 * STATS_BAR
    assert bool((out[:, N:] == 0).all())                                                 # absent samples are no observations


# ---- the two stages on the reduced HIP network ---------------------------------------------------------------------------------------------
T_STEPS, SEEDS = 3, [31, 32]


@functools.lru_cache(maxsize=None)
def _net():
    from test_gpu_bwe_long import _small_net
    smp, _, Ls = _small_net(xi=0.25)
    smp.args.tester.blind_bwe = dict(BLIND)
    return smp, Ls


def _recordings(Ls, N=None, R=2):
    """R recordings of N samples (default 2 Ls + Ls // 3: three windows), recording r through a 101-tap windowed sinc at 3 kHz (r = 0) or 7 kHz"""
    N = 2 * Ls + Ls // 3 if N is None else N
    clean = torch.stack([torch.randn(N, generator=torch.Generator().manual_seed(70 + r)) for r in range(R)]) * 0.063
    hs = [torch.from_numpy(scipy.signal.firwin(101, fc, fs=FS).astype(np.float32)) for fc in (3000, 7000)]
    return torch.cat([torch.nn.functional.conv1d(clean[r:r + 1, None], hs[r % 2][None, None], padding="same").squeeze(1) for r in range(R)]).to(DEV)


def _taps(fc):
    return torch.from_numpy(scipy.signal.firwin(BLIND["K"], fc, fs=FS).astype(np.float32))


def test_frozen_taps_are_predict_bwe_long_bit_for_bit_and_stage_one_launches_nothing():
    smp, Ls = _net()
    y = _recordings(Ls)
    h = _taps(3000)
    n0 = smp.n_evals
    with _Launches() as names:
        out = smp.predict_blind_bwe_long(y, seeds=SEEDS, frozen_taps=h)
    assert smp.n_evals - n0 == 6 * (2 * T_STEPS - 1) and not {"aid_window_energy", "aid_lowpass_fit_groups", "aid_stft_band_stats", "aid_stft_mag"} & set(names)
    assert torch.equal(out, smp.predict_bwe_long(y, h, "firwin", seeds=SEEDS)) and not torch.equal(out, y)
    assert torch.equal(smp.blind_taps.cpu(), h.expand(2, -1)) and smp.blind_fit.shape == (2, 2) and smp.blind_probes == [[], []]
    # two different rows: recording r is predict_bwe_long of recording r with row r and the same seed
    rows = torch.stack([h, _taps(7000)])
    out = smp.predict_blind_bwe_long(y, seeds=SEEDS, frozen_taps=rows)
    for r in range(2):
        assert torch.equal(out[r:r + 1], smp.predict_bwe_long(y[r:r + 1], rows[r], "firwin", seeds=SEEDS[r:r + 1])), r


@functools.lru_cache(maxsize=None)
def _live():
    """the live call on the two recordings together, probes = 2: (y, result, blind_fit, blind_taps, blind_probes, evaluations)"""
    smp, Ls = _net()
    y = _recordings(Ls)
    n0 = smp.n_evals
    out = smp.predict_blind_bwe_long(y, probes=2, seeds=SEEDS)
    return y, out, smp.blind_fit.clone(), smp.blind_taps.clone(), smp.blind_probes, smp.n_evals - n0


def test_live_recordings_together_equal_each_alone_and_get_different_filters():
    from audio_inpainting_diffusion_amd import blind_long
    from audio_inpainting_diffusion_amd.sampler import autoregressive_overlap
    smp, Ls = _net()
    y, out, fit, taps, probes, evals = _live()
    N = y.shape[1]
    assert out.shape == (2, N) and bool(torch.isfinite(out).all()) and fit.shape == (2, 2) and taps.shape == (2, BLIND["K"])
    assert evals == (4 + 6) * (2 * T_STEPS - 1)                                          # four probes, then six windows
    print(f"live, reduced network: fitted (Hz, dB/oct) {[(round(float(f[0])), round(float(f[1]), 1)) for f in fit]}, probes {probes}")
    assert not torch.equal(fit[0], fit[1]) and not torch.equal(taps[0], taps[1])
    end = int(autoregressive_overlap(smp.args) * Ls)
    starts = blind_long.candidate_starts(N, Ls, end, BLIND["K"])
    assert starts == [0, Ls - end]
    E = blind_long.window_energy_host(y.cpu().numpy(), starts, Ls)
    assert probes == [[starts[w] for w in c] for c in blind_long.choose_probes(E, 2, 8)]
    for r in range(2):
        alone = smp.predict_blind_bwe_long(y[r:r + 1], probes=2, seeds=SEEDS[r:r + 1])
        assert torch.equal(alone, out[r:r + 1]) and torch.equal(smp.blind_fit, fit[r:r + 1]) and torch.equal(smp.blind_taps, taps[r:r + 1]), r
        assert smp.blind_probes == probes[r:r + 1]
    # stage 2 is predict_bwe_long with the fitted rows
    assert torch.equal(smp.predict_blind_bwe_long(y, seeds=SEEDS, frozen_taps=taps), out)


def test_live_chunks_of_whole_recordings_give_the_same_bits():
    smp, _ = _net()
    y, out, fit, taps, probes, _ = _live()
    two = smp.predict_blind_bwe_long(y, probes=2, max_batch=2, seeds=SEEDS)
    assert torch.equal(two, out) and torch.equal(smp.blind_fit, fit) and torch.equal(smp.blind_taps, taps) and smp.blind_probes == probes


def test_a_recording_shorter_than_a_window_runs_on_window_zero():
    smp, Ls = _net()
    N = Ls - 500
    y = _recordings(Ls, N=N, R=1)
    with _Launches() as names:
        out = smp.predict_blind_bwe_long(y, seeds=[5])
    assert out.shape == (1, N) and bool(torch.isfinite(out).all()) and not torch.equal(out, y) and smp.blind_probes == [[0]]
    assert names.count("aid_window_energy") == 1 and names.count("aid_lowpass_fit_groups") == 2 * T_STEPS - 1
    assert bool(torch.isfinite(smp.blind_fit).all()) and smp.blind_fit.shape == (1, 2)


def test_the_harness_wrapper_groups_files_by_length():
    from audio_inpainting_diffusion_amd import harness
    smp, Ls = _net()
    y, out, fit, taps, probes, _ = _live()
    short = _recordings(Ls, N=Ls + 700, R=1)
    files = [y[0].cpu(), short[0].cpu(), y[1].cpu()]
    res = harness.blind_bwe_long(smp, files, probes=2, seeds=[SEEDS[0], 9, SEEDS[1]], device=DEV)
    assert [t.shape for t in res] == [f.shape for f in files]
    assert torch.equal(res[0], out[0]) and torch.equal(res[2], out[1])
    assert torch.equal(smp.blind_fit[[0, 2]], fit) and torch.equal(smp.blind_taps[[0, 2]], taps) and [smp.blind_probes[0], smp.blind_probes[2]] == probes
    held = smp.blind_taps[1].clone()
    alone = smp.predict_blind_bwe_long(short, probes=2, seeds=[9])
    assert torch.equal(res[1], alone[0]) and torch.equal(held, smp.blind_taps[0])


# ---- three ranks on one GPU ----------------------------------------------------------------------------------------------------------------
WORLD, T_DIST = 3, 2


def _dist_sampler(dev, seed_offset=0):
    from audio_inpainting_diffusion_amd.config import small_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.init import seeded_init_
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    from audio_inpainting_diffusion_amd.sampler import Sampler
    z = np.load(os.path.join(GOLDEN, "unet_small_a.npz"))
    kw = ast.literal_eval(str(z["cfg"]))
    args = small_args(**kw)
    args.tester.T, args.tester.posterior_sampling.xi = T_DIST, 0.25
    args.tester.data_consistency.use = False
    args.tester.blind_bwe = dict(BLIND)
    net = seeded_init_(Unet_CQT_oct_with_attention(args, torch.device(dev)), int(z["seed"]) + seed_offset, gate_scale=10.0, affine_scale=10.0)
    return net, Sampler(model=net, diff_params=EDM(args), args=args), kw["audio_len"]


def _dist_call(smp, Ls, dev):
    y = _recordings(Ls).to(dev)
    n0 = smp.n_evals
    out = smp.predict_blind_bwe_long(y, probes=2, seeds=SEEDS)
    return out.cpu().numpy(), smp.blind_taps.cpu().numpy(), smp.blind_fit.cpu().numpy(), smp.blind_probes, smp.n_evals - n0


def _worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                          AID_DIST_BACKEND="gloo")
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from audio_inpainting_diffusion_amd import dist as D
        D.init_distributed()
        torch.cuda.set_device(0)
        net, smp, Ls = _dist_sampler("cuda:0", seed_offset=rank)                          # ranks start with DIFFERENT weights: the broadcast must fix that
        D.broadcast_parameters(net, src=0)
        res = _dist_call(smp, Ls, "cuda:0")
        D.barrier()
        q.put((rank, res))
        torch.distributed.destroy_process_group()
    except BaseException:
        q.put((rank, traceback.format_exc()))
        raise


def test_three_ranks_on_one_gpu_return_the_single_process_result_and_filters_on_every_rank():
    """Two recordings for three ranks: rank 2 has no recording in stage 1 and contributes [0, K + 4] to the one exchange of the filters; in
    stage 2 it takes its share of the windows (tests/test_gpu_long_dist.py).  Every rank holds the single process's result, taps, fit and
    probes, bit for bit; the ranks' evaluations add up to the single process's."""
    from test_gpu_long_dist import _free_port
    _, smp, Ls = _dist_sampler("cuda")
    want = _dist_call(smp, Ls, "cuda")
    per = 2 * T_DIST - 1
    assert want[4] == (4 + 6) * per and np.isfinite(want[0]).all()
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_worker, args=(r, WORLD, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    got = []
    try:
        for _ in range(WORLD):
            got.append(q.get(timeout=600))
            assert isinstance(got[-1][1], tuple), got[-1][1]
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
    except queue.Empty:
        pytest.fail("a worker did not answer within 600 s")
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join(timeout=10)
    ranks = [res for _, res in sorted(got, key=lambda t: t[0])]
    for rank, res in enumerate(ranks):
        assert np.array_equal(res[0], want[0]) and np.array_equal(res[1], want[1]) and np.array_equal(res[2], want[2]) and res[3] == want[3], rank
    # stage 1: ranks 0 and 1 a recording of two probes each, rank 2 none; stage 2: shard_range of four and two windows
    assert [res[4] for res in ranks] == [(2 + 3) * per, (2 + 2) * per, (0 + 1) * per]
