"""GPU tests of declicking (csrc/aid_declick.hip, declick.py, Sampler.predict_declicking_long, harness.declick_long): aid_ar_score against
declick.score_host, aid_click_mask bit for bit against declick.mask_host, detect against detect_host, the front end on the reduced HIP network
(the recipe of tests/test_gpu_restore_long.py), and the refusals of the two launchers.

THE SCORE BAR.  The kernel does score_host's operations one for one (floating-point contraction is off in the kernel's file) but for the
order in which the products of an autocorrelation lag are added.  What a second order moves is measured on the CPU, on the inputs below:
score_host(autocorr="forward") against score_host(autocorr="pairwise"), the largest relative difference over the samples with a score >= 1,
per case, before the float32 store (``REORDER``; ``python tests/test_gpu_declick.py`` prints that column, no GPU needed).  The bar is
2^-23 + 16 * the largest figure: 2^-23 is the float32 store of the score with a factor 2, the 16 is there because the kernel's order
(256 strided partial sums, then a tree) differs from both.  Below a score of 1 the bar is absolute.  The kernel's worst case on one
MI355X stands next to each figure in ``REORDER``: 0 (the host's float32 bits) in eight of ten cases, one float32 step of one score
(1.179e-07) at block 4096.
"""
import ast
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2
from test_declick_host import signal

pytestmark = pytest.mark.gpu
DEV = "cuda"
# case -> (the CPU figure: forward against pairwise in float64, relative, scores >= 1; the kernel's worst distance from score_host on one MI355X)
REORDER = {
    "three_blocks": (5.408e-12, 0.0), "unscored_tail": (2.329e-13, 0.0), "short": (1.426e-13, 0.0), "defaults": (1.610e-11, 0.0),
    "largest": (1.178e-10, 1.179e-07), "order_one": (1.774e-14, 0.0), "padded": (1.365e-12, 0.0), "border_clicks": (7.466e-12, 0.0),
    "zero_and_constant": (1.464e-12, 0.0), "end_to_end": (1.750e-11, 1.455e-11),
}
BAR = 2.0 ** -23 + 16 * max(v[0] for v in REORDER.values())                  # 1.211e-07: one bar, from the largest figure
E2E_SEED = 11                     # add_clicks seed of the end-to-end case: score_host leaves no sample within the bar of the threshold (asserted)


def score_cases():
    """case -> (y [R, N] float32 numpy, block, order); seeded, shared by the tests here and the CPU measurement of ``REORDER``"""
    c = {"three_blocks": (signal(1000, 21, R=2), 256, 8),                    # three blocks and a scored tail of 232
         "unscored_tail": (signal(300, 22), 256, 8),                         # a tail of 44 < 64
         "short": (signal(200, 23), 256, 8),                                 # N < block
         "defaults": (signal(5000, 24), 2048, 16),                           # ragged at the defaults
         "largest": (signal(4113, 25, R=3), 4096, 32),                       # the largest block, an unscored tail of 17
         "order_one": (signal(1000, 26), 256, 1),
         "padded": (signal(1000, 27, R=2), 256, 8)}
    y = signal(1000, 28)
    y[0, 256] += 0.3                                                         # on the first and on the last sample of block 1: the ringing
    y[0, 511] -= 0.3                                                         # of the second crosses into block 2 through its history
    c["border_clicks"] = (y, 256, 8)
    y = signal(1000, 29)
    y[0, 256:512] = 0.0
    y[0, 512:768] = 0.25
    c["zero_and_constant"] = (y, 256, 8)
    return c


def e2e_input():
    from audio_inpainting_diffusion_amd import declick
    return declick.add_clicks(signal(5000, 30, R=2), 12, seed=E2E_SEED, dropouts=1)


_HOST = {}


def host_score(case):
    """score_host of a case, computed once and shared"""
    from audio_inpainting_diffusion_amd import declick
    if case not in _HOST:
        y, block, order = score_cases()[case]
        _HOST[case] = declick.score_host(y, block=block, order=order)
    return _HOST[case]


def distance(dev, host):
    """the largest distance of a device score plane from the host's: relative where the host score is >= 1, absolute below"""
    d, h = dev.double().cpu(), host.double()
    return float(((d - h).abs() / h.clamp(min=1.0)).max())


# ---- the score ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["three_blocks", "unscored_tail", "short", "defaults", "largest", "order_one", "border_clicks", "zero_and_constant"])
def test_score_against_the_float64_restatement(case):
    from audio_inpainting_diffusion_amd import declick
    y, block, order = score_cases()[case]
    want, want_sigma = host_score(case)
    yd = torch.from_numpy(y).to(DEV)
    s, sigma = declick.score(yd, block=block, order=order)
    worst = distance(s, want)
    print(f"declick score {case}: worst distance {worst:.3e}, bar {BAR:.3e}")
    assert s.shape == yd.shape and sigma.shape == want_sigma.shape and bool(torch.isfinite(s).all())
    assert torch.equal(s.cpu() == 0, want == 0)                              # what is not scored is exactly 0
    assert worst <= BAR
    hs = want_sigma
    assert torch.equal(sigma.cpu() == 0, hs == 0)
    assert float(((sigma.cpu().double() - hs).abs() / hs.clamp(min=1e-30))[hs > 0].max() if bool((hs > 0).any()) else 0.0) <= BAR
    # a second launch gives the same bits; a row alone gives the bits it has in the batch
    s2, sigma2 = declick.score(yd, block=block, order=order)
    assert torch.equal(s, s2) and torch.equal(sigma, sigma2)
    for r in range(y.shape[0]):
        s1, sigma1 = declick.score(yd[r:r + 1], block=block, order=order)
        assert torch.equal(s1[0], s[r]) and torch.equal(sigma1[0], sigma[r])


def test_score_reads_and_writes_rows_of_a_padded_parent_in_place():
    from audio_inpainting_diffusion_amd import declick
    y, block, order = score_cases()["padded"]
    R, N = y.shape
    parent = torch.full((R, N + 5), float("nan"), device=DEV)
    parent[:, 2:N + 2] = torch.from_numpy(y).to(DEV)
    out = torch.full((R, N + 7), float("nan"), device=DEV)
    sig = torch.full((R, 4), float("nan"), device=DEV)
    s, sigma = declick.score(parent[:, 2:N + 2], block=block, order=order, out=out[:, 3:N + 3], sigma_out=sig)
    assert s.data_ptr() == out[:, 3:].data_ptr() and sigma.data_ptr() == sig.data_ptr()
    ref, ref_sigma = declick.score(torch.from_numpy(y).to(DEV), block=block, order=order)
    assert torch.equal(s, ref) and torch.equal(sigma, ref_sigma) and bool(torch.isfinite(s).all())
    assert bool(torch.isnan(out[:, :3]).all()) and bool(torch.isnan(out[:, N + 3:]).all())     # the padding of the output is untouched
    assert distance(s, host_score("padded")[0]) <= BAR


# ---- the mask ----------------------------------------------------------------------------------------------------------------------------------
def _mask_scene(N=6000):
    """(y, score) on the host: runs of 3, 4, 11 (over the tile border at 1024), 1024 and 1025 samples, runs at both ends, a -0.0 / +0.0
    pair; scores above the threshold at 0, N - 1, on either side of the tile border at 2048, and exactly at / one ulp above the threshold"""
    y = torch.randn(N, generator=torch.Generator().manual_seed(40)).numpy().copy()
    for a, b, v in ((100, 103, 0.5), (200, 204, -0.5), (1020, 1031, 0.0), (1500, 2524, 0.125), (3000, 4025, 0.25), (0, 10, 0.7), (N - 10, N, -0.7),
                    (4200, 4206, -0.0), (4206, 4212, 0.0)):
        y[a:b] = v
    s = np.zeros(N, dtype=np.float32)
    s[[0, N - 1, 2047, 2048, 5000]] = 9.0
    s[5200] = 8.0
    s[5300] = np.nextafter(np.float32(8.0), np.float32(9.0))
    return y.astype(np.float32).reshape(1, -1), s.reshape(1, -1)


@pytest.mark.parametrize("pad", [0, 16, 256])
@pytest.mark.parametrize("min_run, max_run", [(0, 1024), (4, 1024), (6, 10), (12, 1024)])
def test_mask_is_the_restatement_bit_for_bit(pad, min_run, max_run):
    from audio_inpainting_diffusion_amd import declick
    y, s = _mask_scene()
    kw = dict(threshold=8.0, pad=pad, min_run=min_run, max_run=max_run)
    want = declick.mask_host(y, s, **kw)
    got = declick.mask(torch.from_numpy(y).to(DEV), torch.from_numpy(s).to(DEV), **kw)
    assert torch.equal(got.cpu(), want)
    f = declick.flags_host(y, s, threshold=8.0, min_run=min_run, max_run=max_run)[0]
    # the scene does what it was built for: the runs of min_run - 1 / max_run + 1 samples and those at the ends are not flagged, the others are
    assert f[5300] and not f[5200] and not f[1:10].any() and not f[-10:-1].any()
    if (min_run, max_run) == (4, 1024):
        assert not f[100:103].any() and f[200:204].all() and f[1020:1031].all() and f[1500:2524].all() and not f[3000:4025].any() and f[4200:4212].all()
    if (min_run, max_run) == (6, 10):
        assert f[4200:4212].all() and not f[1020:1031].any() and not f[200:204].any()
    if min_run == 12:
        assert not f[1020:1031].any() and not f[4200:4212].any() and f[1500:2524].all()
    assert torch.equal(declick.mask(torch.from_numpy(y).to(DEV), torch.from_numpy(s).to(DEV), **kw), got)       # a second launch: the same bits


@pytest.mark.parametrize("N", [1, 2, 1024, 1025, 2049])
def test_mask_at_short_and_ragged_lengths_and_in_a_padded_parent(N):
    from audio_inpainting_diffusion_amd import declick
    R = 3
    g = torch.Generator().manual_seed(50 + N)
    y = torch.randn(R, N, generator=g)
    if N > 1000:
        y[0, N - 20:N - 8] = 0.5                                             # a run short of the end
        y[1, N - 12:] = 0.5                                                  # ... and one that holds the last sample
        y[2, :9] = 0.25
    s = torch.rand(R, N, generator=g) * 8.05                                 # a few scores above the threshold
    s[1, 0], s[2, N - 1] = 9.0, 9.0
    parent_y = torch.full((R, N + 3), float("nan"), device=DEV)
    parent_s = torch.full((R, N + 6), float("nan"), device=DEV)
    parent_y[:, 1:N + 1], parent_s[:, 4:N + 4] = y.to(DEV), s.to(DEV)
    out = torch.full((R, N + 2), float("nan"), device=DEV)
    for pad in (0, 16, 256):
        want = declick.mask_host(y, s, pad=pad)
        got = declick.mask(parent_y[:, 1:N + 1], parent_s[:, 4:N + 4], pad=pad, out=out[:, 1:N + 1])
        assert torch.equal(got.cpu(), want), pad
        assert bool(torch.isnan(out[:, 0]).all()) and bool(torch.isnan(out[:, N + 1]).all())
        for r in range(R):                                                   # a row alone: the bits it has in the batch
            assert torch.equal(declick.mask(y[r:r + 1].to(DEV), s[r:r + 1].to(DEV), pad=pad)[0], got[r])
    assert float((declick.mask_host(y, s) == 0).float().mean()) > 0


# ---- detect --------------------------------------------------------------------------------------------------------------------------------------
def test_detect_against_detect_host_end_to_end():
    """(2, 5000) at the defaults.  The masks agree everywhere but within ``pad`` of a sample whose host score lies within the score bar of
    the threshold; E2E_SEED was chosen so that the host restatement leaves out none, which is asserted."""
    from audio_inpainting_diffusion_amd import declick
    y, truth = e2e_input()
    host = declick.detect_host(y)
    det = declick.detect(torch.from_numpy(y).to(DEV))
    bar = BAR
    worst = distance(det.score, host.score)
    print(f"declick score end_to_end: worst distance {worst:.3e}, bar {bar:.3e}")
    assert worst <= bar
    thr = declick.make_settings().threshold
    close = ((host.score.double() - thr).abs() <= bar * thr).float()
    assert int(close.sum()) == 0                                             # the seed's promise
    leave = declick.mask_host(np.zeros(y.shape, dtype=np.float32), close.numpy(), threshold=0.5, min_run=0) == 0
    assert float(leave.float().mean()) <= 1e-3
    assert torch.equal(det.mask.cpu()[~leave], host.mask[~leave])
    assert torch.equal(det.mask.cpu(), declick.mask_host(y, det.score.cpu()))                                   # exact on the device's own score
    assert bool((det.mask.cpu()[torch.from_numpy(truth)] == 0).all())        # every damaged sample is under the mask
    if not bool(leave.any()):
        assert (det.n_flagged.tolist(), det.n_gaps.tolist(), det.longest_gap.tolist()) == (host.n_flagged.tolist(), host.n_gaps.tolist(), host.longest_gap.tolist())
    assert det.n_gaps.min() >= 1 and float(det.n_flagged.max()) / 5000 < 0.2 and det.sigma.shape == (2, 3)
    sc = declick.detection_scores(det.mask, truth)
    assert sc["recall"] == 1.0 and sc["precision"] > 0.8


# ---- through the reduced network -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_net():
    """(sampler, audio_len) of the reduced HIP network (the recipe of tests/test_gpu_restore_long.py::_small_net), built once for this module
    and released with it.  The projection onto the data is the final, un-smoothed one (data_consistency type "end", smooth off):
    mask * y + (1 - mask) * x gives back y's bits wherever mask is 1."""
    from audio_inpainting_diffusion_amd.config import small_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.init import seeded_init_
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    from audio_inpainting_diffusion_amd.sampler import Sampler
    z = np.load(os.path.join(GOLDEN, "unet_small_a.npz"))
    kw = ast.literal_eval(str(z["cfg"]))
    args = small_args(**kw)
    args.tester.T, args.tester.posterior_sampling.xi = 3, 0.25
    args.tester.data_consistency.use, args.tester.data_consistency.type, args.tester.data_consistency.smooth = True, "end", False
    net = seeded_init_(Unet_CQT_oct_with_attention(args, torch.device(DEV)), int(z["seed"]), gate_scale=10.0, affine_scale=10.0)
    yield Sampler(model=net, diff_params=EDM(args), args=args), kw["audio_len"]


def _recordings(N, R=2):
    """clean recordings and their damaged versions [R, N] on the GPU: a few clicks and one dropout each"""
    from audio_inpainting_diffusion_amd import declick
    x = signal(N, 60, R=R) * np.float32(0.3)
    y, truth = declick.add_clicks(x, 5, seed=61, amplitude=(0.05, 0.2), dropouts=1)
    return torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), torch.from_numpy(truth)


def test_predict_declicking_long_is_predict_inpainting_long_on_the_detected_mask(small_net):
    from audio_inpainting_diffusion_amd import declick
    smp, Ls = small_net
    N = Ls + Ls // 2 + 200
    x, y, truth = _recordings(N)
    seeds = [31, 32]
    det = declick.detect(y)
    assert bool((det.mask.cpu()[truth] == 0).all()) and det.n_flagged.min() > 0
    n0 = smp.n_evals
    out = smp.predict_declicking_long(y, max_batch=8, seeds=seeds)
    evals = smp.n_evals - n0
    ref = smp.predict_inpainting_long(y, det.mask, max_batch=8, seeds=seeds)
    assert evals > 0 and torch.equal(out, ref) and out.shape == y.shape and bool(torch.isfinite(out).all())
    keep = det.mask == 1
    assert torch.equal(out[keep], y[keep]) and not torch.equal(out[~keep], y[~keep])         # mask 1: the recording's bits
    rep = smp.declick_report
    assert rep.score is None and torch.equal(rep.mask, det.mask) and rep.n_flagged.tolist() == det.n_flagged.tolist() and torch.equal(rep.sigma, det.sigma)
    # together / alone, max_batch 2 / 8: the bound for results across batch compositions (tests/test_gpu_restore_long.py: 5e-6, measured 0.0)
    errs = {}
    for r in range(2):
        alone = smp.predict_declicking_long(y[r:r + 1], max_batch=8, seeds=seeds[r:r + 1])
        assert torch.equal(smp.declick_report.mask, det.mask[r:r + 1])
        errs[f"recording {r} alone"] = rel_l2(alone.cpu(), out[r:r + 1].cpu())
    errs["max_batch 2"] = rel_l2(smp.predict_declicking_long(y, max_batch=2, seeds=seeds).cpu(), out.cpu())
    print("declick batch invariance, rel-L2:", {k: "%.2e" % v for k, v in errs.items()})
    assert all(e <= 5e-6 for e in errs.values()), errs
    # known gaps: the product of the two masks is what is restored
    known = torch.ones(N)
    known[Ls // 2:Ls // 2 + 150] = 0
    got = smp.predict_declicking_long(y, seeds=seeds, mask=known)
    both = det.mask * known.to(DEV)
    assert torch.equal(smp.declick_report.mask, both) and smp.declick_report.n_flagged.tolist() == (both == 0).sum(dim=1).tolist() and torch.equal(got, smp.predict_inpainting_long(y, both, seeds=seeds))
    assert not torch.equal(got[:, Ls // 2:Ls // 2 + 150], y[:, Ls // 2:Ls // 2 + 150]) and torch.equal(got[both == 1], y[both == 1])
    # a clean recording: a copy, and nothing is evaluated
    n0 = smp.n_evals
    clean = smp.predict_declicking_long(x, seeds=seeds)
    assert torch.equal(clean, x) and clean.data_ptr() != x.data_ptr() and smp.n_evals == n0 and smp.declick_report.n_flagged.tolist() == [0, 0]
    # more than max_fraction masked: refused by index before the sampler runs
    from audio_inpainting_diffusion_amd import _lib
    with pytest.raises(_lib.AidError, match="recording 1"):
        smp.predict_declicking_long(torch.stack([y[0], declick.add_clicks(y[1].cpu(), 150, seed=3)[0].to(DEV)]), seeds=seeds)
    assert smp.n_evals == n0


def test_harness_declick_long_pooled_equals_not_pooled(small_net):
    from audio_inpainting_diffusion_amd import declick, harness
    smp, Ls = small_net
    _, y, _ = _recordings(Ls + Ls // 2 + 200, R=3)
    files = [y[0].cpu(), y[1, :Ls + 300].cpu(), y[2].cpu()]                   # two lengths: two detect calls, one pooled restoration
    plain, reports = harness.declick_long(smp, files, seeds=[7, 8, 9], max_batch=4, device=DEV, pool=False)
    pooled, reports2 = harness.declick_long(smp, files, seeds=[7, 8, 9], max_batch=4, device=DEV, pool=True)
    for i, f in enumerate(files):
        det = declick.detect(f.reshape(1, -1).to(DEV))
        assert torch.equal(reports[i].mask, det.mask[0]) and torch.equal(reports2[i].mask, det.mask[0]) and int(reports[i].n_flagged) == int(det.n_flagged[0]) > 0
        assert plain[i].shape == pooled[i].shape == f.shape and rel_l2(pooled[i].cpu(), plain[i].cpu()) <= 5e-6
        keep = det.mask[0] == 1
        assert torch.equal(plain[i][keep], f.to(DEV)[keep]) and not torch.equal(plain[i][~keep], f.to(DEV)[~keep])


def test_the_tool_writes_masks_and_the_report_without_a_model(tmp_path, capsys):
    import importlib.util
    import json
    from audio_inpainting_diffusion_amd import declick, harness
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("declick_tool", os.path.join(ROOT, "tools", "declick.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    y, _ = declick.add_clicks(signal(5000, 70, R=2), 6, seed=71, dropouts=1)
    for i, n in enumerate((5000, 3000)):
        harness.write_audio_file(torch.from_numpy(y[i, :n]), 22050, f"take{i}", str(tmp_path / "in"))
    rows = tool.main([str(tmp_path / "in"), str(tmp_path / "out"), "--detect-only", "--json", str(tmp_path / "report.json"), "--pad", "8"])
    assert [r["name"] for r in rows] == ["take0.wav", "take1.wav"] and "longest" in capsys.readouterr().out
    for i, r in enumerate(rows):
        x, fs = harness.read_wav(str(tmp_path / "in" / f"take{i}.wav"))
        det = declick.detect(x.to(DEV), pad=8)
        m, _ = harness.read_wav(str(tmp_path / "out" / "masks" / f"take{i}.wav"))
        assert torch.equal((m != 0).float(), det.mask.cpu()) and r["n_flagged"] == int(det.n_flagged[0]) > 0 and r["n_gaps"] == int(det.n_gaps[0])
    saved = json.load(open(tmp_path / "report.json"))
    assert saved["rows"] == rows and saved["settings"]["pad"] == 8 and saved["settings"]["detect_only"] is True
    with pytest.raises(SystemExit, match="--checkpoint"):
        tool.main([str(tmp_path / "in"), str(tmp_path / "out")])


# ---- the launchers' refusals -----------------------------------------------------------------------------------------------------------------------
def test_launcher_refusals_return_their_code_without_launching():
    import ctypes
    from audio_inpainting_diffusion_amd import _lib
    R, N = 2, 1000
    y = torch.zeros(R, N, device=DEV)
    out = torch.full((R, N), -7.5, device=DEV)
    sig = torch.full((R, 4), -7.5, device=DEV)

    def ar(block=256, order=8, J=4, rec_ld=N, out_ld=N, ridge=1e-6, floor=1e-6, rows=R, n=N):
        sc = (ctypes.c_float * 2)(ridge, floor)
        return lambda: _lib.call("aid_ar_score", _lib.BweGatherParams(y.data_ptr(), ctypes.addressof(sc), out.data_ptr(), sig.data_ptr(), None,
                                                                      J, rows, order, block, n, rec_ld, out_ld))
    for bad in (dict(block=300), dict(block=8192), dict(order=0), dict(order=33), dict(J=3), dict(J=5), dict(rec_ld=N - 1), dict(out_ld=N - 1),
                dict(ridge=-1.0), dict(ridge=float("inf")), dict(floor=0.0), dict(floor=float("nan")), dict(rows=0), dict(rows=65536), dict(n=0)):
        with pytest.raises(_lib.AidError, match="rc=-1"):
            ar(**bad)()

    def cm(thr=8.0, pad=16, lo=8, hi=1024, mode=0, x_ld=N, y_ld=N, out_ld=N, rows=R):
        sc = (ctypes.c_float * 4)(thr, pad, lo, hi)
        return lambda: _lib.call("aid_click_mask", _lib.FirObservedParams(y.data_ptr(), y.data_ptr(), None, ctypes.addressof(sc), out.data_ptr(),
                                                                         rows, 0, mode, N, x_ld, y_ld, 0, out_ld))
    for bad in (dict(thr=0.0), dict(thr=float("inf")), dict(pad=-1), dict(pad=257), dict(pad=1.5), dict(lo=1), dict(lo=2.5), dict(lo=9, hi=8),
                dict(hi=1025), dict(hi=0), dict(mode=1), dict(x_ld=N - 1), dict(y_ld=N - 1), dict(out_ld=N - 1), dict(rows=0), dict(rows=65536)):
        with pytest.raises(_lib.AidError, match="rc=-1"):
            cm(**bad)()
    assert bool((out == -7.5).all()) and bool((sig == -7.5).all())
    ar()()
    cm()()
    torch.cuda.synchronize()
    assert bool((out == 1).all()) and bool((sig == 0).all())                  # silence: nothing scored, nothing flagged (the runs hold the ends)


def reorder_figures():
    """the CPU column of ``REORDER``: forward against pairwise summation of the autocorrelation, in float64, on the inputs of the tests"""
    from audio_inpainting_diffusion_amd import declick
    cases = dict(score_cases(), end_to_end=(e2e_input()[0], 2048, 16))
    out = {}
    for name, (y, block, order) in cases.items():
        a = declick.score_host(y, block=block, order=order, store=np.float64)[0]
        b = declick.score_host(y, block=block, order=order, autocorr="pairwise", store=np.float64)[0]
        out[name] = float(((a - b).abs() / a.clamp(min=1.0))[a >= 1].max()) if bool((a >= 1).any()) else 0.0
    return out


if __name__ == "__main__":
    for k, v in reorder_figures().items():
        print(f"{k:18s} {v:.3e}   bar {2.0 ** -23 + 16 * v:.3e}")
