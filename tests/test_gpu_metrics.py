"""GPU tests of the restoration metrics (csrc/aid_eval.hip, metrics.py): aid_stft_logspec_dist and aid_eval_sums against their float64
restatements at the smallest shapes where they can go wrong, the sentinels of the frames that are not counted, bit-equality of two calls and
of an item alone against the item in a batch, the launchers' refusals, one run on the reduced network, and the command-line tool on two
small folders.

The inputs (tests/test_metrics_host.py: ``signals``) are seeded white noise for the reference and reference + 0.1 * noise for the estimate:
every bin then sits within a few tens of dB of its frame's peak, so the logarithm does not magnify the fp32 rounding of an FFT at empty bins.
That is a condition on the inputs of these tests, not on the kernel.

THE BAR OF THE FRAME DISTANCES.  tests/test_metrics_host.py::FP32_REL holds, per band, how far a float32 torch.stft evaluation of the same
formula lies from the float64 one on these inputs, on the CPU, relative to the float64 value and at its worst over all shapes and frames:
all bins 4.6e-5, one bin 2.1e-4, bins 0 .. N/4 1.8e-5, bins N/4 + 1 .. N/2 4.6e-5 (measured 4.524e-5, 2.054e-4, 1.714e-5, 4.558e-5).  The
kernel is another fp32 FFT with another order of operations and has no claim to be closer: it gets KERNEL_FACTOR = 4 times that.  The bar was
not derived from the kernel's output.
THE BAR OF THE SUMS is the one aid_window_energy is held to: relative 2^-40 against float64 (fp64 sums of exact fp32 products in another
order); the sample count, the frame count and the largest error must be exact."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch

from test_metrics_host import BANDS, FP32_REL, FS, KERNEL_FACTOR, REGIONS, SHAPES, band, region, signals

pytestmark = pytest.mark.gpu
DEV = "cuda"
SUMS_BAR = 2.0 ** -40


@functools.lru_cache(maxsize=None)
def _want_frames(shape, kind):
    """the float64 frame distances of every frame of ``signals(shape)`` over the band, computed once per (shape, band) and shared"""
    from audio_inpainting_diffusion_amd import metrics
    n_fft, hop, L, B = shape
    ref, est = signals(*shape)
    k_lo, k_hi = band(kind, n_fft)
    out = metrics.logspec_dist_host(ref, est, n_fft=n_fft, hop=hop, k_lo=k_lo, k_hi=k_hi)
    out.setflags(write=False)
    return out


def _on_gpu(x, wide):
    """x on the GPU; ``wide``: as rows of a wider buffer (row stride L + 7)"""
    if not wide:
        return x.to(DEV)
    buf = torch.full((x.shape[0], x.shape[1] + 7), 3.0, device=DEV)
    buf[:, 2:2 + x.shape[1]] = x.to(DEV)
    return buf[:, 2:2 + x.shape[1]]


@pytest.mark.parametrize("kind", REGIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_the_two_kernels_against_their_float64_restatements(shape, kind):
    from audio_inpainting_diffusion_amd import metrics
    n_fft, hop, L, B = shape
    wide = shape == (64, 16, 1000, 3)                                                            # x_ld > L
    ref, est = signals(*shape)
    w = region(kind, *shape)
    rd, ed, wd = _on_gpu(ref, wide), _on_gpu(est, wide), None if w is None else _on_gpu(w, wide)
    counted = metrics.counted_frames_host(w, B, L, n_fft, hop)
    for bk in BANDS:
        k_lo, k_hi = band(bk, n_fft)
        frames = metrics.logspec_dist(rd, ed, wd, n_fft=n_fft, hop=hop, k_lo=k_lo, k_hi=k_hi)
        assert frames.shape == (B, 1 + L // hop) and frames.dtype == torch.float32
        got = frames.cpu().double().numpy()
        want = np.where(counted, _want_frames(shape, bk), -1.0)
        assert np.array_equal(got == -1.0, ~counted), (shape, kind, bk)                          # the sentinels sit where the host rule puts them
        assert (got[counted] >= 0).all()
        err = np.abs(got - want)[counted]
        rel = float((err / np.maximum(want[counted], 1e-300)).max()) if counted.any() else 0.0
        print(f"frames {shape} region {kind} band {bk}: {int(counted.sum())} counted, largest relative difference {rel:.3e} "
              f"(bar {KERNEL_FACTOR * FP32_REL[bk]:.1e})")
        assert (err <= KERNEL_FACTOR * FP32_REL[bk] * want[counted]).all(), (shape, kind, bk, rel)
        sums = metrics.eval_sums(rd, ed, wd, frames)
        assert sums.shape == (B, 8) and sums.dtype == torch.float64
        s = sums.cpu().numpy()
        ws = metrics.eval_sums_host(ref, est, w, got)
        srel = float((np.abs(s - ws) / np.maximum(np.abs(ws), 1e-300)).max())
        print(f"sums   {shape} region {kind} band {bk}: largest relative difference {srel:.2e} (2^{math.log2(max(srel, 1e-300)):.1f})")
        assert (np.abs(s - ws) <= SUMS_BAR * np.abs(ws)).all(), (shape, kind, bk, s, ws)
        assert np.array_equal(s[:, [0, 5, 6]], ws[:, [0, 5, 6]])                                 # n, max |r - e| and the counted frames: exact
        assert np.array_equal(s[:, 6], counted.sum(axis=1))
        assert torch.equal(metrics.logspec_dist(rd, ed, wd, n_fft=n_fft, hop=hop, k_lo=k_lo, k_hi=k_hi), frames)      # a second launch: the same bits
        assert torch.equal(metrics.eval_sums(rd, ed, wd, frames), sums)
    # the whole of evaluate on the last band against evaluate_host
    hz = FS / n_fft
    m = metrics.evaluate(rd, ed, wd, sample_rate=FS, n_fft=n_fft, hop=hop, band=(k_lo * hz, k_hi * hz))
    mh = metrics.evaluate_host(ref, est, w, sample_rate=FS, n_fft=n_fft, hop=hop, band=(k_lo * hz, k_hi * hz))
    assert torch.equal(m["lsd_frames"], frames)
    for k in ("n_samples", "n_frames", "max_abs_err"):
        assert torch.equal(m[k].isnan(), mh[k].isnan()) and torch.equal(m[k].nan_to_num(-7.0), mh[k].nan_to_num(-7.0)), k
    for k in ("lsd", "snr_db", "si_sdr_db"):
        assert m[k].dtype == torch.float64 and m[k].shape == (B,) and torch.equal(m[k].isnan(), mh[k].isnan()), k
        a, b = m[k].nan_to_num(0.0, 1e9, -1e9), mh[k].nan_to_num(0.0, 1e9, -1e9)
        # lsd: the frames' bar.  The dB figures: 10 log10 of a ratio of sums that each hold 2^-40; the denominator of si_sdr cancels to about
        # 1 / 100 of its terms on these inputs (est = ref + 0.1 noise), which multiplies what they hold by some 300: 1000 * 2^-40 covers both
        tol = KERNEL_FACTOR * FP32_REL[bk] * b.abs() if k == "lsd" else torch.full_like(b, 10 / math.log(10) * 1000 * SUMS_BAR)
        assert bool(((a - b).abs() <= tol).all()), (k, a, b)
    if kind == "empty":
        assert math.isnan(m["lsd"][0]) and math.isnan(m["snr_db"][0]) and m["n_samples"][0] == 0 and m["n_frames"][0] == 0


@pytest.mark.parametrize("shape", [(64, 16, 1000, 3), (2048, 512, 5000, 3)], ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("kind", ["none", "run"])
def test_an_item_alone_is_the_item_in_a_batch_of_three_bit_for_bit(shape, kind):
    from audio_inpainting_diffusion_amd import metrics
    n_fft, hop, L, B = shape
    ref, est = signals(*shape)
    w = region(kind, *shape)
    if w is not None:
        w[1] = w[1].roll(37)                                                                     # (the items do not share one region)
    rd, ed, wd = ref.to(DEV), est.to(DEV), None if w is None else w.to(DEV)
    frames = metrics.logspec_dist(rd, ed, wd, n_fft=n_fft, hop=hop)
    sums = metrics.eval_sums(rd, ed, wd, frames)
    for b in range(B):
        wb = None if wd is None else wd[b:b + 1]
        fb = metrics.logspec_dist(rd[b:b + 1], ed[b:b + 1], wb, n_fft=n_fft, hop=hop)
        assert torch.equal(fb, frames[b:b + 1]) and torch.equal(metrics.eval_sums(rd[b:b + 1], ed[b:b + 1], wb, fb), sums[b:b + 1]), b
    if wd is not None:                                                                           # one shared row (state_ld = 0) is that row for every item
        shared = metrics.logspec_dist(rd, ed, wd[:1], n_fft=n_fft, hop=hop)
        assert torch.equal(shared, metrics.logspec_dist(rd, ed, wd[:1].expand(B, L).contiguous(), n_fft=n_fft, hop=hop))
        assert torch.equal(metrics.eval_sums(rd, ed, wd[:1], shared), metrics.eval_sums(rd, ed, wd[:1].expand(B, L).contiguous(), shared))


def test_every_refusal_of_the_launchers_is_the_python_error_and_nothing_is_launched():
    from audio_inpainting_diffusion_amd import _lib, metrics
    n_fft, hop, L, B = 64, 16, 200, 2
    T = 1 + L // hop
    x, y, w = (torch.randn(B, L, device=DEV) for _ in range(3))
    window, twiddle = metrics.tables(n_fft, DEV)
    out = torch.full((B, T), 7.0, device=DEV)
    sums = torch.full((B, 8), 7.0, dtype=torch.float64, device=DEV)
    args = dict(x=x.data_ptr(), g=y.data_ptr(), state=w.data_ptr(), window=window.data_ptr(), twiddle=twiddle.data_ptr(), band=(0.0, 32.0, 1e-10),
                out=out.data_ptr(), L=L, x_ld=L, g_ld=L, state_ld=L, out_ld=T, B=B, n_fft=n_fft, hop=hop, n_frames=T, mode=0)

    def dist(**kw):
        a = dict(args, **kw)
        bandv = None if a["band"] is None else (ctypes.c_float * 3)(*a["band"])
        _lib.call("aid_stft_logspec_dist", _lib.StftMagObservedParams(
            a["x"], a["g"], a["state"], a["window"], a["twiddle"], None if bandv is None else ctypes.addressof(bandv), a["out"],
            a["L"], a["x_ld"], a["g_ld"], a["state_ld"], a["out_ld"], a["B"], a["n_fft"], a["hop"], a["n_frames"], a["mode"]))
    for bad, why in ((dict(n_fft=48), "power of two"), (dict(n_fft=8), "power of two"), (dict(n_fft=16384), "power of two"),
                     (dict(hop=65), r"hop must be in \[1, n_fft\]"), (dict(hop=0), "hop must be"),
                     (dict(band=(0.0, 33.0, 1e-10)), "k_lo <= k_hi <= n_fft / 2"), (dict(band=(5.0, 4.0, 0.0)), "k_lo <= k_hi"),
                     (dict(band=(-1.0, 4.0, 0.0)), "0 <= k_lo"), (dict(band=(1.5, 4.0, 0.0)), "whole bins"), (dict(band=(0.0, 4.0, -1.0)), "floor"),
                     (dict(band=(0.0, 4.0, float("nan"))), "floor"), (dict(mode=1), "mode must be 0"),
                     (dict(x=None), "null pointer"), (dict(g=None), "null pointer"), (dict(out=None), "null pointer"), (dict(window=None), "null pointer"),
                     (dict(twiddle=None), "null pointer"), (dict(band=None), "null pointer"),
                     (dict(x_ld=L - 1), "row stride"), (dict(g_ld=L - 1), "row stride"), (dict(state_ld=L - 1), "weights' row stride"),
                     (dict(out_ld=T - 1), "shorter than n_frames"), (dict(n_frames=T + 1), r"1 \+ L / hop"), (dict(B=0), "bad shape"), (dict(L=0), "bad shape")):
        with pytest.raises(_lib.AidError, match="aid_stft_logspec_dist failed.*" + why):
            dist(**bad)
    dist(state=None)                                                                             # (no weights is not a refusal)
    torch.cuda.synchronize()
    assert bool((out[:, :T - 1] >= 0).all())
    out.fill_(7.0)
    fr = torch.rand(B, T, device=DEV)
    sargs = dict(x=x.data_ptr(), y=y.data_ptr(), state=w.data_ptr(), h=fr.data_ptr(), out=sums.data_ptr(), B=B, K=T, mode=0, L=L, x_ld=L, y_ld=L, state_ld=L)

    def launch(**kw):
        a = dict(sargs, **kw)
        _lib.call("aid_eval_sums", _lib.FirObservedParams(a["x"], a["y"], a["state"], a["h"], a["out"], a["B"], a["K"], a["mode"], a["L"],
                                                          a["x_ld"], a["y_ld"], a["state_ld"], 0))
    for bad, why in ((dict(x=None), "null pointer"), (dict(y=None), "null pointer"), (dict(h=None), "null pointer"), (dict(out=None), "null pointer"),
                     (dict(mode=1), "mode must be 0"), (dict(B=0), "empty shape"), (dict(L=0), "empty shape"), (dict(K=0), "empty shape"),
                     (dict(x_ld=L - 1), "row stride"), (dict(y_ld=L - 1), "row stride"), (dict(state_ld=1), "weights' row stride"),
                     (dict(out=sums.data_ptr() + 4), "8-byte aligned")):
        with pytest.raises(_lib.AidError, match="aid_eval_sums failed.*" + why):
            launch(**bad)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((sums == 7.0).all())                                # none of the refused calls reached the GPU


def test_a_restoration_of_the_reduced_network_is_evaluated_over_its_gap_and_outside_it():
    """predict_inpainting on the reduced network of the other GPU tests (seeded random weights, so NO quality threshold: only what must hold).
    The sampler runs with the replacement branch (xi = 0) and a hard mask (data_consistency.smooth = False, one last projection at the end): the
    result is then the observation itself, bit for bit, at every observed sample -- which the complementary region measures."""
    from audio_inpainting_diffusion_amd import metrics
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.sampler import Sampler
    from test_gpu_network import _net_from_golden
    net, z, kw, args = _net_from_golden("a")
    args.tester.T, args.tester.posterior_sampling.xi = 3, 0.0
    args.tester.data_consistency.type, args.tester.data_consistency.smooth = "end", False
    Ls = kw["audio_len"]
    ref = (torch.from_numpy(z["x"]) * 0.126).to(DEV)
    mask = torch.ones(1, Ls)
    mask[:, 1800:2300] = 0
    smp = Sampler(model=net, diff_params=EDM(args), args=args, rid=False)
    smp.seeds = [5, 6]
    est = smp.predict_inpainting(ref * mask.to(DEV), mask.to(DEV))
    gap, _ = metrics.region_of("inpainting", mask=mask)
    m = metrics.evaluate(ref, est, gap.to(DEV), sample_rate=FS, n_fft=256, hop=64)
    print({k: v.tolist() for k, v in m.items() if k != "lsd_frames"})
    B = ref.shape[0]
    assert m["n_samples"].tolist() == [500.0] * B
    # the frames that touch [1800, 2300): 64 t <= 2299 and 64 t + 256 > 1800
    assert m["n_frames"].tolist() == [float(sum(1 for t in range(1 + Ls // 64) if 64 * t <= 2299 and 64 * t + 256 > 1800))] * B
    for k in ("lsd", "snr_db", "si_sdr_db", "max_abs_err"):
        assert bool(torch.isfinite(m[k]).all()), k
    out = metrics.evaluate(ref, est, mask.to(DEV), sample_rate=FS, n_fft=256, hop=64)
    assert out["n_samples"].tolist() == [float(Ls - 500)] * B and out["max_abs_err"].tolist() == [0.0] * B
    assert out["snr_db"].tolist() == [math.inf] * B


def test_the_tool_prints_the_table_of_two_small_folders(tmp_path, capsys):
    """tools/evaluate.py in this process (main(argv)): three recordings of two lengths written by harness.write_audio_file, paired by name"""
    import importlib.util
    import json
    from audio_inpainting_diffusion_amd import harness, metrics
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("evaluate_tool", os.path.join(ROOT, "tools", "evaluate.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    refs = {}
    for i, n in enumerate((3000, 4100, 3000)):
        g = torch.Generator().manual_seed(40 + i)
        r = 0.2 * torch.randn(n, generator=g)
        refs[f"take{i}"] = r
        harness.write_audio_file(r, FS, f"take{i}", str(tmp_path / "ref"))
        harness.write_audio_file(r + 0.02 * torch.randn(n, generator=g), FS, f"take{i}", str(tmp_path / "est"))
    rows, summary = tool.main([str(tmp_path / "ref"), str(tmp_path / "est"), "--n-fft", "256", "--hop", "64", "--task", "bwe", "--cutoff-hz", "3000",
                               "--json", str(tmp_path / "out.json")])
    text = capsys.readouterr().out
    print(text)
    assert all(f"take{i}.wav" in text for i in range(3)) and "median" in text and "3 files" in text
    # the files as they were written (16-bit), evaluated by the float64 restatement
    for i, row in enumerate(rows):
        r, e = (harness.read_wav(str(tmp_path / d / f"take{i}.wav"))[0] for d in ("ref", "est"))
        want = metrics.evaluate_host(r, e, sample_rate=FS, n_fft=256, hop=64, band=(3000, FS / 2))
        assert row["n_samples"] == r.numel() and abs(row["snr_db"] - float(want["snr_db"])) < 1e-9
        assert abs(row["lsd"] - float(want["lsd"])) <= KERNEL_FACTOR * FP32_REL["high"] * float(want["lsd"])     # (white noise again: the frames' bar)
    saved = json.load(open(tmp_path / "out.json"))
    assert saved["settings"]["band"] == [3000.0, FS / 2] and [r["name"] for r in saved["rows"]] == [f"take{i}.wav" for i in range(3)]
    assert saved["summary"]["snr_db"]["n_not_finite"] == 0 and abs(saved["summary"]["snr_db"]["mean"] - sum(r["snr_db"] for r in rows) / 3) < 1e-12
    # a pair whose lengths differ is refused by name
    harness.write_audio_file(refs["take1"][:4000], FS, "take1", str(tmp_path / "est"))
    with pytest.raises(SystemExit, match="take1.wav: the reference has 4100 samples, the estimate 4000"):
        tool.main([str(tmp_path / "ref"), str(tmp_path / "est")])
