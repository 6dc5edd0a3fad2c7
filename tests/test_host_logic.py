"""CPU tests (no GPU): host-side logic of the product package and the C-ABI surface.

 * libaid_hip.so loads here and answers its host queries (no compute calls; the C ABI itself: tests/test_abi_host.py);
 * the product's vectorised CQT plan equals the oracle's band-by-band design, and a numpy emulation of the
   device algorithm (gather * window -> power-of-two inverse FFT; FFT * dual window -> overlap-add) built
   from the plan's tables reproduces the oracle transform;
 * drop-in surface: state_dict keys/shapes equal the reference module's (recorded in the golden fixtures),
   the plugin classes resolve through the dotted-string mechanism the reference uses;
 * EDM host schedule == golden; smooth-mask construction == oracle; the product fails loudly without a GPU.
"""
import ast
import importlib
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, rel_l2


def test_pack_dims_of_the_library():
    from audio_inpainting_diffusion_amd import _lib
    a, b = _lib.pack_dims(2, 96)
    assert (a, b) == (32, 96)
    assert _lib.pack_dims(256, 256) == (256, 256) and _lib.pack_dims(40, 5120) == (64, 5120) and _lib.pack_dims(64, 192) == (64, 192)


@pytest.mark.parametrize("cfg", [(7, 64, 22050, 184184), (8, 64, 44100, 368368), (7, 8, 22050, 16384), (3, 8, 22050, 2048)])
def test_cqt_plan_matches_oracle_design(cfg):
    from audio_inpainting_diffusion_amd.cqt import CQTPlan
    from oracle.nsgt_cqt import OracleCQT
    no, bpo, fs, L = cfg
    P, O = CQTPlan(no, bpo, fs, L, ("kaiser", 1.0)), OracleCQT(no, bpo, "oct", ("kaiser", 1), fs, L)
    K = no * bpo
    assert P.T_oct == O.size_per_oct
    assert np.array_equal(P.Lg, O.Lg[1:K + 1]) and np.array_equal(P.rc, O.rc[1:K + 1])
    assert np.allclose(P.g, np.concatenate(O.g[1:K + 1]), rtol=1e-6)
    assert np.allclose(P.gdM, np.concatenate([O.gd[k] * O.M[k] for k in range(1, K + 1)]), rtol=1e-5)
    assert np.allclose(P.hpf, O.Hhpf.numpy(), atol=1e-6)


def _emulate_device_cqt(P, x):
    """numpy restatement of csrc/aid_cqt.hip driven by the plan tables (float64)."""
    B, L = x.shape
    X = np.fft.rfft(x, axis=-1)
    coefs, ws = [], np.zeros((B, P.ws_per_b), dtype=complex)
    for k in range(P.K):
        T, Lg, rc = int(P.Tk[k]), int(P.Lg[k]), int(P.rc[k])
        j = np.arange(Lg) - Lg // 2
        buf = np.zeros((B, T), dtype=complex)
        buf[:, (j + T) & (T - 1)] = X[:, rc + j] * P.g[P.goff[k]:P.goff[k] + Lg]
        c = np.fft.ifft(buf, axis=-1)
        coefs.append(c)
        ws[:, P.woff[k]:P.woff[k] + T] = np.fft.fft(c, axis=-1)
    Y = np.zeros((B, P.Lh), dtype=complex)
    for v in range(P.Lh):
        for k in range(P.kfirst[v], P.kfirst[v] + P.kcount[v]):
            jj = v - int(P.rc[k])
            idx = jj + int(P.Lg[k]) // 2
            if 0 <= idx < P.Lg[k]:
                T = int(P.Tk[k])
                Y[:, v] += ws[:, P.woff[k] + ((jj + T) & (T - 1))] * P.gdM[P.goff[k] + idx]
    return coefs, np.fft.irfft(Y, n=L, axis=-1)


def test_cqt_device_algorithm_emulation_matches_oracle():
    from audio_inpainting_diffusion_amd.cqt import CQTPlan
    from oracle.nsgt_cqt import OracleCQT
    no, bpo, fs, L = 3, 8, 22050, 2048
    P, O = CQTPlan(no, bpo, fs, L, ("kaiser", 1.0)), OracleCQT(no, bpo, "oct", ("kaiser", 1), fs, L, dtype=torch.float64)
    x = torch.randn(2, L, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    coefs, y = _emulate_device_cqt(P, x.numpy())
    ref = O.fwd(x[:, None])
    for o in range(no):
        got = np.stack(coefs[o * bpo:(o + 1) * bpo], axis=1)
        assert rel_l2(torch.view_as_real(torch.from_numpy(got)), torch.view_as_real(ref[o][:, 0])) < 1e-6
    assert rel_l2(y, O.apply_hpf_DC(x)) < 1e-6          # bwd(fwd(x)) == apply_hpf_DC(x)


def test_oracle_cqt_properties():
    """CQT parity is unpinned (no reference source): the oracle is held to the NSGT properties instead."""
    from oracle.nsgt_cqt import OracleCQT
    L, fs = 16384, 22050
    q = OracleCQT(7, 8, "oct", ("kaiser", 1), fs, L, dtype=torch.float64)
    g = torch.Generator().manual_seed(1)
    x, x2 = torch.randn(1, L, dtype=torch.float64, generator=g), torch.randn(1, L, dtype=torch.float64, generator=g)
    c = q.fwd(x[:, None])
    assert [ci.shape[-1] for ci in c] == q.size_per_oct and all(a * 2 == b for a, b in zip(q.size_per_oct, q.size_per_oct[1:]))
    h = q.apply_hpf_DC(x)
    assert rel_l2(q.bwd(c)[:, 0], h) < 1e-10                      # perfect reconstruction
    assert rel_l2(q.apply_hpf_DC(h), h) < 0.2 and rel_l2(q.apply_hpf_DC(h), h) >= 0   # smooth projector (not idempotent by design)
    c2 = q.fwd((2 * x + 3 * x2)[:, None])
    cx2 = q.fwd(x2[:, None])
    assert all(rel_l2(torch.view_as_real(a), torch.view_as_real(2 * b + 3 * d)) < 1e-10 for a, b, d in zip(c2, c, cx2))
    # pure tone lands in the expected octave / bin
    k, o = 3, 4
    f0 = (fs / 2) / 2 ** 7 * 2 ** ((o * 8 + k) / 8)
    tone = torch.sin(2 * np.pi * f0 * torch.arange(L, dtype=torch.float64) / fs)[None]
    e = torch.stack([ci.abs().pow(2).sum(-1)[0, 0] * (q.size_per_oct[-1] / ci.shape[-1]) for ci in q.fwd(tone[:, None])])
    assert int(e.flatten().argmax()) == o * 8 + k


def test_state_dict_surface_matches_reference():
    from audio_inpainting_diffusion_amd.config import make_args, small_args
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    for tag in ("a", "b"):
        z = np.load(os.path.join(GOLDEN, f"unet_small_{tag}.npz"))
        kw = ast.literal_eval(str(z["cfg"]))
        net = Unet_CQT_oct_with_attention(small_args(**kw), torch.device("cpu"))
        sd = net.state_dict()
        assert list(sd.keys()) == list(z["keys"])
        assert [repr(tuple(v.shape)) for v in sd.values()] == list(z["shapes"])
    # the product refuses to compute without a GPU instead of falling back
    net = Unet_CQT_oct_with_attention(small_args(), torch.device("cpu"))
    from audio_inpainting_diffusion_amd._lib import AidError
    with pytest.raises(AidError):
        net(torch.zeros(1, 4096), torch.zeros(1, 1))


def test_plugin_strings_resolve_like_the_reference_does():
    """utils/dnnlib/util.py:235-273 resolves `callable` strings with importlib.import_module on dotted prefixes.
    Both spellings of the package (the importable one and the repository's hyphenated alias) must resolve to the
    SAME class objects -- one identity for isinstance / pickling, one loaded libaid_hip.so."""
    for tail in ("network.Unet_CQT_oct_with_attention", "sampler.Sampler", "edm.EDM"):
        objs = []
        for pkg in ("audio_inpainting_diffusion_amd", "audio-inpainting-diffusion_amd"):
            mod, _, attr = (pkg + "." + tail).rpartition(".")
            objs.append(getattr(importlib.import_module(mod), attr))
        assert callable(objs[0]) and objs[0] is objs[1]
        assert objs[0].__module__.startswith("audio_inpainting_diffusion_amd.")
    import audio_inpainting_diffusion_amd._lib as a
    b = importlib.import_module("audio-inpainting-diffusion_amd._lib")
    assert a is b


def test_edm_host_schedule_matches_golden():
    from audio_inpainting_diffusion_amd.config import make_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.sampler import Sampler
    z = np.load(os.path.join(GOLDEN, "edm_schedule.npz"))
    args = make_args()
    edm = EDM(args)
    Sampler(model=None, diff_params=edm, args=args)          # applies tester.diff_params like the reference (:43-53)
    for T in (35, 36, 70, 128):
        t = edm.create_schedule(T)
        assert np.array_equal(t.numpy(), z[f"t{T}"]) and np.array_equal(edm.get_gamma(t).numpy(), z[f"gamma{T}"])
    s = torch.from_numpy(z["sigma"])
    for n in ("cskip", "cout", "cin", "cnoise"):
        assert np.array_equal(getattr(edm, n)(s).numpy(), z[n])


def test_smooth_mask_matches_oracle_and_reference_geometry():
    from audio_inpainting_diffusion_amd.sampler import prepare_smooth_mask
    from oracle.sampler import smooth_mask_rows
    L = 184184
    gap = int(300 * 22050 / 1000)
    start = L // 2 - gap // 2
    assert (gap, start) == (6615, 88785)                      # SURVEY.md section 8c closed form
    m = torch.ones(2, L)
    m[0, start:start + gap] = 0
    m[1, 1000:1400] = 0
    m[1, 90000:90800] = 0
    a, b = prepare_smooth_mask(m, 50), smooth_mask_rows(m, 50)
    assert torch.equal(a, b)
    assert float(a[0, start - 1]) < 1e-3 and float(a[0, start - 50]) == 1.0 and float(a[0, start + gap]) == 0.0


def test_masks_match_reference_prepare_mask_geometry():
    """Closed forms quoted in SURVEY.md section 8c: 300 ms @22050 -> 6615 samples from 88785; 1.5 s @44100 -> 66150;
    25/50/100 ms @16 kHz -> 400/800/1600 samples, 4 gaps."""
    from audio_inpainting_diffusion_amd.config import make_args
    from audio_inpainting_diffusion_amd.masks import long_gap_mask, mask_from_args, short_gaps_mask
    from audio_inpainting_diffusion_amd.sampler import prepare_smooth_mask
    L = 184184
    m = long_gap_mask(L, 22050, 300)
    z = (m[0] == 0).nonzero().flatten()
    assert (len(z), int(z[0])) == (6615, 88785)
    assert int((long_gap_mask(L, 44100, 1500)[0] == 0).sum()) == 66150
    for ms, n in ((25, 400), (50, 800), (100, 1600)):
        g = torch.Generator().manual_seed(ms)
        m = short_gaps_mask(L, 16000, ms, 4, g)
        assert (m == 0).sum() <= 4 * n and (m == 0).sum() >= n
        sm = prepare_smooth_mask(m, 100)
        assert float(sm.min()) == 0.0 and float(sm.max()) == 1.0 and torch.all(sm >= m * 0)   # cross-fades stay in [0,1]
    a = make_args("librispeech16k", T=70, gap_ms=50.0)
    assert a.tester.T == 70 and a.tester.data_consistency.hann_size == 100
    assert mask_from_args(a, torch.Generator().manual_seed(0)).shape == (1, L)
    assert torch.equal(mask_from_args(make_args("maestro22k", gap_ms=300.0)), long_gap_mask(L, 22050, 300))


def _emulate_stft_kernels(x, mask, L, n_fft, hop, win, adjoint):
    """numpy transcription of csrc/aid_stft.hip (frames kernel + overlap-add gather) in float64."""
    from audio_inpainting_diffusion_amd.stft import stft_tables
    w, env, _ = stft_tables(L, n_fft, hop, win)
    Lp, N, half = len(env), n_fft, n_fft // 2
    nfr = 1 + Lp // hop
    B = x.shape[0]
    fr = np.zeros((B, nfr, N))
    f = np.arange(N)
    fm = np.where(f <= half, f, N - f)
    for n in range(nfr):
        q = n * hop - half + np.arange(N)
        if adjoint:
            inside, qq = (q >= 0) & (q < Lp), np.clip(q, 0, Lp - 1)
        else:
            qq = np.where(q < 0, -q, q)
            qq = np.where(qq >= Lp, 2 * (Lp - 1) - qq, qq)
            inside = np.ones(N, bool)
        ok = inside & (qq < L)
        v = np.where(ok, x[:, np.minimum(qq, L - 1)], 0.0)
        if adjoint:
            v = v * np.where(ok, 1.0 / env[qq], 0.0)
        fr[:, n] = np.fft.ifft(np.fft.fft(v * w, axis=-1) * mask[fm, n], axis=-1).real * w

    def cover(pos):
        q = pos + half
        n1 = min(q // hop, nfr - 1)
        n0 = 0 if q - (N - 1) < 0 else -(-(q - (N - 1)) // hop)
        return sum((fr[:, n, q - n * hop] for n in range(n0, n1 + 1)), np.zeros(B))

    out = np.zeros((B, L))
    for t in range(L):
        v = cover(t)
        if adjoint:
            if 1 <= t <= half:
                v = v + cover(-t)
            r = 2 * (Lp - 1) - t
            if Lp <= r < Lp + half:
                v = v + cover(r)
        else:
            v = v / env[t]
        out[:, t] = v
    return out


@pytest.mark.parametrize("case", [(1000, 64, 16, 64), (1024, 64, 16, 64), (777, 128, 32, 128), (1500, 64, 16, 32)])
def test_stft_mask_device_algorithm_and_adjoint_match_oracle(case):
    """The frame/overlap-add decomposition the HIP kernels use (and its transposed border handling) equals
    torch.stft -> mask -> torch.istft and the gradient autograd takes through it."""
    from oracle.sampler import spectral_mask_apply
    L, n_fft, hop, win = case
    Lp = L + (n_fft - L % n_fft)
    rng = np.random.default_rng(0)
    mask = (rng.random((n_fft // 2 + 1, 1 + Lp // hop)) > 0.3).astype(np.float64)
    x, g = rng.standard_normal((2, L)), rng.standard_normal((2, L))
    xt = torch.from_numpy(x).requires_grad_()
    ref = spectral_mask_apply(xt, torch.from_numpy(mask), n_fft, hop, win)
    (ref * torch.from_numpy(g)).sum().backward()
    assert rel_l2(_emulate_stft_kernels(x, mask, L, n_fft, hop, win, 0), ref.detach()) < 1e-7
    assert rel_l2(_emulate_stft_kernels(g, mask, L, n_fft, hop, win, 1), xt.grad) < 1e-7


def test_spectral_mask_matches_reference_prepare_spectral_mask_geometry():
    """tester_inpainting.py:256-294 with conf/tester/inpainting_tester.yaml:78-87 at 22.05 kHz, L=184184."""
    from audio_inpainting_diffusion_amd.config import make_args
    from audio_inpainting_diffusion_amd.masks import spectral_mask_from_args
    A = spectral_mask_from_args(make_args("maestro22k"))
    assert tuple(A.shape) == (513, 721)
    zr, zc = np.nonzero((A == 0).any(1).numpy())[0], np.nonzero((A == 0).any(0).numpy())[0]
    assert (zr[0], zr[-1] + 1) == (14, 93)              # 300 Hz .. 2 kHz in 21.53 Hz bins
    assert (zc[0], zc[-1] + 1) == (273, 445)            # (92092 - 22050)//256, + 44100//256
    assert int((A == 0).sum()) == (93 - 14) * (445 - 273)


def test_checkpoint_loading_strategies_and_long_file_window():
    """harness.load_checkpoint follows utils/training_utils.py:214-289 (strict -> non-strict -> shape-matched);
    centre_gap_window reproduces tester_inpainting.py:399-411."""
    from audio_inpainting_diffusion_amd.config import small_args
    from audio_inpainting_diffusion_amd.harness import centre_gap_window, load_checkpoint
    from audio_inpainting_diffusion_amd.init import seeded_init_
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    src = seeded_init_(Unet_CQT_oct_with_attention(small_args(), torch.device("cpu")), 1)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    dst = Unet_CQT_oct_with_attention(small_args(), torch.device("cpu"))
    from audio_inpainting_diffusion_amd.harness import UnpinnedCQTError
    with pytest.raises(UnpinnedCQTError, match="NOT pinned to cqt_nsgt_pytorch"):    # trained weights on an unpinned CQT: refused by default
        load_checkpoint(dst, {"it": 750000, "ema": sd}, cqt_pinned=False)
    with pytest.warns(RuntimeWarning, match="NOT pinned to cqt_nsgt_pytorch"):      # ... and loud when the caller opts out
        assert load_checkpoint(dst, {"it": 750000, "ema": sd}, cqt_pinned=False, allow_unpinned_cqt=True) == (750000, "strict")
    assert all(torch.equal(a, b) for a, b in zip(dst.state_dict().values(), sd.values()))
    k0 = next(k for k in sd if k.endswith("H.0.weight"))
    extra = dict(sd, **{"not.a.parameter": torch.zeros(3)})
    del extra[k0]
    dst = Unet_CQT_oct_with_attention(small_args(), torch.device("cpu"))
    assert load_checkpoint(dst, {"ema": extra}, allow_unpinned_cqt=True) == (0, "non-strict")
    bad = dict(sd)
    bad[k0] = torch.zeros(1, 2, 3)                                   # wrong shape: only the third strategy survives
    dst = Unet_CQT_oct_with_attention(small_args(), torch.device("cpu"))
    before = dst.state_dict()[k0].clone()
    assert load_checkpoint(dst, {"ema": bad}, allow_unpinned_cqt=True)[1] == "shape-matched"
    assert torch.equal(dst.state_dict()[k0], before)
    k1 = next(k for k in sd if k.endswith("H.1.weight"))
    assert torch.equal(dst.state_dict()[k1], sd[k1])
    assert load_checkpoint(dst, {"ema": {"nothing": torch.zeros(1)}}, allow_unpinned_cqt=True)[1] == "non-strict"      # (as the reference: attempt 2 accepts it)
    with pytest.raises(ValueError):
        load_checkpoint(dst, {"ema": {k0: torch.zeros(1, 2, 3)}}, allow_unpinned_cqt=True)                            # nothing matches by name AND shape
    # 6 s file at 22.05 kHz, 1.5 s gap, 184184-sample model window
    assert centre_gap_window(132300 * 2, 184184, 33075) == (132300 - 16537, 132300 - 92092)
    with pytest.raises(ValueError):
        centre_gap_window(1000, 184184, 10)


def test_resampling_kernel_tables_wav_io_and_case_logic(tmp_path):
    """harness._sinc_kernel == the oracle's restatement of torchaudio's default kernel; write_audio_file (utils/logging.py:295-319)
    round-trips through read_wav; oracle resample: tone in -> same tone out, lengths ceil(new*L/orig)."""
    from audio_inpainting_diffusion_amd.harness import _sinc_kernel, read_wav, write_audio_file
    from oracle.resample import resample, resample_batch, sinc_resample_kernel
    for o, n in ((2, 1), (320, 147), (160, 147), (441, 160), (147, 320)):
        k, w = sinc_resample_kernel(o, n)
        k2, w2 = _sinc_kernel(o, n)
        assert w == w2 and k.shape[-1] == 2 * w + o and float(np.abs(k[:, 0].numpy() - k2).max()) < 1e-15
    t = torch.arange(48000, dtype=torch.float64) / 48000
    x = torch.sin(2 * np.pi * 1000 * t)[None]
    y = resample(x, 320, 147)
    assert y.shape[-1] == int(np.ceil(147 * 48000 / 320))
    tt = torch.arange(y.shape[-1], dtype=torch.float64) * 320 / 147 / 48000
    assert float((y[0, 200:-200] - torch.sin(2 * np.pi * 1000 * tt)[200:-200]).abs().max()) < 2e-3
    assert resample_batch(torch.zeros(2, 100000), torch.tensor([44100, 44100]), 22050, 40000).shape == (2, 40000)
    assert resample_batch(torch.zeros(1, 100000), 48000, 44100, 50000).shape == (1, 50000)
    sig = 0.5 * torch.sin(2 * np.pi * 440 * torch.arange(2205) / 22050)
    fn = write_audio_file(sig.reshape(1, -1), 22050, "tone", path=str(tmp_path))
    back, sr = read_wav(fn)
    assert sr == 22050 and back.shape == (1, 2205) and float((back[0] - sig).abs().max()) < 1.0 / 32767
    loud = write_audio_file(4.0 * sig.reshape(1, -1), 22050, "loud", path=str(tmp_path))      # max >= 1 -> rescaled to peak 1
    assert abs(float(read_wav(loud)[0].max()) - 32767 / 32768) < 1e-4


def test_graft_entry_build_checks_the_header_abi_version():
    """__graft_entry__.build() is what the driver runs: it must compile, load the library and agree with the header's ABI version."""
    import __graft_entry__ as g
    g.build()


def test_a_weighting_taps_match_the_reference_filter():
    """training.a_weighting_taps restates FIRFilter("aw") (utils/training_utils.py:94-120); golden from the imported reference (make_golden.py --only aweighting)."""
    from audio_inpainting_diffusion_amd.training import a_weighting_taps
    z = np.load(os.path.join(GOLDEN, "aweighting.npz"))
    for fs in (22050, 44100, 16000):
        t = a_weighting_taps(fs, 101)
        assert t.dtype == np.float32 and np.allclose(t, z[f"taps{fs}"], rtol=0, atol=1e-7)
        y = torch.nn.functional.conv1d(torch.from_numpy(z["x"]).unsqueeze(1), torch.from_numpy(t).view(1, 1, -1), padding=50).squeeze(1)
        assert rel_l2(y, z[f"y{fs}"]) < 1e-6
    with pytest.raises(ValueError):
        a_weighting_taps(22050, 100)


def test_edm_scalar_normalisation_of_the_fused_entry_points():
    """numpy.float32 / int / 0-d / 1-element values are host scalars, device vectors need B elements, anything else is refused
    before it can reach a kernel as a pointer."""
    from audio_inpainting_diffusion_amd._lib import AidError
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention as U
    dev = torch.device("cpu")
    out = U._norm_scalars(3, dev, (np.float32(0.5), 1, torch.tensor(0.25), torch.tensor([2.0])))
    assert out == (0.5, 1.0, 0.25, 2.0) and all(isinstance(v, float) for v in out)
    out = U._norm_scalars(2, dev, (torch.tensor([1.0, 2.0]), torch.tensor([[3.0], [4.0]]), torch.tensor([5.0, 6.0], dtype=torch.float64), 7.0))
    assert all(torch.is_tensor(v) and v.dtype == torch.float32 and v.shape == (2,) for v in out) and out[3].tolist() == [7.0, 7.0] and out[1].tolist() == [3.0, 4.0]
    with pytest.raises(AidError):
        U._norm_scalars(3, dev, (torch.zeros(2), 1.0, 1.0, 1.0))
    with pytest.raises(AidError):
        U._norm_scalars(3, dev, ("0.5", 1.0, 1.0, 1.0))


def test_cpu_thread_placements_and_numa_binding_are_well_formed():
    """bench.cpu_thread_configs (the placements the CPU baseline sweeps) and dist.bind_rank_to_gpu_numa (per-rank CPU shares): disjoint, non-empty
    shares of the cores this process may use; without a GPU / sysfs entry the split is even."""
    import bench
    from audio_inpainting_diffusion_amd import dist as D
    avail = sorted(os.sched_getaffinity(0))
    cfgs = bench.cpu_thread_configs()
    assert 1 <= len(cfgs) <= 3 and all(cpus and set(cpus) <= set(avail) for _, cpus in cfgs)
    assert len({tuple(c) for _, c in cfgs}) == len(cfgs) and len(cfgs[0][1]) <= len(cfgs[-1][1])
    assert D._cpulist("0-3,8,10-11\n") == [0, 1, 2, 3, 8, 10, 11]
    threads0 = torch.get_num_threads()
    try:
        shares = []
        for r in range(2):
            n = D.bind_rank_to_gpu_numa(r, 2)
            shares.append(sorted(os.sched_getaffinity(0)))
            os.sched_setaffinity(0, avail)
            assert n == len(shares[-1]) >= 1
        assert not (set(shares[0]) & set(shares[1])) or len(avail) == 1
        assert set(shares[0]) | set(shares[1]) <= set(avail)
    finally:
        os.sched_setaffinity(0, avail)
        torch.set_num_threads(threads0)


def _c_tables(header):
    """name -> the brace-initialiser table a ``#define`` of csrc/<header> holds, as a float64 array"""
    hdr = open(os.path.join(ROOT, "audio_inpainting_diffusion_amd", "csrc", header)).read()

    def macro(name):
        body = re.search(r"#define %s (\{.*\})" % name, hdr).group(1)
        return np.array(ast.literal_eval(body.replace("{", "[").replace("}", "]").replace("f,", ",").replace("f]", "]")), dtype=np.float64)
    return macro


@pytest.mark.parametrize("gen", ["gen_wino8", "gen_wino45"])
def test_generators_reproduce_the_committed_winograd_headers(gen, tmp_path):
    """tools/gen_wino8.py and tools/gen_wino45.py write csrc/aid_wino8.h and csrc/aid_wino45.h from winograd.cook_toom, the construction the weight
    packs use: run on this tree they give the committed headers byte for byte."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(gen, os.path.join(ROOT, "tools", gen + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = tmp_path / os.path.basename(mod.HEADER)
    mod.main(str(out))
    assert out.read_bytes() == open(mod.HEADER, "rb").read()


def test_f45xf43_matrices_header_and_python_twin_agree():
    """csrc/aid_wino45.h and _lib.wino45_matrices(): each axis reproduces its correlation in fp64; the header's G tables are the doubles themselves
    (%.17g round-trips) and its B^T / A^T tables are the matrices rounded to float32 (%.9g round-trips)."""
    from audio_inpainting_diffusion_amd import _lib
    AFT, GF, BFT, ATT, GT, BTT = _lib.wino45_matrices()
    rng = np.random.default_rng(5)
    for AT, G, BT, m, r in ((AFT, GF, BFT, 4, 5), (ATT, GT, BTT, 4, 3)):
        assert AT.shape == (m, m + r - 1) and G.shape == (m + r - 1, r) and BT.shape == (m + r - 1, m + r - 1)
        d, w = rng.standard_normal(m + r - 1), rng.standard_normal(r)
        ref = np.array([sum(w[k] * d[o + k] for k in range(r)) for o in range(m)])
        assert np.abs(AT @ ((G @ w) * (BT @ d)) - ref).max() < 1e-10
    macro = _c_tables("aid_wino45.h")
    assert np.array_equal(macro("AID_W45_GF"), GF) and np.array_equal(macro("AID_W45_GT"), GT)
    for name, M in (("AID_W45_BTF", BFT), ("AID_W45_BTT", BTT), ("AID_W45_ATF", AFT), ("AID_W45_ATT", ATT)):
        assert np.array_equal(macro(name).astype(np.float32), M.astype(np.float32)), name


def test_pack_forms_are_the_builders_forms_and_the_f43_pack_is_its_g():
    """_lib.PACK_FORMS and network._FORMS speak of the same forms with the same number of planes; the F(4,3) pack, which applies its G row by row with
    one division each as the device kernel does, is the product with the explicit _G43 up to the float32 rounding of the stored value."""
    from audio_inpainting_diffusion_amd import _lib, network
    assert set(network._FORMS) == set(_lib.PACK_FORMS)
    for f, fm in network._FORMS.items():
        assert (fm.taps or 5 * 3) == _lib.pack_planes(f), f
    w = torch.randn(3, 7, 5, 3, generator=torch.Generator().manual_seed(43), dtype=torch.float64)
    cip, cop = _lib.pack_dims(7, 3)
    U = _lib.pack_conv_weight_form(w, 4)
    ref = torch.einsum("xk,oihk->xhio", _lib._G43, w).reshape(30, 7, 3)
    assert U.shape == (30, cip, cop) and U.dtype == torch.float32 and not U[:, 7:].any() and not U[:, :, 3:].any()
    assert bool(((U[:, :7, :3].double() - ref).abs() <= 2.0 ** -24 * ref.abs() + 1e-15).all())


def test_f83_matrices_header_and_python_twin_agree():
    """csrc/aid_wino8.h (generated by tools/gen_wino8.py, compiled into the kernels) and _lib.wino8_matrices() (weight packs, tests) describe the same
    F(8,3): y = A^T [(G w) * (B^T d)] reproduces the 3-tap correlation of 10 samples exactly in fp64, the header's fp32 constants are the rounded
    matrices, and the +-a rows have the even / odd structure the kernels' transforms rely on."""
    from audio_inpainting_diffusion_amd import _lib
    AT, G, BT = _lib.wino8_matrices()
    rng = np.random.default_rng(3)
    for _ in range(4):
        d, w = rng.standard_normal(10), rng.standard_normal(3)
        y = AT @ ((G @ w) * (BT @ d))
        ref = np.array([sum(w[k] * d[o + k] for k in range(3)) for o in range(8)])
        assert np.abs(y - ref).max() < 1e-10
    sg = np.array([(-1.0) ** k for k in range(10)])
    for j in range(4):
        assert np.abs(BT[2 + 2 * j] - sg * BT[1 + 2 * j]).max() < 1e-12 and BT[1 + 2 * j][0] == 0 and BT[1 + 2 * j][9] == 0
    macro = _c_tables("aid_wino8.h")
    assert np.abs(macro("AID_W8_G") - G).max() < 1e-12
    assert np.abs(macro("AID_W8_BT0") - BT[0][0::2]).max() < 1e-7
    assert np.abs(macro("AID_W8_BTE") - np.stack([BT[1 + 2 * j][2::2] for j in range(4)])).max() < 1e-7
    assert np.abs(macro("AID_W8_BTO") - np.stack([BT[1 + 2 * j][1:9:2] for j in range(4)])).max() < 1e-7
    at = macro("AID_W8_AT")
    assert np.abs(at - np.stack([AT[:, 1 + 2 * j] for j in range(4)])).max() < 1e-4 * np.abs(at).max() and at.shape == (4, 8)


def test_winograd_form_choice_is_a_function_of_the_launch_shape():
    """aid_conv2d_wino_form / aid_conv2d_wino8_supported (pure host functions of the library): a batch of one takes F(8,3) -- the K-group instances --
    on the levels whose launch is at most one 512-position tile per CU and keeps F(4,3) on the 96-channel levels (384 tiles) and the deepest one (112),
    sub-batches of four take F(8,3) wherever its 512-position tiles quantise, six rows per residue class have no F(8,3) tile, and the answer never
    depends on anything but the launch shape."""
    from audio_inpainting_diffusion_amd import _lib
    L = _lib.lib()
    levels = [(64, 64, 2048, 2), (96, 128, 1024, 3), (96, 192, 512, 4), (128, 256, 256, 5), (128, 320, 128, 6), (256, 384, 64, 7), (256, 448, 32, 7)]
    for C, F, T, nd in levels:
        for k in range(nd):
            f1 = L.aid_conv2d_wino_form(1, C, C, F, T, 1 << k)
            tiles8 = (C // 64) * F * T // 512
            assert f1 == (8 if (C != 96 and 128 < tiles8 <= 256 and L.aid_conv2d_wino8_supported(C, C, F, T, 1 << k)) else 4), (C, F, T, k, f1)
            f4 = L.aid_conv2d_wino_form(4, C, C, F, T, 1 << k)
            assert f4 in (4, 8) and f4 == L.aid_conv2d_wino_form(4, C, C, F, T, 1 << k)
            if f4 == 8:
                assert L.aid_conv2d_wino8_supported(C, C, F, T, 1 << k)
    assert L.aid_conv2d_wino_form(4, 256, 256, 384, 64, 1) == 8 and L.aid_conv2d_wino_form(4, 256, 256, 448, 32, 4) == 8 and L.aid_conv2d_wino_form(4, 64, 64, 64, 2048, 2) == 8
    assert L.aid_conv2d_wino_form(4, 128, 128, 320, 128, 1) == 4                      # 640 tiles of 512 positions = 2.5 per CU: F(4,3) quantises no worse
    assert not L.aid_conv2d_wino8_supported(256, 256, 384, 64, 64) and L.aid_conv2d_wino_form(8, 256, 256, 384, 64, 64) == 4     # 6 rows per class
    assert not L.aid_conv2d_wino8_supported(256, 256, 64, 16, 1) and L.aid_conv2d_wino_form(8, 256, 256, 64, 16, 1) == 4         # T = 16: F(4,3) tiles only
    assert L.aid_conv2d_wino_form(8, 2, 64, 64, 1024, 1) == 0 and L.aid_conv2d_wino_form(8, 64, 2, 64, 1024, 1) == 0              # few-channel layers: no Winograd input
    # fin_mode (the last tile of a sample folds the epilogue partials) is honoured by the row-shared kernels only
    assert L.aid_conv2d_fin_supported(4, 128, 128, 256, 256, 2, 2) == 1 and L.aid_conv2d_fin_supported(4, 128, 128, 256, 256, 2, 1) == 1
    assert L.aid_conv2d_fin_supported(2, 96, 96, 20, 256, 4, 1) == 0          # 5 rows per class: the row-shared kernel declines, the 96 x 512 tiles take the launch
    assert L.aid_conv2d_fin_supported(8, 256, 256, 384, 64, 64, 2) == 0       # no F(8,3) tile for 6 rows per class
    assert L.aid_conv2d_fin_supported(4, 128, 128, 256, 256, 2, 0) == 0 and L.aid_conv2d_fin_supported(4, 2, 64, 64, 1024, 1, 1) == 0


def _wino_r_host_grid():
    import json
    with open(os.path.join(GOLDEN, "wino_r_host_grid.json")) as f:
        return json.load(f)


def test_row_shared_winograd_host_queries_answer_as_recorded():
    """The seven host queries of the row-shared Winograd kernels (form, F(8,3) support, Winograd-input support, fin_mode support, split-K scratch,
    statistics and dot partials) over the recorded grid of launch shapes -- the seven levels at every dilation and batch 1, 2, 3, 4, 8, T = 16 ... 96,
    F not a multiple of the dilation, few-channel and 96 / 192-channel layers, the shapes the kernels decline: every answer equals the one recorded
    from the library of the commit the fixture names (tools/wino_r_host_grid.py), before the queries read one tile plan (csrc/aid_wino_plan.h)."""
    from audio_inpainting_diffusion_amd import _lib
    L = _lib.lib()
    grid = _wino_r_host_grid()
    assert len(grid["commit"]) == 40 and len(grid["rows"]) == 1320
    for rec in grid["rows"]:
        s = rec[:6]
        got = s + [L.aid_conv2d_wino_form(*s), L.aid_conv2d_wino8_supported(*s[1:]), L.aid_conv2d_wino_input_ok(*s), L.aid_conv2d_wino_split_ws_bytes(*s),
                   [L.aid_conv2d_fin_supported(*s, x) for x in (0, 1, 2)], [L.aid_conv2d_stat_partials(*s, x) for x in (0, 1, 2)],
                   [L.aid_conv2d_dot_partials(*s, x) for x in (0, 1, 2)]]
        assert got == rec, (dict(zip(grid["columns"], rec)), got)


def test_tile_plan_header_runs_clean_under_sanitizers_and_counts_what_the_library_counts(tmp_path):
    """csrc/aid_wino_plan.h is plain host C++: a stand-alone program built with -fsanitize=address,undefined walks the recorded grid and extreme shapes
    (B = 4096, F = 2^20, dilation 2^10, T = 2^16) for both forms and exits clean; the plan's partial slots per sample are aid_conv2d_stat_partials of the
    library, and its tile count is B * (dilF / NC) * quads * ttiles * Cout tiles summed over the families, in unbounded integers."""
    import shutil
    import subprocess
    from audio_inpainting_diffusion_amd import _lib
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    L = _lib.lib()
    rows = [tuple(r[:6]) for r in _wino_r_host_grid()["rows"]]
    extreme = [(4096, 64, c, 1 << 20, 1 << 16, d) for c in (64, 96, 256) for d in (1, 1 << 10)] + [(4096, 64, 64, (1 << 20) + 1, 1 << 16, 1 << 10), (1, 64, 96, 7, 16, 1)]
    shapes = [(B, _lib.pack_dims(ci, co)[1], F, T, d) for B, ci, co, F, T, d in rows + extreme]
    src = tmp_path / "plan.cpp"
    src.write_text('#include <stdio.h>\n#include "aid_wino_plan.h"\nstatic const int S[][5] = {\n' + "".join("    {%d, %d, %d, %d, %d},\n" % s for s in shapes) + '''};
int main() {
    for (const auto& s : S)
        for (int form = 4; form <= 8; form += 4) {
            const WinoRPlan p = wino_r_plan(form, s[0], s[1], s[2], s[3], s[4]);
            printf("%d", p.nl);
            for (int l = 0; l < 2; ++l) printf(" %d %d %d %d %lld", p.f[l].TT, p.f[l].NC, p.f[l].quads, p.f[l].ttiles, (long long)p.f[l].ntiles);
            printf(" %d %lld\\n", p.slots, (long long)p.tiles);
        }
    return 0;
}
''')
    exe = tmp_path / "plan"
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "audio_inpainting_diffusion_amd", "csrc"), str(src), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-2000:]
    out = [[int(v) for v in line.split()] for line in run.stdout.splitlines()]
    assert len(out) == 2 * len(shapes)
    checked = 0
    for i, (B, cop, F, T, d) in enumerate(shapes):
        for j, form in enumerate((4, 8)):
            nl, fam, slots, tiles = out[2 * i + j][0], [out[2 * i + j][1:6], out[2 * i + j][6:11]], out[2 * i + j][11], out[2 * i + j][12]
            ny = cop // (96 if nl == 2 else 64)
            per_family = [B * (d // NC) * quads * ttiles * ny for TT, NC, quads, ttiles, _ in fam[:nl]]
            assert [f[4] for f in fam[:nl]] == per_family and tiles == sum(per_family), (form, B, cop, F, T, d, out[2 * i + j])
            assert fam[nl:] == [[0] * 5] * (2 - nl) and (nl > 0 or slots == 0)
            assert slots == sum((d // NC) * quads * ttiles for TT, NC, quads, ttiles, _ in fam[:nl]) < 2 ** 31
            if i < len(rows) and rows[i][1] == 64 and rows[i][2] in (64, 96, 128, 256):
                assert slots == L.aid_conv2d_stat_partials(*rows[i], 1 if form == 4 else 2), (form, rows[i], slots)
                checked += 1
    assert checked >= 100
    assert out[2 * len(rows)][0] == 1 and out[2 * len(rows)][12] == 4096 * (2 ** 20 // 4) * 1024 > 2 ** 31      # F(4,3), 64 channels, dilation 1: TT = 64, RA = 4


def _conv1x1_host_grid():
    import json
    with open(os.path.join(GOLDEN, "conv1x1_host_grid.json")) as f:
        return json.load(f)


def _cin1s(cin):
    return (16, 64, cin // 2, cin - 16, cin, 24)


def test_conv1x1_host_queries_answer_as_recorded():
    """aid_conv2d_pack_dims, aid_conv2d_dot_partials_1x1 and aid_conv2d_x2_supported over the recorded grid -- the network's own 1x1 layers (channels C, 2C, 8, 2
    at each level's F), Cin in 16 ... 512 x Cout in 32 ... 288 x F in 1 ... 2048, each at T = 8 ... 2048, x2 with six Cin1 per shape: every answer equals the one
    recorded from the library of the commit the fixture names (tools/conv1x1_host_grid.py), before the queries read one plan (csrc/aid_conv1x1_plan.h)."""
    from audio_inpainting_diffusion_amd import _lib
    L = _lib.lib()
    grid = _conv1x1_host_grid()
    B, TS = grid["B"], grid["TS"]
    assert len(grid["commit"]) == 40 and len(grid["rows"]) == 1144 and len(TS) == 12
    for rec in grid["rows"]:
        cin, cout, F = rec[:3]
        got = [cin, cout, F, *_lib.pack_dims(cin, cout), [L.aid_conv2d_dot_partials_1x1(B, cin, cout, F, T) for T in TS],
               [sum(L.aid_conv2d_x2_supported(cin, c1, cout, F, T) << i for i, c1 in enumerate(_cin1s(cin))) for T in TS]]
        assert got == rec, (dict(zip(grid["columns"], rec)), got)


def test_conv1x1_plan_header_runs_clean_under_sanitizers_and_answers_what_the_library_answers(tmp_path):
    """csrc/aid_conv1x1_plan.h is plain host C++: a stand-alone program built with -fsanitize=address,undefined walks the recorded grid and extreme shapes
    (B = 4096, F = 2^20, T = 2^16, Cin = 2^20; every option set; scratch of 0, 2^20 and 2^62 bytes) through the whole chain and exits clean; its partial
    slots and x2 verdicts are the library's aid_conv2d_dot_partials_1x1 / aid_conv2d_x2_supported, and the counts it plans with fit the kernels' ints."""
    import shutil
    import subprocess
    from audio_inpainting_diffusion_amd import _lib
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    L = _lib.lib()
    grid = _conv1x1_host_grid()
    shapes = [(grid["B"], r[0], r[1], r[2], T) for r in grid["rows"] for T in grid["TS"] if T in (8, 16, 48, 256, 2048)]
    n_grid = len(shapes)
    shapes += [(B, ci, co, F, T) for B in (1, 4096, 2 ** 31 - 1) for ci in (64, 256, 1 << 20) for co in (64, 96, 128, 1 << 20) for F in (1, 9, 1 << 20, 2 ** 31 - 1)
               for T in (8, 1 << 16, 2 ** 31 - 1)]
    src = tmp_path / "plan.cpp"
    src.write_text('#include <stdio.h>\n#include "aid_conv1x1_plan.h"\nstatic const int S[][6] = {\n' +
                   "".join("    {%d, %d, %d, %d, %d, %d},\n" % (s + (_lib.pack_dims(s[1], s[2])[1],)) for s in shapes) + '''};
int main() {
    for (const auto& v : S) {
        C11Shape s = {};
        s.B = v[0]; s.Cin = v[1]; s.Cout = v[2]; s.F = v[3]; s.T = v[4]; s.Cout_pad = v[5];
        C11Shape q = s;
        q.epi = 1; q.dot = true;
        printf("%d", c11_plan(q).slots);
        const int c1[6] = {16, 64, s.Cin / 2, s.Cin - 16, s.Cin, 24};
        for (int i = 0; i < 6; ++i) {
            C11Shape x = s;
            x.B = 1; x.x2 = true; x.Cin1 = c1[i];
            printf(" %d", c11_dma_plan(x).family ? 1 : 0);
        }
        long long worst = 0;                                   // the largest count any option set plans with
        for (int o = 0; o < 128; ++o)
            for (int w = 0; w < 3; ++w) {
                C11Shape t = s;
                t.act = o & 1; t.in_scale = o & 2; t.epi = (o >> 2) & 1; t.res = o & 8; t.x2 = o & 16; t.dot = o & 32; t.ws = w > 0;
                t.Cin1 = (o & 64) ? 16 : s.Cin / 2;
                t.ws_bytes = w == 1 ? (1LL << 20) : (w == 2 ? (1LL << 62) : 0);
                const C11Plan pl = c11_plan(t);
                if (!pl.ok) continue;
                const long long c[] = {pl.nrows, pl.nx, (long long)pl.nx * pl.ny + 7, pl.ntiles, pl.ntiles ? pl.ntiles + 2048LL : 0, pl.pblocks * pl.mchunks, pl.slots, pl.S, pl.gx};
                for (long long k : c) worst = k > worst ? k : worst;
                if (pl.family == C11_STREAM && pl.npos != (long long)t.B * t.F * t.T) return 2;
                if (pl.S > 1 && !c11_splitk_fits(pl.S, t.B, t.Cout, t.F, t.T, t.ws_bytes)) return 3;
            }
        printf(" %lld\\n", worst);
    }
    return 0;
}
''')
    exe = tmp_path / "plan"
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "audio_inpainting_diffusion_amd", "csrc"), str(src), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, (run.returncode, run.stderr[-2000:])
    out = [[int(v) for v in line.split()] for line in run.stdout.splitlines()]
    assert len(out) == len(shapes)
    nonzero = 0
    for (B, cin, cout, F, T), o in zip(shapes, out):
        assert o[0] == L.aid_conv2d_dot_partials_1x1(B, cin, cout, F, T), (B, cin, cout, F, T, o)
        assert o[1:7] == [L.aid_conv2d_x2_supported(cin, c1, cout, F, T) for c1 in _cin1s(cin)], (B, cin, cout, F, T, o)
        assert 0 <= o[7] <= 2 ** 31 - 1, (B, cin, cout, F, T, o)
        nonzero += o[0] > 0
    assert nonzero >= 1000 and any(o[0] > 0 for o in out[n_grid:]) and any(o[0] == 0 for o in out[n_grid:])


def test_conv1x1_plan_names_the_kernel_that_the_dispatch_recording_names(tmp_path):
    """c11_plan (the chain rs, dma, stream, tiled on scalars, which the host queries read) and aid_conv2d's dispatch (the same chain through the *_try
    functions) state the order twice: for every case of tests/golden/conv1x1_dispatch.json the family and K split of c11_plan, from a stand-alone program
    over the header, name the kernel that the recording (aid_last_kernel after aid_conv2d on an MI355X) names."""
    import json
    import shutil
    import subprocess
    from audio_inpainting_diffusion_amd import _lib
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    with open(os.path.join(GOLDEN, "conv1x1_dispatch.json")) as f:
        cases = json.load(f)["cases"]
    assert len(cases) >= 61
    src = tmp_path / "family.cpp"
    src.write_text('#include <stdio.h>\n#include "aid_conv1x1_plan.h"\nstatic const int S[][13] = {\n' +
                   "".join("    {%s},\n" % ", ".join(str(v) for v in c[:12] + [_lib.pack_dims(c[1], c[2])[1]]) for c in cases) + '''};
int main() {
    for (const auto& v : S) {
        C11Shape s = {};
        s.B = v[0]; s.Cin = v[1]; s.Cout = v[2]; s.F = v[3]; s.T = v[4]; s.act = v[5]; s.in_scale = v[6]; s.epi = v[7]; s.res = v[8]; s.dot = v[9];
        s.Cin1 = v[10]; s.x2 = v[10] > 0; s.ws = v[11]; s.ws_bytes = v[11] ? 4LL * 8 * v[0] * v[2] * v[3] * v[4] : 0; s.Cout_pad = v[12];
        const C11Plan pl = c11_plan(s);
        printf("%d %d %d\\n", pl.ok ? pl.family : -1, pl.S, pl.slots);
    }
    return 0;
}
''')
    exe = tmp_path / "family"
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "audio_inpainting_diffusion_amd", "csrc"), str(src), "-o", str(exe)])
    out = [[int(v) for v in line.split()] for line in subprocess.check_output([str(exe)], text=True).splitlines()]
    names = {1: "conv11_rs_kernel", 2: "conv11_dma_kernel", 3: "gemm_skinny_kernel+splitk", 4: "conv11_dma_kernel+splitk", 5: "conv1x1_stream_kernel"}
    assert len(out) == len(cases)
    for c, (family, S, slots) in zip(cases, out):
        want = names[family] if family else ("conv_mfma_kernel+splitk" if S > 1 else "conv_mfma_kernel(1x1)")
        assert want == c[12], (c, family, S)
        assert (slots > 0) == bool(c[9]) and (not c[9] or slots == _lib.lib().aid_conv2d_dot_partials_1x1(*c[:5])), (c, slots)
    assert {c[12] for c in cases} == set(names.values()) | {"conv_mfma_kernel+splitk", "conv_mfma_kernel(1x1)"}


def test_two_dimensional_winograd_choice_is_a_function_of_the_launch_shape():
    """aid_conv2d_wino2d_supported / _wanted / _positions (pure host functions): K = 256 levels always (padding up to 4/3), K = 128 levels with T <= 256 up to
    1.2 padding (longer rows only for launches of at most two samples), nothing below 128 channels; positions = B * ceil(F / (4 dil)) * dil * T / 4."""
    from audio_inpainting_diffusion_amd import _lib
    L = _lib.lib()
    for B in (1, 2, 4, 8):
        for d in (1, 2, 4, 8, 16, 32, 64):
            assert L.aid_conv2d_wino2d_wanted(B, 256, 256, 448, 32, d) == 1 and L.aid_conv2d_wino2d_wanted(B, 256, 256, 384, 64, d) == 1
        for d in (1, 2, 4, 8, 16, 32):
            assert L.aid_conv2d_wino2d_wanted(B, 128, 128, 320, 128, d) == 1                 # (d = 32: 10 rows per class -> 12, padding 1.2)
        assert L.aid_conv2d_wino2d_wanted(B, 128, 128, 384, 64, 64) == 0                    # 6 rows per class -> 8: 1.33 does not pay at K = 128
        assert L.aid_conv2d_wino2d_wanted(B, 128, 128, 256, 256, 2) == 1 and L.aid_conv2d_wino2d_wanted(B, 128, 128, 128, 512, 2) == (1 if B <= 2 else 0)
        assert L.aid_conv2d_wino2d_wanted(B, 96, 96, 192, 512, 2) == 1 and L.aid_conv2d_wino2d_wanted(B, 96, 96, 64, 2048, 1) == 0 and L.aid_conv2d_wino2d_wanted(B, 64, 64, 64, 2048, 1) == 0
        assert L.aid_conv2d_wino2d_wanted(B, 128, 128, 320, 128, 4) == L.aid_conv2d_wino2d_wanted(B, 128, 128, 320, 128, 4)
        assert L.aid_conv2d_wino2d_positions(B, 448, 32, 64) == B * 2 * 64 * 8 and L.aid_conv2d_wino2d_positions(B, 384, 64, 1) == B * 96 * 16
    assert L.aid_conv2d_wino2d_supported(256, 256, 448, 32, 1) == 1 and L.aid_conv2d_wino2d_supported(128, 128, 256, 256, 16) == 1
    assert L.aid_conv2d_wino2d_supported(96, 96, 192, 512, 2) == 1 and L.aid_conv2d_wino2d_supported(64, 64, 64, 2048, 1) == 0 and L.aid_conv2d_wino2d_supported(256, 256, 448, 24, 1) == 0      # Cout % 128 or % 96, T % 16
    assert L.aid_conv2d_wino2d_supported(256, 256, 450, 32, 4) == 0 and L.aid_conv2d_wino2d_supported(128, 128, 64, 4096, 1) == 0    # F % dil, T <= 2048


def test_failed_launch_re_zeroes_the_scratch_that_must_be_found_zero():
    """Plan._fail: arrival counters / split-K flags have the contract "zero before a launch, left zero by it"; a launch that fails must not leave them
    half-way for the next run."""
    import ctypes as C
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.plan import Op, Plan
    pl = Plan()
    cnt = torch.ones(4, dtype=torch.int32)
    flags = torch.ones(4096, dtype=torch.float32)
    pl.zero_on_fail.extend([cnt, flags])
    holder = C.c_int(0)
    pl.ops.append(Op(lambda addr, stream: 2, C.addressof(holder), "aid_conv2d", 0, 0, "fake", 0, [], [], holder))
    pl.run = Plan.run.__get__(pl)
    with pytest.raises(_lib.AidError, match="aid_conv2d failed rc=2"):
        pl._fail(pl.ops[0], 2)
    assert int(cnt.abs().sum()) == 0 and float(flags[:1024].abs().sum()) == 0.0 and float(flags[1024:].sum()) == 3072.0
    # the flag region's size is the header's constant, not a literal of plan.py
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aid_kernels.h")).read()
    assert int(re.search(r"#define AID_CONV2D_SPLIT_FLAG_BYTES (\d+)", hdr).group(1)) == _lib.AID_CONV2D_SPLIT_FLAG_BYTES == 4096
    # a run ABANDONED half-way for any other reason (an exception between launches) marks the plan dirty: the next run re-zeroes before its first launch
    pl2 = Plan()
    cnt2 = torch.zeros(4, dtype=torch.int32)
    pl2.zero_on_fail.append(cnt2)
    seen = []

    def first(addr, stream):
        cnt2.fill_(7)                                     # "a kernel left its counter half-way"
        return 0

    def boom(addr, stream):
        raise KeyboardInterrupt
    pl2.ops.append(Op(first, C.addressof(holder), "aid_add2", 0, 0, "fake", 0, [], [], holder))
    pl2.ops.append(Op(boom, C.addressof(holder), "aid_add2", 0, 0, "fake", 0, [], [], holder))
    import unittest.mock as mock
    with mock.patch("torch.cuda.current_stream", lambda: type("S", (), {"cuda_stream": 0})()), mock.patch("torch.cuda.synchronize", lambda: None):
        with pytest.raises(KeyboardInterrupt):
            pl2.run()
        assert pl2._dirty and int(cnt2.sum()) == 28
        pl2.ops[0] = Op(lambda addr, stream: seen.append(int(cnt2.sum())) or 0, C.addressof(holder), "aid_add2", 0, 0, "fake", 0, [], [], holder)
        pl2.ops.pop()
        pl2.run()
    assert seen == [0] and not pl2._dirty                 # zeroed BEFORE the first launch of the next run


def test_bench_reports_pmc_traffic_only_for_the_same_build_and_names_kernels_as_rocprof_does():
    """bench.py: roofline.traffic comes from a committed PMC profile ONLY when that profile was taken on the same kernel sources (no stale
    numbers); the per-kernel tables aggregate by the device kernel's name as rocprofv3 lists it; executed-FLOP fractions per Winograd form."""
    import bench
    assert bench.kernel_base("w2d_gemm_kernel<128x256,kc16,nb3>") == "w2d_gemm_kernel" and bench.kernel_base("conv53_wino8r_kernel(64+32)") == "conv53_wino8r_kernel"
    assert bench.kernel_base("conv11_dma_kernel+splitk") == "conv11_dma_kernel" and bench.kernel_base("w2d_gemm_s6_kernel<128x128,nb3,wpc3>") == "w2d_gemm_s6_kernel"
    assert bench.WINO_EXEC["w2d_gemm_kernel"] == 0.2 and abs(bench.WINO_EXEC["conv53_wino8r_kernel"] - 5 / 12) < 1e-12 and bench.WINO_EXEC["conv53_wino4r_kernel"] == 0.5
    f = bench._traffic_fields("conv53_wino8r_kernel", {"algorithmic_mb_per_launch": 500.0})
    tp = f["traffic_from_profile"]
    if tp is None:
        assert f["traffic"] is None and f["traffic_over_algorithmic"] is None
    else:
        same = tp.get("kernel_sources_sha16") == bench._kernel_sources_sha16()
        assert tp["used"] == same and (f["traffic"] is None or same) and (f["traffic_source"] is None) == (not same)
    assert len(bench._kernel_sources_sha16()) == 16


def test_bench_dump_outputs_writes_float32_and_a_fixed_sample_within_the_budget(tmp_path, monkeypatch):
    """bench.py --dump-outputs: an array within the budget is written whole in float32; one over it keeps a fixed seeded sample of its rows (the same
    rows on every run, their indices beside it), and the files stay within DUMP_MAX_BYTES."""
    import bench
    g0 = torch.Generator().manual_seed(3)
    x = torch.randn(8, 1000, generator=g0, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "a"), {"x": x})
    v = np.load(tmp_path / "a" / "x.npy")
    assert v.dtype == np.float32 and np.array_equal(v, x.float().numpy()) and not (tmp_path / "a" / "x_rows.npy").exists()
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2 ** 16 + 5 * 4000 + 100)         # room for five rows of 1000 float32
    big = torch.randn(64, 1000, generator=g0)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"x": big})
    rows, v = np.load(tmp_path / "b" / "x_rows.npy"), np.load(tmp_path / "b" / "x.npy")
    assert rows.dtype == np.float64 and len(rows) == 5 and np.all(np.diff(rows) > 0)
    assert np.array_equal(v, big.numpy()[rows.astype(int)])
    assert np.array_equal(rows, np.load(tmp_path / "c" / "x_rows.npy")) and np.array_equal(v, np.load(tmp_path / "c" / "x.npy"))
    assert sum(f.stat().st_size for f in (tmp_path / "b").iterdir()) <= bench.DUMP_MAX_BYTES


def test_lambda_degradation_is_the_jacobian_transpose_product_at_x_hat():
    """sampler.LambdaDegradation (Sampler.predict_resample, edm_sampler_inpainting.py:164-173): apply = the callable on a detached copy, adjoint = its VJP at the
    same point -- what the reference's torch.autograd.grad forms through `degradation(x_hat)` (:65-81) -- for a linear operator that changes the length and for a
    non-linear one; a second adjoint without an apply is refused, a constant degradation has no gradient."""
    from audio_inpainting_diffusion_amd._lib import AidError
    from audio_inpainting_diffusion_amd.sampler import LambdaDegradation
    from degradations import resample_degradations
    g0 = torch.Generator().manual_seed(0)
    x = torch.randn(2, 512, generator=g0)
    for which in (0, 1):
        fn = resample_degradations([0.1, 0.2, 0.4, 0.2, 0.1])[which]
        op = LambdaDegradation(fn)
        den = op.apply(x)
        assert not den.requires_grad and torch.equal(den, fn(x))
        seed = torch.randn(den.shape, generator=g0)
        got = op.adjoint(seed)
        xl = x.clone().requires_grad_()
        (ref,) = torch.autograd.grad(fn(xl), xl, seed)
        assert got.shape == x.shape and torch.allclose(got, ref, rtol=0, atol=1e-7)
        with pytest.raises(AidError):
            op.adjoint(seed)
    op = LambdaDegradation(lambda v: torch.zeros_like(v))
    op.apply(x)
    with pytest.raises(RuntimeError):
        op.adjoint(torch.ones(2, 512))
    with pytest.raises(AttributeError):
        op.project(x, x)


def test_sampler_and_edm_expose_the_reference_classes_method_names():
    """Every method of testing/edm_sampler_inpainting.Sampler (:8-364) and diff_params/edm.EDM (:7-193) exists under the same name with the same
    positional parameters (the names are the reference's API, listed here; the mirrors' behaviour is pinned by the golden / GPU tests)."""
    import inspect
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.sampler import Sampler
    sampler_api = {"__init__": ["model", "diff_params", "args", "rid"], "update_diff_params": [], "get_score_rec_guidance": ["x", "y", "t_i", "degradation"],
                   "get_score": ["x", "y", "t_i", "degradation"], "predict_unconditional": ["shape", "device"], "predict_resample": ["y", "shape", "degradation"],
                   "predict": ["shape", "device"], "apply_mask": ["x", "mask"], "apply_spectral_mask": ["x"], "prepare_smooth_mask": ["mask", "size"],
                   "predict_inpainting": ["y_masked", "mask"], "predict_spectrogram_inpainting": ["y_masked", "mask"]}
    edm_api = {"__init__": ["args"], "get_gamma": ["t"], "create_schedule": ["nb_steps"], "sample_ptrain": ["N"], "sample_ptrain_safe": ["N"],
               "sample_prior": ["shape", "sigma"], "cskip": ["sigma"], "cout": ["sigma"], "cin": ["sigma"], "cnoise": ["sigma"], "lambda_w": ["sigma"],
               "denoiser": ["xn", "net", "sigma"], "prepare_train_preconditioning": ["x", "sigma"], "loss_fn": ["net", "x"]}
    for cls, api in ((Sampler, sampler_api), (EDM, edm_api)):
        for name, params in api.items():
            fn = getattr(cls, name, None)
            assert callable(fn), f"{cls.__name__}.{name} is missing"
            got = [p for p in inspect.signature(fn).parameters if p != "self"]
            assert got[:len(params)] == params, (cls.__name__, name, got)


def test_three_dimensional_observations_take_the_induced_matrix_norm_or_are_rejected():
    """torch.linalg.norm(y - den, dim=(1, 2), ord=2) over 3-D observations (edm_sampler_inpainting.py:67-75) is the SPECTRAL norm, not the
    Frobenius norm of the flattened item.  The oracle keeps the reference's semantics; the HIP sampler (whose guidance seed is element-wise)
    refuses such a call instead of silently computing another norm."""
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.config import small_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.sampler import Sampler
    from oracle.edm import OracleEDM
    from oracle.sampler import OracleSampler
    from test_oracle_golden import _Toy
    L = 2048
    deg = lambda v: v.reshape(v.shape[0], 4, L // 4)[:, :3, ::2]                # noqa: E731  (a linear map onto [B, 3, L/8] observations)
    torch.manual_seed(3)
    y = deg(0.063 * torch.randn(1, L))
    runs = {}
    for norm in (2, "fro"):
        s = OracleSampler(_Toy(L), OracleEDM(), T=2, xi=0.25, data_consistency=False, audio_len=L, norm=norm)
        torch.manual_seed(4)
        runs[norm] = s.predict_resample(y, (1, L), deg)
    assert torch.isfinite(runs[2]).all() and rel_l2(runs[2], runs["fro"]) > 1e-3        # ord = 2 is NOT the flattened (Frobenius) norm
    args = small_args()
    args.tester.posterior_sampling.norm = 2

    class _Fused:                                                                   # (stands for the MI355X network: never evaluated here)
        denoise = denoise_guided = None
    smp = Sampler(model=_Fused(), diff_params=EDM(args), args=args)
    with pytest.raises(_lib.AidError, match="induced matrix norm"):
        smp.predict_resample(y, (1, L), deg)
