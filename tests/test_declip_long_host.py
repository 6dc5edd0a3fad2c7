"""CPU tests (no GPU) of declipping whole recordings (declip_long.py, include/aid_declip.h, Sampler.predict_declipping_long,
harness.declip_long): the plan from a clipped recording against restore_plan over |y| < c, and the
refusals, all raised before anything touches a GPU."""

import numpy as np
import pytest
import torch

from test_restore_long_host import CASES


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
def _clipped(R, N, levels, seed):
    """[R, N] recordings clipped at their levels: sparse peaks above the level over a quiet floor, so that some windows are jobs and some are not"""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(R, N, generator=g) * 0.01
    for r in range(R):
        idx = torch.randint(0, N, (3,), generator=g)
        y[r, idx] = torch.tensor([2.0, -3.0, 1.5])[:idx.numel()] * levels[r]
    c = torch.tensor(levels, dtype=torch.float32)[:, None]
    return torch.maximum(torch.minimum(y, c), -c)


@pytest.mark.parametrize("N,L,end", CASES)
def test_the_plan_of_a_clipped_recording_is_restore_plan_over_the_unclipped_samples(N, L, end):
    from audio_inpainting_diffusion_amd.declip_long import clip_levels, declip_plan
    from audio_inpainting_diffusion_amd.restore import restore_plan, restore_windows
    levels = [0.25, 0.05, 1.0]
    y = _clipped(3, N, levels, 5 + N)
    c = torch.tensor(levels)[:, None]
    got = declip_plan(y, clip_levels(levels, 3), L, end)
    assert got == restore_plan(y.abs() < c, L, end)
    # ... which is: a window is a job exactly when its owned range holds a sample with |y| >= c_r
    want = ([], [])
    for r in range(3):
        for w, (s, head, tail, lo, hi) in enumerate(restore_windows(N, L, end)):
            if bool((y[r, s + lo:s + hi].abs() >= levels[r]).any()):
                want[w % 2].append((r, s, head, tail, lo, hi))
    assert got[:2] == want and want[0]
    assert declip_plan(y[:1], clip_levels(0.25, 1), L, end) == restore_plan(y[:1].abs() < 0.25, L, end)       # one level for all
    # every sample at its level: every window of every recording is a job
    full = c.expand(3, N) * torch.where(torch.arange(N) % 2 == 0, 1.0, -1.0)
    A, B, _ = declip_plan(full, clip_levels(levels, 3), L, end)
    assert len(A) + len(B) == 3 * len(restore_windows(N, L, end))


@pytest.mark.parametrize("N,L,end", CASES)
def test_a_recording_below_its_level_makes_no_job(N, L, end):
    from audio_inpainting_diffusion_amd.declip_long import clip_levels, declip_plan
    y = torch.randn(2, N, generator=torch.Generator().manual_seed(N)).clamp(-3, 3)
    y = y / y.abs().amax(dim=1, keepdim=True) * torch.tensor([[0.25], [0.05]]) * (1 - 2.0 ** -20)             # peaks just below the levels
    assert float(y[0].abs().max()) < 0.25 and float(y[1].abs().max()) < np.float32(0.05)
    assert declip_plan(y, clip_levels([0.25, 0.05], 2), L, end)[:2] == ([], [])
    y[1, N // 2] = float(np.float32(0.05))                                                                    # one sample AT the level: clipped
    A, B, _ = declip_plan(y, clip_levels([0.25, 0.05], 2), L, end)
    assert len(A) + len(B) == 1 and (A + B)[0][0] == 1


def test_clip_levels_round_to_float32_and_refuse_bad_values():
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.declip_long import clip_levels
    c = clip_levels(0.05, 3)
    assert c.dtype == np.float32 and c.tolist() == [float(np.float32(0.05))] * 3
    assert clip_levels(torch.tensor([0.1, 0.2]), 2).tolist() == [float(np.float32(0.1)), float(np.float32(0.2))]
    for bad in (0.0, -0.1, float("nan"), float("inf"), [0.1, 0.0], []):
        with pytest.raises(_lib.AidError, match="finite and > 0"):
            clip_levels(bad, 2)
    with pytest.raises(_lib.AidError, match="clip levels for"):
        clip_levels([0.1, 0.2, 0.3], 2)


# ---- refusals that need no GPU, the harness wrapper --------------------------------------------------------------------------------------
class _Fused:                                                                # (stands for the MI355X network: never evaluated here)
    denoise = denoise_guided = None


def _stub_sampler(rid=False, overlap=0.25):
    from audio_inpainting_diffusion_amd.config import small_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.sampler import Sampler
    args = small_args(xi=0.25)
    args.tester.autoregressive.overlap = overlap
    return Sampler(model=_Fused(), diff_params=EDM(args), args=args, rid=rid), int(args.exp.audio_len)


def test_every_refusal_is_raised_before_any_launch(monkeypatch):
    from audio_inpainting_diffusion_amd import _lib, declip_long
    launched = []
    monkeypatch.setattr(_lib, "call", lambda name, p: launched.append(name))
    monkeypatch.setattr(declip_long, "declip_plan", lambda *a, **k: launched.append("plan"))
    smp, L = _stub_sampler()
    smp.seeds = [5]
    N = 3 * L
    y = torch.zeros(2, N)                                                    # (on the host: a valid call is refused for that, every other one for its own reason)
    with pytest.raises(_lib.AidError, match="GPU only"):
        smp.predict_declipping_long(y, [0.05, 0.03], max_batch=1, seeds=[1, 2])
    with pytest.raises(_lib.AidError, match="GPU only"):
        declip_long.declip_passes(smp, y, 0.05, L, L // 4)
    for bad in (0.0, -0.05, float("nan"), float("inf"), [0.05, 0.0]):
        with pytest.raises(_lib.AidError, match="finite and > 0"):
            smp.predict_declipping_long(y, bad)
    for bad in ([0.05, 0.05, 0.05], []):
        with pytest.raises(_lib.AidError, match="clip level"):
            smp.predict_declipping_long(y, bad)
    for bad in ([1], [1, 2, 3]):
        with pytest.raises(_lib.AidError, match="seeds"):
            smp.predict_declipping_long(y, 0.05, seeds=bad)
    for bad in (0, -2):
        with pytest.raises(_lib.AidError, match="max_batch"):
            smp.predict_declipping_long(y, [0.05, 0.03], max_batch=bad)
    with pytest.raises(_lib.AidError, match="rid"):
        _stub_sampler(rid=True)[0].predict_declipping_long(y, 0.05)
    for ov in (0.5, 0.75, 0.0):
        with pytest.raises(_lib.AidError, match="end"):
            _stub_sampler(overlap=ov)[0].predict_declipping_long(y, 0.05)
    for end in (0, L // 2 + 1, L, -3):
        with pytest.raises(_lib.AidError, match="end"):
            declip_long.declip_passes(smp, y, 0.05, L, end)
    assert launched == [] and smp.seeds == [5] and smp.y is None and smp.spectral is None and smp.n_evals == 0


def test_declip_long_groups_equal_lengths_and_checks_its_arguments():
    from audio_inpainting_diffusion_amd.harness import declip_long

    class Rec:
        def __init__(self):
            self.calls = []

        def predict_declipping_long(self, y, clip_value, max_batch=8, seeds=None):
            self.calls.append((tuple(y.shape), list(clip_value), max_batch, seeds))
            return y + 1

    files = [torch.full((n,), float(k)) for k, n in enumerate((700, 300, 700, 301, 300))]
    rec = Rec()
    out = declip_long(rec, files, [0.1, 0.2, 0.3, 0.4, 0.5], seeds=[10, 11, 12, 13, 14], max_batch=4, device="cpu")
    assert [c[0] for c in rec.calls] == [(2, 700), (2, 300), (1, 301)] and all(c[2] == 4 for c in rec.calls)
    assert [c[1] for c in rec.calls] == [[0.1, 0.3], [0.2, 0.5], [0.4]] and [c[3] for c in rec.calls] == [[10, 12], [11, 14], [13]]
    assert all(torch.equal(o, f + 1) for o, f in zip(out, files))        # full length, in the order of the files
    rec = Rec()
    declip_long(rec, files, 0.25, device="cpu")                          # one level for every file, the global generator
    assert [c[1] for c in rec.calls] == [[0.25, 0.25], [0.25, 0.25], [0.25]] and all(c[3] is None for c in rec.calls)
    with pytest.raises(ValueError):
        declip_long(rec, files, [0.1, 0.2], device="cpu")
    with pytest.raises(ValueError):
        declip_long(rec, files, 0.1, seeds=[1], device="cpu")
