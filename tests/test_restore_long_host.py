"""CPU tests (no GPU) of whole-recording restoration (restore.py, include/aid_restore.h, Sampler.predict_inpainting_long,
harness.restore_long): the window plan against the ownership rule restated here, the refusals (all
raised before anything touches a GPU) and the smoothed mask of a window whose gap touches an end of the window."""
import math

import pytest
import torch


CASES = [(1000, 256, 64), (1001, 256, 1), (2500, 256, 127), (100, 256, 64), (256, 256, 64)]


def expected_windows(N, L, end):
    """The rule, restated: [(s, head, tail, lo, hi)] with [lo, hi) the owned range relative to s, cut at N."""
    step = L - end
    W = max(1, math.ceil((N - L) / step) + 1)
    wins = []
    for w in range(W):
        s = w * step
        if w % 2 == 0:
            a, b, head, tail = s, s + L, 0, 0
        elif w == W - 1:
            a, b, head, tail = s + end, s + L, end, 0
        else:
            a, b, head, tail = s + end, s + L - end, end, end
        wins.append((s, head, tail, a - s, min(b, N) - s))
    return wins


def _masks(N, R):
    """all ones, all zeros, and sparse random gaps (so that some windows are jobs and some are not), [R, N]"""
    g = torch.Generator().manual_seed(N + R)
    out = [torch.ones(R, N), torch.zeros(R, N)]
    for n_zero in (1, 3, 40):
        m = torch.ones(R, N)
        for r in range(R):
            m[r, torch.randint(0, N, (n_zero,), generator=g)] = 0
        out.append(m)
    m = torch.ones(R, N)
    m[:, N - 1] = 0                                         # a gap of one sample at the very end
    out.append(m)
    return out


@pytest.mark.parametrize("N,L,end", CASES)
def test_owned_ranges_partition_the_recording(N, L, end):
    from audio_inpainting_diffusion_amd.restore import restore_plan
    step = L - end
    A, B, N_pad = restore_plan(torch.zeros(1, N), L, end)     # every sample a gap: every window is a job
    W = max(1, math.ceil((N - L) / step) + 1)
    assert N_pad == L + (W - 1) * step and N_pad >= N and len(A) + len(B) == W
    assert len(A) == (W + 1) // 2 and all((s // step) % 2 == 0 and s % step == 0 for _, s, *_ in A) and all((s // step) % 2 == 1 for _, s, *_ in B)
    ranges = sorted((s + lo, s + hi) for _, s, _, _, lo, hi in A + B)
    assert ranges[0][0] == 0 and ranges[-1][1] == N
    assert all(a < b for a, b in ranges)                       # nobody owns an empty range
    assert all(ranges[k][1] == ranges[k + 1][0] for k in range(len(ranges) - 1))
    assert [(s, h, t, lo, hi) for _, s, h, t, lo, hi in sorted(A + B, key=lambda j: j[1])] == expected_windows(N, L, end)
    if N < L:
        assert (A, B, N_pad) == ([(0, 0, 0, 0, 0, N)], [], L)  # one window, hi cut at N
    if W % 2 == 0:                                             # an odd last window owns up to its end: head = end, tail = 0
        r, s, head, tail, lo, hi = B[-1]
        assert (head, tail, lo, hi) == (end, 0, end, min(L, N - s))
    for r, s, head, tail, lo, hi in B[:-1] if W % 2 == 0 else B:
        assert (head, tail, lo, hi) == (end, end, end, L - end)
    for r, s, head, tail, lo, hi in A:
        assert (head, tail, lo) == (0, 0, 0) and hi == min(L, N - s)


@pytest.mark.parametrize("N,L,end", CASES)
@pytest.mark.parametrize("R", [1, 3])
def test_a_window_is_a_job_iff_its_owned_range_holds_a_zero(N, L, end, R):
    from audio_inpainting_diffusion_amd.restore import restore_plan
    wins = expected_windows(N, L, end)
    step = L - end
    for mask in _masks(N, R):
        want_A, want_B = [], []
        for r in range(R):
            for w, (s, head, tail, lo, hi) in enumerate(wins):
                if bool((mask[r, s + lo:s + hi] == 0).any()):
                    (want_B if w % 2 else want_A).append((r, s, head, tail, lo, hi))
        A, B, N_pad = restore_plan(mask, L, end)
        assert (A, B) == (want_A, want_B) and N_pad == L + (len(wins) - 1) * step
        if bool((mask == 1).all()):
            assert A == [] and B == []
        # other dtypes, and one shared row: its jobs repeat for every recording
        assert restore_plan(mask.bool(), L, end)[:2] == (A, B) and restore_plan(mask.double(), L, end)[:2] == (A, B)
        sA, sB, _ = restore_plan(mask[:1], L, end, R=R)
        one_A, one_B, _ = restore_plan(mask[:1], L, end)
        assert sA == [(r,) + j[1:] for r in range(R) for j in one_A] and sB == [(r,) + j[1:] for r in range(R) for j in one_B]
    assert restore_plan(torch.ones(N), L, end)[:2] == ([], [])      # a 1-D mask is one shared row


def test_plan_refuses_an_overlap_outside_its_range():
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.restore import restore_plan
    m = torch.zeros(1, 1000)
    for L, end in ((256, 128), (256, 200), (256, 256), (255, 128), (256, 0), (256, -3)):
        with pytest.raises(_lib.AidError, match="end"):
            restore_plan(m, L, end)
    restore_plan(m, 256, 127), restore_plan(m, 255, 127), restore_plan(m, 256, 1)
    with pytest.raises(_lib.AidError):
        restore_plan(torch.zeros(2, 1000), 256, 64, R=3)
    with pytest.raises(_lib.AidError):
        restore_plan(torch.zeros(2, 3, 1000), 256, 64)


# ---- refusals that need no GPU, the harness wrapper, the smoothed mask of a window -----------------------------------------------------
class _Fused:                                                                # (stands for the MI355X network: never evaluated here)
    denoise = denoise_guided = None


def _stub_sampler(rid=False, overlap=0.25):
    from audio_inpainting_diffusion_amd.config import small_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.sampler import Sampler
    args = small_args(xi=0.25)
    args.tester.autoregressive.overlap = overlap
    return Sampler(model=_Fused(), diff_params=EDM(args), args=args, rid=rid), int(args.exp.audio_len)


def test_predict_inpainting_long_refuses_host_tensors_and_rid():
    from audio_inpainting_diffusion_amd import _lib
    smp, L = _stub_sampler()
    smp.seeds = [5]
    with pytest.raises(_lib.AidError, match="GPU only"):
        smp.predict_inpainting_long(torch.zeros(2, 3 * L), torch.ones(1, 3 * L))
    smp, L = _stub_sampler(rid=True)
    with pytest.raises(_lib.AidError, match="rid"):
        smp.predict_inpainting_long(torch.zeros(2, 3 * L), torch.ones(1, 3 * L))
    assert smp.y is None and smp.mask is None and smp.n_evals == 0


def test_restore_long_groups_equal_lengths_and_checks_its_arguments():
    from audio_inpainting_diffusion_amd.harness import restore_long

    class Rec:
        def __init__(self):
            self.calls = []

        def predict_inpainting_long(self, y, mask, max_batch=8, seeds=None):
            self.calls.append((tuple(y.shape), tuple(mask.shape), max_batch, seeds))
            return y + 1

    files = [torch.full((n,), float(k)) for k, n in enumerate((700, 300, 700, 301, 300))]
    masks = [torch.ones(f.numel()) for f in files]
    rec = Rec()
    out = restore_long(rec, files, masks, seeds=[10, 11, 12, 13, 14], max_batch=4, device="cpu")
    assert [c[0] for c in rec.calls] == [(2, 700), (2, 300), (1, 301)] and all(c[0] == c[1] and c[2] == 4 for c in rec.calls)
    assert [c[3] for c in rec.calls] == [[10, 12], [11, 14], [13]]
    assert all(torch.equal(o, f + 1) for o, f in zip(out, files))        # full length, in the order of the files
    with pytest.raises(ValueError):
        restore_long(rec, files, masks[:-1], device="cpu")
    with pytest.raises(ValueError):
        restore_long(rec, files, masks, seeds=[1], device="cpu")
    with pytest.raises(ValueError):
        restore_long(rec, files[:1], [torch.ones(5)], device="cpu")


def test_smooth_mask_cuts_a_ramp_at_the_ends_of_a_window():
    """A window of a whole recording can start or end inside a gap, or within one cross-fade of it: the Hann ramp is cut at the row's ends
    (the reference's slice assignment raises there); every ramp that fits is the reference's, as before."""
    from audio_inpainting_diffusion_amd.sampler import prepare_smooth_mask
    from oracle.sampler import smooth_mask_rows
    size, n = 20, 400
    hann = torch.hann_window(2 * size)
    m = torch.ones(4, n)
    m[0, :30] = 0                          # the window starts inside a gap: no ramp before it
    m[1, 7:50] = 0                         # a gap 7 samples after the start: the last 7 samples of the fade-out
    m[2, 300:n - 5] = 0                    # the gap ends 5 samples before the end: the first 5 samples of the fade-in
    m[3, 100:200] = 0                      # both ramps fit
    sm = prepare_smooth_mask(m, size)
    want0 = m[0].clone()
    want0[30:30 + size] = hann[:size]
    assert torch.equal(sm[0], want0)
    assert torch.equal(sm[1, :7], hann[2 * size - 7:]) and torch.equal(sm[1, 50:50 + size], hann[:size]) and float(sm[1, 7:50].abs().max()) == 0
    assert torch.equal(sm[2, n - 5:], hann[:5]) and torch.equal(sm[2, 300 - size:300], hann[size:])
    assert torch.equal(sm[3:], smooth_mask_rows(m[3:], size))
    assert float(sm.min()) >= 0.0 and float(sm.max()) <= 1.0
