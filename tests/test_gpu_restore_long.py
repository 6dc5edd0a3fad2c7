"""GPU tests of whole-recording restoration (csrc/aid_restore.hip, restore.py, Sampler.predict_inpainting_long): the gather / scatter
kernels bit-exact against torch indexing, the two passes stitched around a stub sampler, one window against predict_inpainting, the
independence of a recording's result from the other recordings and from max_batch on the reduced HIP network, and the refusals.
Toy and reduced-size models only."""
import ast
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2
from test_restore_long_host import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.5
ATOL_OBSERVED = 16 * 2.0 ** -24          # a handful of float32 roundings of values of the recording's size, relative to its largest sample


def _all_windows(N, L, end, R):
    """every window of every recording as a job, whatever the mask: (jobs_A, jobs_B)"""
    from audio_inpainting_diffusion_amd.restore import restore_plan
    return restore_plan(torch.zeros(1, N), L, end, R=R)[:2]


def _strided(R, N, seed, shift):
    """[R, N] view with row stride N + 3 starting ``shift`` elements into its buffer -> (buffer, view), on the host"""
    base = torch.randn(R, N + 3, generator=torch.Generator().manual_seed(seed))
    return base, base[:, shift:shift + N]


# ---- the kernels -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L,end", CASES)
@pytest.mark.parametrize("R", [1, 3])
def test_window_gather_and_scatter_are_bit_exact_against_torch_indexing(N, L, end, R):
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.restore import job_table, window_gather, window_scatter
    A, B = _all_windows(N, L, end, R)
    _, rec = _strided(R, N, 1 + N, 0)
    _, out = _strided(R, N, 2 + N, 1)                                            # (rows of out start at an odd element)
    rec_d = torch.empty(R, N + 3, device=DEV)[:, :N].copy_(rec)
    out_d = torch.empty(R, N + 3, device=DEV)[:, 1:N + 1].copy_(out)
    assert rec_d.stride(0) == N + 3 and out_d.stride(0) == N + 3
    i = torch.arange(L)
    for rows in (1, R):                                                          # shared and per-recording masks
        mask = (torch.rand(rows, N, generator=torch.Generator().manual_seed(3 + N + rows)) < 0.7).float()
        mask_d = mask.to(DEV)
        for jobs in (A, B, A + B):
            if not jobs:
                continue
            y, m = window_gather(rec_d, out_d, mask_d, job_table(jobs, DEV), L)
            assert y.shape == m.shape == (len(jobs), L)
            for j, (r, s, head, tail, lo, hi) in enumerate(jobs):
                q = s + i
                inside, qc = q < N, (s + i).clamp(max=N - 1)
                edge = (i < head) | (i >= L - tail)
                mrow = mask[r if rows > 1 else 0]
                m_ref = torch.where(edge, torch.ones(L), torch.where(inside, mrow[qc], torch.zeros(L)))
                src = torch.where(inside, torch.where(edge, out[r, qc], rec[r, qc]), torch.zeros(L))
                assert torch.equal(m[j].cpu(), m_ref), (rows, j)
                assert torch.equal(y[j].cpu(), m_ref * src), (rows, j)
    for jobs in (A, B):
        if not jobs:
            continue
        x = torch.randn(len(jobs), L, generator=torch.Generator().manual_seed(5 + N))
        buf = torch.full((R, N + 3), SENT, device=DEV)
        guard = torch.full((2, R, N + 3), SENT, device=DEV)                      # neighbours in memory are not the kernel's business either
        window_scatter(x.to(DEV), buf[:, 1:N + 1], job_table(jobs, DEV))
        ref = torch.full((R, N + 3), SENT)
        changed = torch.zeros(R, N, dtype=torch.bool)
        for j, (r, s, head, tail, lo, hi) in enumerate(jobs):
            b = min(s + hi, N)
            ref[r, 1 + s + lo:1 + b] = x[j, lo:lo + b - (s + lo)]
            changed[r, s + lo:b] = True
        assert torch.equal(buf.cpu(), ref)                                       # exactly the owned samples below N changed, the row padding did not
        assert bool((ref[:, 1:N + 1][changed] != SENT).all()) and bool((guard == SENT).all())
    # refusals of the launchers: checked on the host, nothing is launched
    tab = job_table(A, DEV)
    y0 = torch.zeros(len(A), L, device=DEV)
    mask_d = torch.ones(1, N, device=DEV)
    for bad in (dict(rec_ld=N - 1), dict(out_ld=N - 1), dict(mask_ld=N - 1), dict(J=0), dict(J=65536)):
        kw = dict(J=len(A), rec_ld=N + 3, out_ld=N + 3, mask_ld=0)
        kw.update(bad)
        with pytest.raises(_lib.AidError):
            _lib.call("aid_window_gather", _lib.WindowGatherParams(rec_d.data_ptr(), out_d.data_ptr(), mask_d.data_ptr(), y0.data_ptr(), y0.data_ptr(), tab.data_ptr(),
                                                                    kw["J"], R, L, N, kw["rec_ld"], kw["out_ld"], kw["mask_ld"]))
    with pytest.raises(_lib.AidError):
        _lib.call("aid_window_scatter", _lib.WindowScatterParams(y0.data_ptr(), out_d.data_ptr(), tab.data_ptr(), len(A), R, L, N, N - 1))
    assert bool((y0 == 0).all())


def test_an_invalid_job_row_touches_nothing_outside_its_own_output():
    """The table is device memory: a row with a recording outside [0, R), a negative or too large start gathers zeros and scatters nothing;
    head / tail / lo / hi beyond L are clamped."""
    from audio_inpainting_diffusion_amd.restore import job_table, window_gather, window_scatter
    R, N, L = 2, 300, 128
    rec = torch.randn(R, N, generator=torch.Generator().manual_seed(1)).to(DEV)
    out = torch.randn(R, N, generator=torch.Generator().manual_seed(2)).to(DEV)
    mask = torch.ones(1, N, device=DEV)
    jobs = [(R, 0, 0, 0, 0, L), (-1, 0, 0, 0, 0, L), (0, -4, 0, 0, 0, L), (0, N, 0, 0, 0, L), (1, 200, 0, 0, -5, 10 * L), (1, 0, 10 * L, 0, 0, L)]
    tab = job_table(jobs, DEV)
    y, m = window_gather(rec, out, mask, tab, L)
    assert bool((y[:4] == 0).all()) and bool((m[:4] == 0).all())
    assert torch.equal(y[4, :100], rec[1, 200:]) and bool((y[4, 100:] == 0).all()) and bool((m[4, 100:] == 0).all())
    assert torch.equal(y[5], out[1, :L]) and bool((m[5] == 1).all())              # head clamped to L: the whole window observed from out
    buf = torch.full((R, N), SENT, device=DEV)
    x = torch.ones(len(jobs), L, device=DEV)
    window_scatter(x[:5], buf, tab[:5])
    ref = torch.full((R, N), SENT)
    ref[1, 200:] = 1.0
    assert torch.equal(buf.cpu(), ref)


# ---- the two passes around a stub sampler ------------------------------------------------------------------------------------------------
class _Stub:
    """predict_inpainting(y, m) = y + (1 - m) * 7: observed samples pass through, every gap sample becomes 7"""

    def __init__(self):
        self.calls, self.seeds = [], "untouched"

    def predict_inpainting(self, y, m):
        self.calls.append((y.clone(), m.clone(), self.seeds))
        return y + (1 - m) * 7


def _gap_mask(rows, N, L, seed):
    """a few short gaps per row, one of them across the first window boundary the row has"""
    g = torch.Generator().manual_seed(seed)
    mask = torch.ones(rows, N)
    for r in range(rows):
        for st in torch.randint(0, N, (4,), generator=g).tolist():
            mask[r, st:st + 1 + int(torch.randint(0, 40, (1,), generator=g))] = 0
    if N > L:
        mask[0, L - 3:L + 5] = 0
    return mask


@pytest.mark.parametrize("N,L,end", CASES)
@pytest.mark.parametrize("rows,max_batch", [(1, 8), (3, 2), (3, 8)])
def test_two_passes_stitch_the_stub_sampler_output(N, L, end, rows, max_batch):
    from audio_inpainting_diffusion_amd.restore import restore_passes, restore_plan
    R, step = 3, L - end
    buf, rec = _strided(R, N, 11 + N, 1)
    rec_d = torch.empty(R, N + 3, device=DEV)[:, 1:N + 1].copy_(rec)
    mask = _gap_mask(rows, N, L, 12 + N + rows)
    full = mask.expand(R, N)
    A, B, _ = restore_plan(mask, L, end, R=R)
    assert A and (B or N <= L)
    stub, seeds = _Stub(), [5, 6, 7]
    out = restore_passes(stub, rec_d, mask.to(DEV), L, end, max_batch=max_batch, seeds=seeds)
    assert out.is_cuda and torch.equal(out.cpu(), torch.where(full == 1, rec, torch.full((R, N), 7.0)))
    assert stub.seeds == "untouched"
    nA, nB = math.ceil(len(A) / max_batch), math.ceil(len(B) / max_batch)
    assert len(stub.calls) == nA + nB and all(c[0].shape[0] <= max_batch and c[0].shape == c[1].shape for c in stub.calls)
    assert sum(c[0].shape[0] for c in stub.calls) == len(A) + len(B)
    assert sum(c[0].shape[0] for c in stub.calls[:nA]) == len(A)
    got_seeds = [s for c in stub.calls for s in c[2]]
    assert got_seeds == [seeds[r] * 65536 + s // step for r, s, *_ in A + B]
    # what pass B sees at its windows' heads and tails is what pass A left there, bit for bit
    after_A = rec.clone()
    for r, s, head, tail, lo, hi in A:
        after_A[r, s + lo:s + hi] = torch.where(full[r, s + lo:s + hi] == 1, rec[r, s + lo:s + hi], torch.full((hi - lo,), 7.0))
    yB = torch.cat([c[0] for c in stub.calls[nA:]]).cpu() if B else torch.zeros(0, L)
    mB = torch.cat([c[1] for c in stub.calls[nA:]]).cpu() if B else torch.zeros(0, L)
    for j, (r, s, head, tail, lo, hi) in enumerate(B):
        assert head == end and torch.equal(yB[j, :head], after_A[r, s:s + head]) and bool((mB[j, :head] == 1).all())
        if tail:
            assert torch.equal(yB[j, L - tail:], after_A[r, s + L - tail:s + L]) and bool((mB[j, L - tail:] == 1).all())
        n_in = min(L - tail, N - s)
        assert torch.equal(mB[j, head:n_in], full[r, s + head:s + n_in]) and bool((mB[j, n_in:L - tail] == 0).all())
    # the global generator when no seeds are given; an all-ones mask makes no call and returns the recording
    stub2 = _Stub()
    out2 = restore_passes(stub2, rec_d, mask.to(DEV), L, end, max_batch=max_batch)
    assert torch.equal(out2, out) and all(c[2] is None for c in stub2.calls) and stub2.seeds == "untouched"
    stub3 = _Stub()
    out3 = restore_passes(stub3, rec_d, torch.ones(rows, N), L, end, max_batch=max_batch, seeds=seeds)
    assert stub3.calls == [] and torch.equal(out3.cpu(), rec) and out3.data_ptr() != rec_d.data_ptr()


# ---- one window: the existing path -------------------------------------------------------------------------------------------------------
def test_one_window_equals_predict_inpainting_bit_for_bit():
    from test_gpu_generic import _sampler
    L, seed = 4096, 23
    smp = _sampler(L, 3, 0.25)
    rec = (torch.randn(1, L, generator=torch.Generator().manual_seed(4)) * 0.063).to(DEV)
    mask = torch.ones(1, L)
    mask[:, 1500:1900] = 0
    smp.seeds = [99]
    out = smp.predict_inpainting_long(rec, mask, seeds=[seed])
    assert smp.seeds == [99] and out.is_cuda and out.shape == (1, L)
    smp.seeds = [seed * 65536]
    ref = smp.predict_inpainting(rec * mask.to(DEV), mask)
    assert torch.equal(out, ref)
    # (an observed sample of a sampled window is the recording's up to the roundings of the last Euler step onto t = 0, x + h * (x - x_hat) / t)
    assert float((out[:, :1400] - rec[:, :1400]).abs().max()) <= ATOL_OBSERVED * float(rec.abs().max())
    assert not torch.equal(out[:, 1500:1900], rec[:, 1500:1900])


# ---- reduced HIP network: a recording's result depends neither on the other recordings nor on max_batch --------------------------------------
def _small_net(xi=0.25, dc=True):
    """Reduced HIP network (the recipe of tests/test_gpu_degrade.py::_small_net, without the oracle twin)."""
    from audio_inpainting_diffusion_amd.config import small_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.init import seeded_init_
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    from audio_inpainting_diffusion_amd.sampler import Sampler
    z = np.load(os.path.join(GOLDEN, "unet_small_a.npz"))
    kw = ast.literal_eval(str(z["cfg"]))
    args = small_args(**kw)
    args.tester.T, args.tester.posterior_sampling.xi = 3, xi
    args.tester.data_consistency.use = dc                                    # (type "always", smooth, hann_size 50: the shipped tester's)
    net = seeded_init_(Unet_CQT_oct_with_attention(args, torch.device(DEV)), int(z["seed"]), gate_scale=10.0, affine_scale=10.0)
    return Sampler(model=net, diff_params=EDM(args), args=args), kw["audio_len"]


def test_hip_network_result_is_independent_of_the_other_recordings_and_of_max_batch():
    """Two recordings of N = 2 Ls + Ls // 3 samples (three windows each, a gap in every owned range, one across a window boundary), T = 3:
    restored together, each alone, and with max_batch 1 against 8.  form_batch is left unpinned, so the documented bound for results across
    batch compositions applies (<= 5e-6, tests/test_gpu_degrade.py::test_predict_bwe_batch_of_four_takes_the_sub_batch_streams).  The floor
    is printed next to it: predict_inpainting itself on the same window jobs of pass A, at batch 1 against all at once.
    Measured on one MI355X: all four comparisons 0.0 (bit-equal), and so is the floor -- the bound stays at the documented 5e-6."""
    from audio_inpainting_diffusion_amd.restore import job_table, restore_plan, window_gather
    from audio_inpainting_diffusion_amd.sampler import autoregressive_overlap
    smp, Ls = _small_net()
    end = int(autoregressive_overlap(smp.args) * Ls)
    N, hann, step = 2 * Ls + Ls // 3, int(smp.args.tester.data_consistency.hann_size), Ls - end
    rec = (torch.stack([torch.randn(N, generator=torch.Generator().manual_seed(70 + r)) for r in range(2)]) * 0.063).to(DEV)
    mask = torch.ones(2, N)
    for r in range(2):
        mask[r, Ls // 3 + 50 * r:Ls // 3 + 50 * r + 300] = 0                 # window 0
        mask[r, Ls + Ls // 5:Ls + Ls // 5 + 200 + 10 * r] = 0                # window 1 (its middle)
        mask[r, 2 * Ls - 100:2 * Ls + 150] = 0                               # window 2
    mask[0, Ls - 20:Ls + 30] = 0                                             # across the boundary of windows 0 and 1
    mask[0, 2 * step + 7:2 * step + 80] = 0                                  # 7 samples into window 2: its fade-out is cut at the window's start
    mask[1, 2 * step - 30:2 * step + 60] = 0                                 # window 2 starts inside a gap
    mask[1, N - 40:] = 0                                                     # up to the last sample
    A, B, N_pad = restore_plan(mask, Ls, end)
    assert len(A) == 4 and len(B) == 2 and N_pad > N
    seeds = [31, 32]
    n0 = smp.n_evals
    both = smp.predict_inpainting_long(rec, mask, max_batch=8, seeds=seeds)
    assert smp.n_evals - n0 == 6 * (2 * 3 - 1) and both.shape == (2, N) and bool(torch.isfinite(both).all())
    gap = torch.ones(2, N_pad)                                               # (samples from N on are gathered with mask 0: the recording's end is a gap's start)
    gap[:, :N] = (mask == 0).float()
    near_gap = (torch.nn.functional.max_pool1d(gap.unsqueeze(1), 2 * hann + 1, 1, hann).squeeze(1) > 0)[:, :N]
    # observed samples a cross-fade away from every gap are the recording's (up to the roundings of the last Euler step: every window is sampled here)
    assert float((both.cpu()[~near_gap] - rec.cpu()[~near_gap]).abs().max()) <= ATOL_OBSERVED * float(rec.abs().max())
    assert not torch.equal(both.cpu()[mask == 0], rec.cpu()[mask == 0])
    errs = {}
    for r in range(2):
        alone = smp.predict_inpainting_long(rec[r:r + 1], mask[r:r + 1], max_batch=8, seeds=seeds[r:r + 1])
        errs[f"recording {r} alone"] = rel_l2(alone.cpu(), both[r:r + 1].cpu())
    one = smp.predict_inpainting_long(rec, mask, max_batch=1, seeds=seeds)
    for r in range(2):
        errs[f"recording {r} max_batch 1"] = rel_l2(one[r:r + 1].cpu(), both[r:r + 1].cpu())
    yw, mw = window_gather(rec, rec, mask.to(DEV), job_table(A, DEV), Ls)
    smp.seeds = [1, 2, 3, 4]
    whole = smp.predict_inpainting(yw, mw)
    floor = []
    for j in range(4):
        smp.seeds = [j + 1]
        floor.append(rel_l2(smp.predict_inpainting(yw[j:j + 1], mw[j:j + 1]).cpu(), whole[j:j + 1].cpu()))
    print("restore_long batch invariance, rel-L2:", {k: "%.2e" % v for k, v in errs.items()}, "| floor (predict_inpainting, batch 1 vs 4):", ["%.2e" % e for e in floor])
    assert all(e <= 5e-6 for e in errs.values()), errs


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(monkeypatch):
    from audio_inpainting_diffusion_amd import _lib
    from test_gpu_generic import _sampler
    L, N = 4096, 3 * 4096
    launched = []
    orig = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, p: launched.append(name) or orig(name, p))
    rec, mask = torch.zeros(2, N, device=DEV), torch.ones(1, N)
    mask[:, 5000:5100] = 0
    smp = _sampler(L, 2, 0.25)
    with pytest.raises(_lib.AidError, match="GPU only"):
        smp.predict_inpainting_long(rec.cpu(), mask)
    for bad in (torch.ones(1, N - 1), torch.ones(3, N), torch.ones(2, 2, N)):
        with pytest.raises(_lib.AidError, match="does not match"):
            smp.predict_inpainting_long(rec, bad)
    with pytest.raises(_lib.AidError, match="seeds"):
        smp.predict_inpainting_long(rec, mask, seeds=[1])
    with pytest.raises(_lib.AidError, match="max_batch"):
        smp.predict_inpainting_long(rec, mask, max_batch=0)
    with pytest.raises(_lib.AidError, match="rid"):
        _sampler(L, 2, 0.25, _rid=True).predict_inpainting_long(rec, mask)
    for ov in (0.5, 0.75, 0.0):
        with pytest.raises(_lib.AidError, match="end"):
            _sampler(L, 2, 0.25, **{"autoregressive.overlap": ov}).predict_inpainting_long(rec, mask)
    assert launched == [] and smp.y is None and smp.n_evals == 0
