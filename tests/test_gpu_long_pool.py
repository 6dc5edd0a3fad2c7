"""Whole recordings of DIFFERENT lengths in pooled passes (Sampler.predict_long_pooled, restore.run_pooled_passes, harness ``pool=True``):
the windows of all files share one pass A and one pass B, a chunk of ``max_batch`` windows may span files, and with seeds the result is
bit-equal to what the files give one by one -- a job's result depends on its seed alone, not on the chunk it ran in (restore.run_passes;
tests/test_gpu_long_dist.py relies on the same at this network size).  Reduced network of tests/golden/unet_small_a.npz, T = 2, xi = 0.25:
the fixtures of tests/test_gpu_long_dist.py.

The sampler calls are counted through a wrapper on the sampler: pooled it is sum over the passes of ceil(J_pass / max_batch), unpooled the
sum over the files as well.  The last tests run three ranks on one GPU over gloo, one set of workers for both modes."""
import functools
import os
import queue
import sys
import traceback

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT
from test_gpu_long_dist import _free_port, _lowpass, _samplers

pytestmark = pytest.mark.gpu
DEV, T, K, WORLD = "cuda", 2, 33, 3
PER_JOB = 2 * T - 1                                       # evaluations of one window
N_FFT, HOP = 256, 64                                      # the small sizes of tests/test_gpu_pr_long.py


@functools.lru_cache(maxsize=None)
def _net():
    """(sampler with data consistency, sampler with guidance only, Ls, end) over one network, built once for the module"""
    from audio_inpainting_diffusion_amd.sampler import autoregressive_overlap
    _, smp_dc, smp, Ls = _samplers(DEV)
    for s in (smp_dc, smp):
        s.args.tester.phase_retrieval.win_size, s.args.tester.phase_retrieval.hop_size = N_FFT, HOP
    return smp_dc, smp, Ls, int(autoregressive_overlap(smp.args) * Ls)


def _lengths(Ls, n):
    """n pairwise different lengths: two windows, three, three (300 samples shorter), two"""
    return [Ls + Ls // 2, 2 * Ls + Ls // 3, 2 * Ls + Ls // 3 - 300, Ls + Ls // 2 + 200][:n]


def _recording(N, i):
    return torch.randn(N, generator=torch.Generator().manual_seed(170 + i)) * 0.063


def _gapped(N, Ls, end, i):
    """a mask [N] with a gap inside every window's owned range, as tests/test_gpu_long_dist.py::_inputs places them"""
    from audio_inpainting_diffusion_amd.restore import restore_plan
    mask = torch.ones(N)
    A, B, _ = restore_plan(torch.zeros(1, N), Ls, end)
    for _, s, _, _, lo, hi in A + B:
        c = s + (lo + hi) // 2
        mask[c - 100 - 10 * i:c + 100] = 0
    return mask


def _calls(J_per_pass, max_batch):
    return sum(-(-J // max_batch) for J in J_per_pass if J)


class _Counted:
    """counts the calls of one method of a sampler while it is active; the evaluations through n_evals"""

    def __init__(self, smp, name):
        self.smp, self.name, self.calls, self.batches = smp, name, 0, []

    def __enter__(self):
        inner = getattr(self.smp, self.name)

        def wrapper(y, *a, **k):
            self.calls += 1
            self.batches.append(int(y.shape[0]))
            return inner(y, *a, **k)
        setattr(self.smp, self.name, wrapper)                 # (an instance attribute over the method)
        self.n0 = self.smp.n_evals
        return self

    def __exit__(self, *exc):
        delattr(self.smp, self.name)
        self.evals = self.smp.n_evals - self.n0


def _both(smp, method, run, jobs_per_file, max_batch):
    """run(pool) -> list of results, pooled and unpooled: asserts bit-equality file by file, the evaluations and the call counts, and
    returns the pooled results.  jobs_per_file: [(J_A, J_B)] per file (files of pairwise different lengths)."""
    with _Counted(smp, method) as plain:
        want = run(False)
    with _Counted(smp, method) as pooled:
        got = run(True)
    J = [sum(j[p] for j in jobs_per_file) for p in range(2)]
    print(f"{method}: pooled {pooled.calls} calls at batches {pooled.batches}, unpooled {plain.calls} at {plain.batches}; jobs per pass {J}")
    assert len(got) == len(want) == len(jobs_per_file)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and bool(torch.isfinite(w).all()) and torch.equal(g, w), f"file {i}: max |diff| = {float((g - w).abs().max()):.3e}"
    assert pooled.evals == plain.evals == sum(J) * PER_JOB
    assert pooled.calls == _calls(J, max_batch) and plain.calls == sum(_calls(j, max_batch) for j in jobs_per_file)
    assert pooled.calls < plain.calls
    return got


def test_inpainting_three_lengths_pooled_is_bit_equal_to_file_by_file_in_fewer_sampler_calls():
    """Three files of two, three and three windows, the last two lengths 300 samples apart, a gap in every window's owned range: 5 jobs in
    pass A and 3 in pass B.  max_batch = 4: pooled pass A is chunks of 4 (files 0, 1, 1, 2) and 1, pass B one chunk of 3 -- 3 sampler calls
    against 6 file by file.  Fails on a harness without ``pool``."""
    from audio_inpainting_diffusion_amd import harness
    from audio_inpainting_diffusion_amd.restore import restore_plan
    smp, _, Ls, end = _net()
    Ns = _lengths(Ls, 3)
    files = [_recording(N, i) for i, N in enumerate(Ns)]
    masks = [_gapped(N, Ls, end, i) for i, N in enumerate(Ns)]
    jobs = [tuple(len(p) for p in restore_plan(m, Ls, end)[:2]) for m in masks]
    assert jobs == [(1, 1), (2, 1), (2, 1)] and len(set(Ns)) == 3 and Ns[1] - Ns[2] == 300
    got = _both(smp, "predict_inpainting", lambda pool: harness.restore_long(smp, files, masks, seeds=[31, 32, 33], max_batch=4, device=DEV, pool=pool), jobs, 4)
    assert all(not torch.equal(g.cpu(), f) for g, f in zip(got, files))                               # (something was restored)


def _two_files(Ls):
    Ns = _lengths(Ls, 2)
    return Ns, [_recording(N, i) for i, N in enumerate(Ns)], [(1, 1), (2, 1)]


def test_declipping_two_lengths_a_level_per_file():
    from audio_inpainting_diffusion_amd import harness
    from audio_inpainting_diffusion_amd.declip_long import declip_plan
    _, smp, Ls, end = _net()
    Ns, files, jobs = _two_files(Ls)
    levels = [0.1, 0.08]
    clipped = [f.clamp(-c, c) for f, c in zip(files, levels)]
    assert [tuple(len(p) for p in declip_plan(y[None], [c], Ls, end)[:2]) for y, c in zip(clipped, levels)] == jobs
    _both(smp, "predict_resample", lambda pool: harness.declip_long(smp, clipped, levels, seeds=[41, 42], max_batch=2, device=DEV, pool=pool), jobs, 2)


def test_bwe_firwin_two_lengths():
    from audio_inpainting_diffusion_amd import harness
    _, smp, Ls, end = _net()
    Ns, files, jobs = _two_files(Ls)
    taps = _lowpass(K)
    low = [torch.nn.functional.conv1d(torch.nn.functional.pad(f.double()[None, None], ((K - 1) // 2, K - 1 - (K - 1) // 2)), taps.double()[None, None]).reshape(-1).float()
           for f in files]
    _both(smp, "predict_resample", lambda pool: harness.bwe_long(smp, low, taps, "firwin", seeds=[51, 52], max_batch=2, device=DEV, pool=pool), jobs, 2)


def test_bwe_lowrate_two_to_one_two_lengths():
    from audio_inpainting_diffusion_amd import harness
    from audio_inpainting_diffusion_amd.lowrate_long import lowrate_plan, rate_of
    _, smp, Ls, end = _net()
    Ns, files, jobs = _two_files(Ls)
    low = [f[:N // 2 * 2].reshape(-1, 2).mean(dim=1) for f, N in zip(files, Ns)]              # (any low-rate signal will do: pooled against unpooled)
    rate = rate_of(2, "resample")
    assert (rate.orig, rate.new) == (2, 1)
    assert [tuple(len(p) for p in lowrate_plan(1, 2 * y.numel(), Ls, end, rate)) for y in low] == jobs
    got = _both(smp, "predict_resample", lambda pool: harness.bwe_lowrate_long(smp, low, 2, "resample", seeds=[61, 62], max_batch=2, device=DEV, pool=pool), jobs, 2)
    assert [g.numel() for g in got] == [2 * y.numel() for y in low]


def test_phase_retrieval_two_lengths():
    from audio_inpainting_diffusion_amd import harness
    from audio_inpainting_diffusion_amd.phase_long import pr_plan
    _, smp, Ls, end = _net()
    Ns, files, jobs = _two_files(Ls)

    def mag(x):
        x2 = torch.cat((x.double(), torch.zeros(N_FFT, dtype=torch.float64)))
        return torch.stft(x2, N_FFT, hop_length=HOP, window=torch.hamming_window(N_FFT, dtype=torch.float64), center=False, return_complex=True).abs().float()
    specs = [mag(f) for f in files]
    assert [s.shape[1] for s in specs] == [1 + N // HOP for N in Ns]
    assert [tuple(len(p) for p in pr_plan(1, N, Ls, end, N_FFT, HOP)) for N in Ns] == jobs
    got = _both(smp, "predict_resample", lambda pool: harness.pr_long(smp, specs, lengths=Ns, seeds=[71, 72], max_batch=2, device=DEV, pool=pool), jobs, 2)
    assert [g.numel() for g in got] == Ns


def test_a_file_without_a_job_among_files_with_jobs_comes_back_as_a_copy():
    from audio_inpainting_diffusion_amd import harness
    smp, _, Ls, end = _net()
    Ns = _lengths(Ls, 3)
    files = [_recording(N, i) for i, N in enumerate(Ns)]
    masks = [_gapped(Ns[0], Ls, end, 0), torch.ones(Ns[1]), _gapped(Ns[2], Ls, end, 2)]
    got = _both(smp, "predict_inpainting", lambda pool: harness.restore_long(smp, files, masks, seeds=[31, 32, 33], max_batch=4, device=DEV, pool=pool),
                [(1, 1), (0, 0), (2, 1)], 4)
    assert torch.equal(got[1].cpu(), files[1]) and got[1].data_ptr() != files[1].data_ptr()


def test_files_of_one_length_pooled_equals_unpooled_equals_the_plain_call_and_max_batch_one():
    from audio_inpainting_diffusion_amd import harness
    smp, _, Ls, end = _net()
    N = _lengths(Ls, 2)[1]
    files = [_recording(N, i) for i in range(2)]
    masks = [_gapped(N, Ls, end, i) for i in range(2)]
    seeds = [31, 32]
    plain = smp.predict_inpainting_long(torch.stack(files).to(DEV), torch.stack(masks), max_batch=4, seeds=seeds)
    with _Counted(smp, "predict_inpainting") as unpooled:
        want = harness.restore_long(smp, files, masks, seeds=seeds, max_batch=4, device=DEV)
    with _Counted(smp, "predict_inpainting") as pooled:
        got = harness.restore_long(smp, files, masks, seeds=seeds, max_batch=4, device=DEV, pool=True)
    assert pooled.batches == unpooled.batches == [4, 2]                    # one group: the same calls
    with _Counted(smp, "predict_inpainting") as ones:
        one = harness.restore_long(smp, files, masks, seeds=seeds, max_batch=1, device=DEV, pool=True)
    assert ones.batches == [1] * 6
    for r in range(2):
        assert torch.equal(got[r], plain[r]) and torch.equal(want[r], plain[r]) and torch.equal(one[r], plain[r])


def test_refusals_of_the_pooled_entry_are_those_of_the_plain_methods():
    from audio_inpainting_diffusion_amd import _lib, harness
    smp_dc, smp, Ls, end = _net()
    y = _recording(_lengths(Ls, 1)[0], 0)[None].to(DEV)
    n0 = smp.n_evals + smp_dc.n_evals
    # spectrogram inpainting does not pool, and says why
    with pytest.raises(_lib.AidError, match="one recording-shaped mask"):
        smp.predict_long_pooled("spectrogram_inpainting", [(y, torch.ones(3, 3))])
    with pytest.raises(_lib.AidError, match="one recording-shaped mask"):
        harness.spectrogram_inpainting_long(smp, [y[0]], [torch.ones(3, 3)], device=DEV, pool=True)
    with pytest.raises(NotImplementedError, match="unknown task"):
        smp.predict_long_pooled("denoising", [y])
    # rid: refused by the pooled entry in the words of the plain method
    smp.rid = True
    try:
        for task, groups, kw, call in (("inpainting", [(y, torch.ones_like(y))], {}, lambda: smp.predict_inpainting_long(y, torch.ones_like(y))),
                                       ("declipping", [(y, 0.1)], {}, lambda: smp.predict_declipping_long(y, 0.1)),
                                       ("bwe", [y], dict(filt=_lowpass(K), filt_type="firwin"), lambda: smp.predict_bwe_long(y, _lowpass(K), "firwin"))):
            with pytest.raises(_lib.AidError, match="rid must be False") as plain:
                call()
            with pytest.raises(_lib.AidError, match="rid must be False") as pooled:
                smp.predict_long_pooled(task, groups, **kw)
            assert str(pooled.value) == str(plain.value)
    finally:
        smp.rid = False
    # data consistency, where the mode refuses it
    low = y[:, ::2].contiguous()
    spec = torch.ones(1, N_FFT // 2 + 1, 1 + y.shape[1] // HOP, device=DEV)
    for task, groups, kw, call in (("bwe_lowrate", [(low, None)], dict(factor=2), lambda: smp_dc.predict_bwe_lowrate_long(low, 2)),
                                   ("pr", [(spec, None)], {}, lambda: smp_dc.predict_pr_long(spec))):
        with pytest.raises(_lib.AidError, match="without data consistency") as plain:
            call()
        with pytest.raises(_lib.AidError, match="without data consistency") as pooled:
            smp_dc.predict_long_pooled(task, groups, **kw)
        assert str(pooled.value) == str(plain.value)
    # a fault in a later group is raised before anything is launched; the seeds are counted over all groups
    with pytest.raises(_lib.AidError, match="IIR"):
        smp.predict_long_pooled("bwe", [y], filt=_lowpass(K), filt_type="cheby1")
    with pytest.raises(_lib.AidError, match="does not match"):
        smp.predict_long_pooled("inpainting", [(y, torch.ones_like(y)), (y, torch.ones(1, 5))], seeds=[1, 2])
    with pytest.raises(_lib.AidError, match="3 seeds for 2 recordings"):
        smp.predict_long_pooled("inpainting", [(y, torch.ones_like(y)), (y, torch.ones_like(y))], seeds=[1, 2, 3])
    assert smp.n_evals + smp_dc.n_evals == n0


# ---- three ranks on one GPU ----------------------------------------------------------------------------------------------------------------
DIST_SEEDS, DIST_MAX_BATCH = [81, 82, 83, 84], 2


def _dist_inputs(Ls, end):
    """four files of four lengths, each with one or two jobs per pass: (files, masks, low-passed files, taps), on the host"""
    Ns = _lengths(Ls, 4)
    assert len(set(Ns)) == 4
    files = [_recording(N, i) for i, N in enumerate(Ns)]
    masks = [_gapped(N, Ls, end, i) for i, N in enumerate(Ns)]
    taps = _lowpass(K)
    low = [torch.nn.functional.conv1d(torch.nn.functional.pad(f.double()[None, None], ((K - 1) // 2, K - 1 - (K - 1) // 2)), taps.double()[None, None]).reshape(-1).float()
           for f in files]
    return files, masks, low, taps


def _dist_calls(smp_dc, smp, Ls, end, dev):
    """{name: ([result per file as numpy], increase of n_evals)} of the two pooled harness calls"""
    from audio_inpainting_diffusion_amd import harness
    files, masks, low, taps = _dist_inputs(Ls, end)
    res = {}
    n0 = smp_dc.n_evals
    outs = harness.restore_long(smp_dc, files, masks, seeds=DIST_SEEDS, max_batch=DIST_MAX_BATCH, device=dev, pool=True)
    res["inpainting"] = ([o.cpu().numpy() for o in outs], smp_dc.n_evals - n0)
    n0 = smp.n_evals
    outs = harness.bwe_long(smp, low, taps, "firwin", seeds=DIST_SEEDS, max_batch=DIST_MAX_BATCH, device=dev, pool=True)
    res["bwe"] = ([o.cpu().numpy() for o in outs], smp.n_evals - n0)
    return res


def _worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                          AID_DIST_BACKEND="gloo")
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from audio_inpainting_diffusion_amd import dist as D
        from audio_inpainting_diffusion_amd.sampler import autoregressive_overlap
        D.init_distributed()
        torch.cuda.set_device(0)
        net, smp_dc, smp, Ls = _samplers("cuda:0", seed_offset=rank)             # ranks start with DIFFERENT weights: the broadcast must fix that
        D.broadcast_parameters(net, src=0)
        res = _dist_calls(smp_dc, smp, Ls, int(autoregressive_overlap(smp.args) * Ls), "cuda:0")
        D.barrier()
        q.put((rank, res))
        torch.distributed.destroy_process_group()
    except BaseException:
        q.put((rank, traceback.format_exc()))
        raise


_FAILED = []


def _results():
    """(single-process pooled results, [results of rank 0, 1, 2]); computed once.  A failure is kept as well: after a worker that raised,
    faulted or did not answer, the other tests fail with the same exception and start nothing on the GPU again."""
    if _FAILED:
        raise _FAILED[0]
    try:
        return _spawned_results()
    except (Exception, pytest.fail.Exception) as e:
        _FAILED.append(e)
        raise


@functools.lru_cache(maxsize=None)
def _spawned_results():
    smp_dc, smp, Ls, end = _net()
    ref = _dist_calls(smp_dc, smp, Ls, end, DEV)
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_worker, args=(r, WORLD, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    got = []
    try:
        for _ in range(WORLD):
            got.append(q.get(timeout=600))
            assert isinstance(got[-1][1], dict), got[-1][1]
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
    return ref, [res for _, res in sorted(got, key=lambda t: t[0])]


@pytest.mark.parametrize("call", ["inpainting", "bwe"])
def test_three_ranks_on_one_gpu_hold_the_single_process_pooled_result_bit_for_bit(call):
    ref, ranks = _results()
    want = ref[call][0]
    assert len(want) == 4 and all(np.isfinite(w).all() for w in want)
    for rank, res in enumerate(ranks):
        for i, (g, w) in enumerate(zip(res[call][0], want)):
            assert g.shape == w.shape and np.array_equal(g, w), f"{call}: rank {rank}, file {i}: max |diff| = {np.abs(g - w).max():.3e}"


@pytest.mark.parametrize("call", ["inpainting", "bwe"])
def test_every_rank_evaluates_its_share_of_the_pooled_windows_only(call):
    """Four files give 1 + 2 + 2 + 1 = 6 pooled jobs in pass A and 4 in pass B; a rank's n_evals grows by its shard_range share of both
    times (2 T - 1), and together the ranks do the single process's work once."""
    from audio_inpainting_diffusion_amd.dist import shard_range
    ref, ranks = _results()
    assert ref[call][1] == 10 * PER_JOB
    share = [sum(hi - lo for lo, hi in (shard_range(J, rank, WORLD) for J in (6, 4))) for rank in range(WORLD)]
    assert sum(share) == 10 and min(share) >= 3
    assert [res[call][1] for res in ranks] == [n * PER_JOB for n in share]
