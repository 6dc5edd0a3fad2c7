"""Whole-recording restoration under a process group, on ONE GPU: three ranks share cuda:0 and the collectives run on gloo, staged through
the host (the pattern of tests/test_gpu_dist.py; RCCL refuses two ranks on one device).  restore.run_passes gives every rank
dist.shard_range of each pass, exchanges once per pass and scatters the whole pass on every rank -- the same code an 8-GPU run uses.

One set of three workers runs everything (most of a spawn test is starting Python): predict_inpainting_long, predict_bwe_long (a
WindowOperator with per-item rows on a share), harness.restore_long with seeds = None and, in the workers only, predict_inpainting_long
with max_batch = 1, so that a rank with two jobs in a pass runs two chunks and joins their results before the exchange.  Two recordings
of three windows each give four jobs in pass A and two in pass B, so at world 3 the last rank has no job in pass B.  The single-process
results are computed once, in the parent.  Reduced network of tests/golden/unet_small_a.npz, T = 2, xi = 0.25."""
import ast
import functools
import os
import queue
import socket
import sys
import traceback

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import GOLDEN, ROOT, rel_l2

pytestmark = pytest.mark.gpu
WORLD, T, K, SEEDS, MAX_BATCH = 3, 2, 33, [31, 32], 8
CALLS = ["inpainting", "bwe", "harness", "inpainting, chunks of one"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _samplers(dev, seed_offset=0):
    """(net, sampler for inpainting -- data consistency on, the shipped tester's --, sampler for bandwidth extension -- guidance only, as
    tests/test_gpu_bwe_long.py::_small_net --, Ls): two samplers over ONE network"""
    from audio_inpainting_diffusion_amd.config import small_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.init import seeded_init_
    from audio_inpainting_diffusion_amd.network import Unet_CQT_oct_with_attention
    from audio_inpainting_diffusion_amd.sampler import Sampler
    z = np.load(os.path.join(GOLDEN, "unet_small_a.npz"))
    kw = ast.literal_eval(str(z["cfg"]))
    both = []
    for dc in (True, False):
        args = small_args(**kw)
        args.tester.T, args.tester.posterior_sampling.xi = T, 0.25
        args.tester.data_consistency.use = dc
        both.append(args)
    net = seeded_init_(Unet_CQT_oct_with_attention(both[0], torch.device(dev)), int(z["seed"]) + seed_offset, gate_scale=10.0, affine_scale=10.0)
    return net, Sampler(model=net, diff_params=EDM(both[0]), args=both[0]), Sampler(model=net, diff_params=EDM(both[1]), args=both[1]), kw["audio_len"]


def _lowpass(taps, cutoff=0.5):
    """a windowed-sinc low-pass (float32), unit gain at DC: the _lowpass of tests/test_gpu_bwe_long.py"""
    n = np.arange(taps) - (taps - 1) / 2
    h = np.sinc(cutoff * n) * np.hamming(taps)
    return torch.from_numpy((h / h.sum()).astype(np.float32))


def _inputs(smp, Ls):
    """(recordings [2, N], mask [2, N] with a gap inside every window's owned range, low-passed recordings [2, N], taps), on the host"""
    from audio_inpainting_diffusion_amd.restore import restore_plan
    from audio_inpainting_diffusion_amd.sampler import autoregressive_overlap
    end = int(autoregressive_overlap(smp.args) * Ls)
    N = 2 * Ls + Ls // 3
    rec = torch.stack([torch.randn(N, generator=torch.Generator().manual_seed(70 + r)) for r in range(2)]) * 0.063
    mask = torch.ones(2, N)
    every_A, every_B, _ = restore_plan(torch.zeros(2, N), Ls, end)
    for r, s, _, _, lo, hi in every_A + every_B:
        c = s + (lo + hi) // 2
        mask[r, c - 100 - 10 * r:c + 100] = 0
    A, B, _ = restore_plan(mask, Ls, end)
    assert (len(A), len(B)) == (4, 2) and A == every_A and B == every_B
    taps = _lowpass(K)
    low = torch.nn.functional.conv1d(torch.nn.functional.pad(rec.double()[:, None], ((K - 1) // 2, K - 1 - (K - 1) // 2)), taps.double()[None, None]).squeeze(1).float()
    return rec, mask, low, taps


def _calls(smp_inp, smp_bwe, Ls, dev, harness_seeds, chunks_of_one=False):
    """the calls under test -> {name: (result on the host as numpy, increase of n_evals)}; ``chunks_of_one``: also the inpainting call with
    max_batch = 1 (its single-process reference is the inpainting call itself: another batch composition of the same seeded jobs)"""
    from audio_inpainting_diffusion_amd import harness
    rec, mask, low, taps = _inputs(smp_inp, Ls)
    res = {}
    n0 = smp_inp.n_evals
    out = smp_inp.predict_inpainting_long(rec.to(dev), mask, max_batch=MAX_BATCH, seeds=SEEDS)
    res["inpainting"] = (out.cpu().numpy(), smp_inp.n_evals - n0)
    n0 = smp_bwe.n_evals
    out = smp_bwe.predict_bwe_long(low.to(dev), taps, "firwin", max_batch=MAX_BATCH, seeds=SEEDS)
    res["bwe"] = (out.cpu().numpy(), smp_bwe.n_evals - n0)
    n0 = smp_inp.n_evals
    outs = harness.restore_long(smp_inp, [rec[0], rec[1]], [mask[0], mask[1]], seeds=harness_seeds, max_batch=MAX_BATCH, device=dev)
    res["harness"] = (torch.stack(outs).cpu().numpy(), smp_inp.n_evals - n0)
    if chunks_of_one:
        n0 = smp_inp.n_evals
        out = smp_inp.predict_inpainting_long(rec.to(dev), mask, max_batch=1, seeds=SEEDS)
        res["inpainting, chunks of one"] = (out.cpu().numpy(), smp_inp.n_evals - n0)
    return res


def _worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                          AID_DIST_BACKEND="gloo")
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from audio_inpainting_diffusion_amd import dist as D
        r, _, w = D.init_distributed()
        torch.cuda.set_device(0)
        net, smp_inp, smp_bwe, Ls = _samplers("cuda:0", seed_offset=rank)        # ranks start with DIFFERENT weights: the broadcast must fix that
        D.broadcast_parameters(net, src=0)
        res = _calls(smp_inp, smp_bwe, Ls, "cuda:0", None, chunks_of_one=True)     # (the harness call without seeds: dist.item_seeds under the group)
        D.barrier()
        q.put((rank, res))
        torch.distributed.destroy_process_group()
    except BaseException:
        q.put((rank, traceback.format_exc()))
        raise


_FAILED = []


def _results():
    """(single-process results, [results of rank 0, 1, 2]); computed once for all the tests below.  A failure is kept as well: after a worker
    that raised, faulted or did not answer, the other tests fail with the same exception and start nothing on the GPU again."""
    if _FAILED:
        raise _FAILED[0]
    try:
        return _spawned_results()
    except (Exception, pytest.fail.Exception) as e:
        _FAILED.append(e)
        raise


@functools.lru_cache(maxsize=None)
def _spawned_results():
    from audio_inpainting_diffusion_amd import dist as D
    net, smp_inp, smp_bwe, Ls = _samplers("cuda")
    ref = _calls(smp_inp, smp_bwe, Ls, "cuda", D.item_seeds(0, 0, 2))
    ref["inpainting, chunks of one"] = ref["inpainting"]
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


@pytest.mark.parametrize("call", CALLS)
def test_three_ranks_on_one_gpu_return_the_single_process_result_on_every_rank(call):
    """Every rank holds the same full result, and it is the single process's: rel-L2 <= 5e-6, the documented bound for results across batch
    compositions (tests/test_gpu_degrade.py::test_predict_bwe_batch_of_four_takes_the_sub_batch_streams) -- a rank's chunk is another batch
    composition of the same seeded jobs.  Bit-equal is expected.  "harness": restore_long with seeds = None under the group against the
    single-process call with seeds = dist.item_seeds(0, 0, 2).  "inpainting, chunks of one": max_batch = 1 under the group (rank 0 runs two
    chunks in pass A) against the single process's max_batch = 8."""
    ref, ranks = _results()
    want = ref[call][0]
    assert np.isfinite(want).all() and want.shape[0] == 2
    for rank, res in enumerate(ranks):
        got = res[call][0]
        e = rel_l2(got, want)
        print(f"{call}: rank {rank}/{WORLD} vs single process: rel-L2 = {e:.2e}")
        assert got.shape == want.shape and e <= 5e-6
        assert np.array_equal(got, ranks[0][call][0])                       # the same on all ranks


@pytest.mark.parametrize("call", CALLS)
def test_every_rank_evaluates_its_share_of_the_windows_only(call):
    """n_evals of a rank grows by (its jobs in pass A + its jobs in pass B) * (2 T - 1); together the ranks do the single process's work once."""
    from audio_inpainting_diffusion_amd.dist import shard_range
    ref, ranks = _results()
    per_job = 2 * T - 1
    assert ref[call][1] == 6 * per_job
    share = [sum(hi - lo for lo, hi in (shard_range(J, rank, WORLD) for J in (4, 2))) for rank in range(WORLD)]
    assert share == [3, 2, 1]
    assert [res[call][1] for res in ranks] == [n * per_job for n in share]
    assert sum(res[call][1] for res in ranks) == ref[call][1]
