"""CPU tests (no GPU) of bandwidth extension of whole recordings that are also clipped and have dropouts (bwe_declip_long.py,
Sampler.predict_bwe_declip_long, harness.bwe_declip_long): the states of a window under a mask against plain indexing, the refusals, all
raised before anything touches a GPU, the pooled task, the harness wrapper, the ABI entries, and the two passes stitched around a stub
sampler with the three launches replaced by their host references."""
import math

import numpy as np
import pytest
import torch

from test_bwe_long_host import BWE_CASES
from test_bwe_long_host import _stub_sampler as _dc_sampler


def _stub_sampler(rid=False, dc=None):
    """the stub sampler of test_bwe_long_host.py with tester.data_consistency off (the mode is guidance only), or in use as ``dc`` says"""
    smp, L = _dc_sampler(rid=rid)
    smp.data_consistency, smp.data_consistency_end = dc == "always", dc == "end"
    return smp, L


def _mask(N, L, end, K, rows, seed):
    """[rows, N] of ones with gaps that cross every window border, the P reach behind a window start and the Q reach before a window end,
    a few gaps elsewhere, single dropped samples, and (row 0) a gap over the last samples of the recording"""
    g = torch.Generator().manual_seed(seed)
    P = (K - 1) // 2
    Q = K - 1 - P
    step = L - end
    m = torch.ones(rows, N)
    for r in range(rows):
        for s in range(0, N, step):
            for a, b in ((s - 3 - r, s + 2), (s + P - 2, s + P + 3 + r), (s + L - Q - 3, s + L - Q + 2), (s + L - 2, s + L + 3), (s + end - 2 - r, s + end + 1)):
                m[r, max(a, 0):max(min(b, N), 0)] = 0
        for a in torch.randint(0, N, (4,), generator=g).tolist():
            m[r, a:a + 1 + a % 7] = 0
    m[0, N - 5:] = 0
    return m


def _state_by_indexing(N, L, K, s, head, tail, row):
    P = (K - 1) // 2
    Q = K - 1 - P
    k = np.empty(L, dtype=np.float32)
    for i in range(L):
        q = s + i
        if q >= N:
            k[i] = -2
        elif i < head or i >= L - tail:
            k[i] = 1
        elif (s > 0 and i < P) or (s + L < N and i >= L - Q):
            k[i] = -1
        elif row is not None and row[q] == 0:
            k[i] = -1
        else:
            k[i] = 0
    return k


@pytest.mark.parametrize("N,L,end,K", BWE_CASES)
def test_window_state_with_a_mask_against_plain_indexing(N, L, end, K):
    from audio_inpainting_diffusion_amd import bwe_long
    from audio_inpainting_diffusion_amd.bwe_declip_long import window_state
    mask = _mask(N, L, end, K, 2, N + K)
    changed = 0
    for r in range(2):
        for s, head, tail, lo, hi in bwe_long.bwe_windows(N, L, end, K):
            plain = bwe_long.window_state(N, L, K, s, head, tail)
            assert np.array_equal(window_state(N, L, K, s, head, tail), plain) and np.array_equal(window_state(N, L, K, s, head, tail, None), plain)
            assert np.array_equal(window_state(N, L, K, s, head, tail, torch.ones(N)), plain)
            for row in (mask[r], mask[r].numpy(), mask[r].bool()):
                k = window_state(N, L, K, s, head, tail, row)
                assert k.dtype == np.float32 and np.array_equal(k, _state_by_indexing(N, L, K, s, head, tail, mask[r].tolist()))
            # only filtered samples change, and only into "unobserved": known, absent and unobserved samples ignore the mask
            diff = k != plain
            assert bool((plain[diff] == 0).all()) and bool((k[diff] == -1).all())
            changed += int(diff.sum())
    assert changed > 0


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_is_raised_before_any_launch(monkeypatch):
    from audio_inpainting_diffusion_amd import _lib, bwe_declip_long, bwe_long, dist
    launched = []
    monkeypatch.setattr(_lib, "call", lambda name, p: launched.append(name))
    monkeypatch.setattr(bwe_long, "bwe_plan", lambda *a, **k: launched.append("plan"))
    smp, L = _stub_sampler()
    smp.seeds = [5]
    N, end = 3 * L, L // 4
    step = L - end
    taps = torch.ones(33) / 33
    y = torch.zeros(2, N)                                                    # (on the host: a valid call is refused for that, every other one for its own reason)
    ok = [dict(), dict(clip_value=0.5), dict(clip_value=[0.5, 0.25]), dict(clip_value=torch.tensor([0.5, 0.25])), dict(mask=torch.ones(N)),
          dict(mask=torch.ones(1, N)), dict(mask=torch.ones(2, N), clip_value=0.1, max_batch=1, seeds=[1, 2])]
    for kw in ok:
        with pytest.raises(_lib.AidError, match="GPU only"):
            smp.predict_bwe_declip_long(y, taps, "firwin", **kw)
    with pytest.raises(_lib.AidError, match="GPU only"):
        smp.predict_bwe_declip_long(y, taps[None, None, :], "firwin_hpf")
    with pytest.raises(_lib.AidError, match="GPU only"):
        bwe_declip_long.bwe_declip_passes(smp, y, taps, "firwin", 0.5, None, L, end)
    # every non-FIR type, with bwe_long.NOT_WINDOWED's reason, in one sentence
    assert set(bwe_long.NOT_WINDOWED) == {"cheby1", "biquad", "decimate", "resample"}
    for ftype, why in bwe_long.NOT_WINDOWED.items():
        with pytest.raises(_lib.AidError) as e:
            smp.predict_bwe_declip_long(y, 2, ftype, clip_value=0.5)
        assert why in str(e.value) and repr(ftype) in str(e.value) and str(e.value).count(". ") == 0
    with pytest.raises(NotImplementedError):
        smp.predict_bwe_declip_long(y, taps, "butterworth")
    with pytest.raises(_lib.AidError, match=r"2 \(K - 1\)"):
        smp.predict_bwe_declip_long(y, torch.ones(end // 2 + 2), "firwin")   # end < 2 (K - 1), three windows
    for bad in (torch.ones(2, 33), torch.ones(0), torch.tensor(1.0)):
        with pytest.raises(_lib.AidError, match="taps"):
            smp.predict_bwe_declip_long(y, bad, "firwin")
    for bad in (y.double(), y.half(), y.long(), y[0], y.numpy()):
        with pytest.raises(_lib.AidError, match="float32 recordings"):
            smp.predict_bwe_declip_long(bad, taps, "firwin")
    # the levels: declip_long.clip_levels' refusals
    for bad in (0.0, -0.5, float("inf"), float("nan"), [0.5, 0.0], []):
        with pytest.raises(_lib.AidError, match="finite and > 0"):
            smp.predict_bwe_declip_long(y, taps, "firwin", clip_value=bad)
    for bad in ([0.5, 0.5, 0.5], torch.ones(3)):
        with pytest.raises(_lib.AidError, match="3 clip levels for 2 recordings"):
            smp.predict_bwe_declip_long(y, taps, "firwin", clip_value=bad)
    # the mask
    for bad in (torch.ones(N - 1), torch.ones(1, N + 1), torch.ones(3, N), torch.ones(2, 1, N), torch.ones(())):
        with pytest.raises(_lib.AidError, match="mask .* does not match recordings"):
            smp.predict_bwe_declip_long(y, taps, "firwin", mask=bad)
    with pytest.raises(_lib.AidError, match="mask must be a tensor"):
        smp.predict_bwe_declip_long(y, taps, "firwin", mask=[1.0] * N)
    # rid, and data consistency in use: no projection exists for the clipped filter
    with pytest.raises(_lib.AidError, match="rid"):
        _stub_sampler(rid=True)[0].predict_bwe_declip_long(y, taps, "firwin")
    for dc_type in ("always", "end"):
        dc, _ = _stub_sampler(dc=dc_type)
        with pytest.raises(_lib.AidError, match="no projection exists for the clipped filter"):
            dc.predict_bwe_declip_long(y, taps, "firwin", clip_value=0.5)
        with pytest.raises(_lib.AidError, match="no projection exists for the clipped filter"):
            dc.predict_long_pooled("bwe_declip", [(y, 0.5, None)], filt=taps, filt_type="firwin")
    # a window without any observation: window 2 (even, not the first) of recording 1 alone
    K = 33
    P, Q = 16, 16
    mask = torch.ones(2, N)
    mask[1, 2 * step + P:2 * step + L - Q] = 0
    with pytest.raises(_lib.AidError, match=r"recording 1, window 2 .*neither a filtered nor a known sample"):
        smp.predict_bwe_declip_long(y, taps, "firwin", mask=mask, max_batch=0)                # (before max_batch is judged)
    with pytest.raises(_lib.AidError, match=r"recording 0, window 2 "):
        smp.predict_bwe_declip_long(y, taps, "firwin", mask=mask[1])                          # one row, shared: recording 0 is named first
    with pytest.raises(_lib.AidError, match=r"recording 0, window 0 "):
        smp.predict_bwe_declip_long(y, taps, "firwin", mask=torch.zeros(N))
    mask[1, 2 * step + P + 7] = 1                                                             # one kept sample: a job like any other
    with pytest.raises(_lib.AidError, match="GPU only"):
        smp.predict_bwe_declip_long(y, taps, "firwin", mask=mask)
    odd = torch.ones(N)
    odd[step:step + L] = 0                                                                     # an odd window wholly dropped keeps its known head
    odd[:P + 1] = 1
    odd[2 * step + L // 2] = 1
    with pytest.raises(_lib.AidError, match="GPU only"):
        smp.predict_bwe_declip_long(y, taps, "firwin", mask=odd)
    # max_batch, the seeds and, last, the device
    for bad in (0, -2, 1.5, True):
        with pytest.raises(_lib.AidError, match="max_batch"):
            smp.predict_bwe_declip_long(y, taps, "firwin", max_batch=bad)
    for bad in ([1], [1, 2, 3]):
        with pytest.raises(_lib.AidError, match="seeds"):
            smp.predict_bwe_declip_long(y, taps, "firwin", seeds=bad)
    with pytest.raises(_lib.AidError, match="seeds"):
        bwe_declip_long.check_bwe_declip_args(y, 0.5, None, bwe_declip_long.bwe_declip_prepare(None, taps, "firwin"), L, end, 8, [1])
    with pytest.raises(_lib.AidError, match="GPU only"):
        bwe_declip_long.check_bwe_declip_args(y, 0.5, None, bwe_declip_long.bwe_declip_prepare(None, taps, "firwin"), L, end, 8, [1, 2])
    # seeds = None under a process group
    monkeypatch.setattr(dist, "_active", lambda: True)
    with pytest.raises(_lib.AidError, match="under a process group needs seeds") as e:
        smp.predict_bwe_declip_long(y, taps, "firwin", clip_value=0.5)
    assert "GPU only" not in str(e.value)
    with pytest.raises(_lib.AidError, match="GPU only"):
        smp.predict_bwe_declip_long(y, taps, "firwin", clip_value=0.5, seeds=[1, 2])
    assert launched == [] and smp.seeds == [5] and smp.y is None and smp.spectral is None and smp.n_evals == 0


def test_check_returns_the_taps_the_levels_and_the_mask_rows(monkeypatch):
    """``None`` for the clip level is carried as +inf per recording, a one-row mask as [1, N]"""
    from audio_inpainting_diffusion_amd import bwe_declip_long, restore
    L, end, N = 256, 64, 600
    y = torch.zeros(3, N)
    calls = []
    monkeypatch.setattr(restore, "check_batch", lambda *a: calls.append(a))  # (the device of y, judged last)
    taps, levels, mask = bwe_declip_long.check_bwe_declip_args(y, None, None, bwe_declip_long.bwe_declip_prepare(None, torch.ones(1, 1, 9), "firwin"), L, end, 8, None)
    assert taps.shape == (9,) and levels.dtype == np.float32 and levels.tolist() == [math.inf] * 3 and mask is None
    taps, levels, mask = bwe_declip_long.check_bwe_declip_args(y, 0.1, torch.ones(N), bwe_declip_long.bwe_declip_prepare(None, torch.ones(9), "firwin"), L, end, 8, None)
    assert levels.tolist() == [np.float32(0.1)] * 3 and mask.shape == (1, N)
    _, levels, mask = bwe_declip_long.check_bwe_declip_args(y, [0.1, 0.2, 0.3], torch.ones(3, N), bwe_declip_long.bwe_declip_prepare(None, torch.ones(9), "firwin_hpf"), L, end, 8, None)
    assert np.array_equal(levels, np.array([0.1, 0.2, 0.3], dtype=np.float32)) and mask.shape == (3, N)
    assert len(calls) == 3


def test_the_operator_refuses_on_the_host_what_it_can():
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.bwe_declip_long import FIRClipObserved
    with pytest.raises(_lib.AidError, match="state must be a float32 GPU tensor"):
        FIRClipObserved(torch.ones(9), torch.zeros(2, 64), [0.5, 0.5])


# ---- the pooled task, the harness wrapper, the ABI -----------------------------------------------------------------------------------------
def test_the_pooled_task_and_the_harness_wrapper():
    from audio_inpainting_diffusion_amd import _lib, harness
    smp, L = _stub_sampler()
    taps = torch.ones(9) / 9
    assert "bwe_declip" in smp.POOLED_TASKS
    y = torch.zeros(1, 2 * L)
    for bad in (dict(), dict(filt=taps), dict(filt=taps, filt_type="firwin", factor=2), dict(factor=2)):
        with pytest.raises(TypeError, match="filt, filt_type"):
            smp.predict_long_pooled("bwe_declip", [y], **bad)
    with pytest.raises(_lib.AidError, match="IIR filter carries state"):
        smp.predict_long_pooled("bwe_declip", [y], filt=taps, filt_type="cheby1")
    # groups are (y, clip_value, mask); a missing entry is None
    for groups in ([y, torch.zeros(2, 3 * L)], [(y,), (torch.zeros(2, 3 * L), [0.5, 0.25])], [(y, 0.5, torch.ones(2 * L)), (torch.zeros(2, 3 * L), None, torch.ones(2, 3 * L))]):
        with pytest.raises(_lib.AidError, match="GPU only"):
            smp.predict_long_pooled("bwe_declip", groups, filt=taps, filt_type="firwin", seeds=[1, 2, 3])
    with pytest.raises(_lib.AidError, match="3 clip levels for 2 recordings"):
        smp.predict_long_pooled("bwe_declip", [(torch.zeros(2, 3 * L), [0.5] * 3), (y, 0.5)], filt=taps, filt_type="firwin")
    with pytest.raises(_lib.AidError, match="recording 0, window 0 "):
        smp.predict_long_pooled("bwe_declip", [(y, None, torch.zeros(2 * L))], filt=taps, filt_type="firwin")

    class Rec:
        def __init__(self):
            self.calls = []

        def predict_bwe_declip_long(self, y, filt, filt_type, clip_value=None, mask=None, max_batch=8, seeds=None):
            self.calls.append((tuple(y.shape), filt, filt_type, clip_value, mask, max_batch, seeds))
            return y + 1

        def predict_long_pooled(self, task, groups, max_batch=8, seeds=None, **task_args):
            self.calls.append((task, groups, max_batch, seeds, task_args))
            return [g[0] + 2 for g in groups]

    files = [torch.full((n,), float(k)) for k, n in enumerate((700, 300, 700, 301, 300))]
    masks = [None, torch.zeros(300), torch.ones(700) * 2, None, None]
    rec = Rec()
    out = harness.bwe_declip_long(rec, files, taps, "firwin_hpf", clip_values=[0.1, 0.2, 0.3, 0.4, 0.5], masks=masks, seeds=[10, 11, 12, 13, 14], max_batch=4, device="cpu")
    assert [c[0] for c in rec.calls] == [(2, 700), (2, 300), (1, 301)] and all(c[5] == 4 and c[2] == "firwin_hpf" and c[1] is taps for c in rec.calls)
    assert [c[3] for c in rec.calls] == [[0.1, 0.3], [0.2, 0.5], [0.4]] and [c[6] for c in rec.calls] == [[10, 12], [11, 14], [13]]
    assert torch.equal(rec.calls[0][4], torch.stack([torch.ones(700), torch.ones(700) * 2])) and torch.equal(rec.calls[1][4], torch.stack([torch.zeros(300), torch.ones(300)]))
    assert rec.calls[2][4] is None and all(torch.equal(o, f + 1) for o, f in zip(out, files))
    rec = Rec()
    harness.bwe_declip_long(rec, files, taps, device="cpu")                  # "firwin", no clipping, no dropouts, the global generator
    assert all(c[2] == "firwin" and c[3] is None and c[4] is None and c[6] is None for c in rec.calls)
    rec = Rec()
    harness.bwe_declip_long(rec, files, taps, clip_values=0.25, device="cpu")
    assert [c[3] for c in rec.calls] == [[0.25, 0.25], [0.25, 0.25], [0.25]]
    rec = Rec()
    out = harness.bwe_declip_long(rec, files, taps, clip_values=0.25, masks=masks, seeds=[10, 11, 12, 13, 14], device="cpu", pool=True)
    (task, groups, mb, sd, targs), = rec.calls
    assert task == "bwe_declip" and mb == 8 and sd == [10, 12, 11, 14, 13] and targs == dict(filt=taps, filt_type="firwin")
    assert [tuple(g[0].shape) for g in groups] == [(2, 700), (2, 300), (1, 301)] and [g[1] for g in groups] == [[0.25, 0.25], [0.25, 0.25], [0.25]]
    assert groups[0][2].shape == (2, 700) and groups[2][2] is None and all(torch.equal(o, f + 2) for o, f in zip(out, files))
    for bad in (dict(seeds=[1]), dict(clip_values=[0.1, 0.2]), dict(masks=masks[:2]), dict(masks=[torch.ones(5)] + masks[1:])):
        with pytest.raises(ValueError):
            harness.bwe_declip_long(rec, files, taps, device="cpu", **bad)


def test_the_new_entries_ride_on_the_existing_structs():
    from audio_inpainting_diffusion_amd import _lib
    bwe = next(a for a in _lib.ABIS if a.header == "aid_bwe_long.h")
    res = next(a for a in _lib.ABIS if a.header == "aid_restore.h")
    assert bwe.version == 1 and set(bwe.structs.values()) == {_lib.FirObservedParams, _lib.BweGatherParams}
    assert res.version == 1 and set(res.structs.values()) == {_lib.WindowGatherParams, _lib.WindowScatterParams}
    assert bwe.launches["aid_fir_clip_observed"] is _lib.FirObservedParams and res.launches["aid_gap_states"] is _lib.WindowGatherParams
    assert all(hasattr(_lib.lib(), name) for name in ("aid_fir_clip_observed", "aid_gap_states"))


# ---- the two passes around a stub sampler, the launches replaced by their host references -------------------------------------------------
class _Stub:
    """predict_resample(y, shape, op)[j, i] = w_j * L + i + r_j / 4, with (r_j, w_j) read from the job's seed (r_j + 1) * 65536 + w_j: every sample
    names the window it was written from (the stub of tests/test_gpu_bwe_long.py)."""

    def __init__(self):
        self.calls, self.seeds = [], "untouched"

    def predict_resample(self, y, shape, op):
        yw, (kw, cw, taps) = y, op
        assert tuple(shape) == tuple(yw.shape) == tuple(kw.shape) and cw.shape == (yw.shape[0],)
        self.calls.append((yw.clone(), kw.clone(), cw.clone(), taps.clone(), self.seeds))
        L = yw.shape[1]
        if self.seeds is None:                                               # (the global generator: nothing names the window)
            return yw + 1
        base = torch.tensor([(s % 65536) * L + (s // 65536 - 1) / 4 for s in self.seeds], dtype=torch.float32)
        return base[:, None] + torch.arange(L, dtype=torch.float32)[None, :]


def _host_launches(monkeypatch):
    """aid_bwe_gather, aid_gap_states and aid_window_scatter as Python indexing over host tensors; the operator as the tuple of its inputs"""
    from audio_inpainting_diffusion_amd import bwe_declip_long, bwe_long, restore
    counts = {"gather": 0, "gap": 0, "scatter": 0}

    def gather(rec, out, jobs, L, K):
        counts["gather"] += 1
        N = rec.shape[1]
        i = torch.arange(L)
        ys, ks = [], []
        for r, s, head, tail, lo, hi in jobs.tolist():
            k = torch.from_numpy(bwe_long.window_state(N, L, K, s, head, tail))
            qc = (s + i).clamp(max=N - 1)
            ys.append(torch.where(k == 1, out[r, qc], torch.where(k == 0, rec[r, qc], torch.zeros(L))))
            ks.append(k)
        return torch.stack(ys), torch.stack(ks)

    def gap(y, k, mask, jobs, R, N):
        counts["gap"] += 1
        L = y.shape[1]
        for j, (r, s, *_) in enumerate(jobs.tolist()):
            n_in = min(L, N - s)
            drop = (k[j, :n_in] == 0) & (mask[r if mask.shape[0] > 1 else 0, s:s + n_in] == 0)
            k[j, :n_in][drop] = -1
            y[j, :n_in][drop] = 0

    def scatter(x, out, table):
        counts["scatter"] += 1
        for row, (r, s, head, tail, lo, hi) in zip(x, table.tolist()):
            out[r, s + lo:s + hi] = row[lo:hi]

    monkeypatch.setattr(bwe_long, "bwe_gather", gather)
    monkeypatch.setattr(bwe_declip_long, "gap_states", gap)
    monkeypatch.setattr(restore, "window_scatter", scatter)
    monkeypatch.setattr(restore, "check_batch", lambda *a: None)               # (the device of y: the host stands in for the GPU here)
    monkeypatch.setattr(bwe_declip_long, "FIRClipObserved", lambda taps, kw, cw: (kw, cw, taps))
    return counts


@pytest.mark.parametrize("N,L,end,K", BWE_CASES)
@pytest.mark.parametrize("max_batch", [2, 8])
def test_two_stubbed_passes_stitch_the_recording(N, L, end, K, max_batch, monkeypatch):
    from audio_inpainting_diffusion_amd import bwe_declip_long, bwe_long
    counts = _host_launches(monkeypatch)
    R, step = 3, L - end
    rec = torch.randn(R, N, generator=torch.Generator().manual_seed(11 + N))
    mask = _mask(N, L, end, K, R, 5 + N)
    levels = [0.5, 0.25, 2.0]
    taps = torch.randn(K, generator=torch.Generator().manual_seed(K))
    A, B = bwe_long.bwe_plan(R, N, L, end, K)
    assert A and (B or N <= L)
    stub, seeds = _Stub(), [1, 2, 3]
    out = bwe_declip_long.bwe_declip_passes(stub, rec, taps, "firwin", levels, mask, L, end, max_batch=max_batch, seeds=seeds)
    assert out.shape == (R, N) and stub.seeds == "untouched" and out is not rec
    # every sample of [0, N) comes from the window that owns it, and from no other
    want = torch.full((R, N), float("nan"))
    for r, s, head, tail, lo, hi in A + B:
        assert bool(torch.isnan(want[r, s + lo:s + hi]).all())
        want[r, s + lo:s + hi] = (s // step) * L + torch.arange(lo, hi) + r / 4
    assert torch.equal(out, want)
    nA, nB = math.ceil(len(A) / max_batch), math.ceil(len(B) / max_batch)
    assert len(stub.calls) == nA + nB and all(c[0].shape[0] <= max_batch for c in stub.calls)
    assert counts == {"gather": 2 if B else 1, "gap": 2 if B else 1, "scatter": nA + nB}       # two gather launches per pass, one scatter per call
    assert [s for c in stub.calls for s in c[4]] == [seeds[r] * 65536 + s // step for r, s, *_ in A + B]
    assert all(torch.equal(c[3], taps) for c in stub.calls)
    ys, ks, cs = (torch.cat([c[i] for c in stub.calls]) for i in range(3))
    assert cs.tolist() == [np.float32(levels[r]) for r, *_ in A + B]                           # the level of a job is its recording's
    for j, (r, s, head, tail, lo, hi) in enumerate(A + B):
        k_ref = torch.from_numpy(bwe_declip_long.window_state(N, L, K, s, head, tail, mask[r]))
        n_in = min(L, N - s)
        assert torch.equal(ks[j], k_ref) and bool((ys[j][k_ref < 0] == 0).all())
        obs = (k_ref == 0)[:n_in]
        assert torch.equal(ys[j, :n_in][obs], rec[r, s:s + n_in][obs]) and bool((mask[r, s:s + n_in][obs] != 0).all())
        if j >= len(A):
            assert torch.equal(ys[j, :head], want[r, s:s + head]) and bool((k_ref[:head] == 1).all())
            if tail:
                assert torch.equal(ys[j, L - tail:], want[r, s + L - tail:s + L])
    # without a mask the second gather launch is not made; without levels every job carries +inf; no seeds: the global generator
    for k in counts:
        counts[k] = 0
    plain = _Stub()
    bwe_declip_long.bwe_declip_passes(plain, rec, taps, "firwin_hpf", None, None, L, end, max_batch=max_batch)
    assert counts["gap"] == 0 and counts["gather"] == (2 if B else 1) and all(c[4] is None for c in plain.calls) and plain.seeds == "untouched"
    assert all(bool(torch.isinf(c[2]).all()) and bool((c[2] > 0).all()) for c in plain.calls)
    ks0 = torch.cat([c[1] for c in plain.calls])
    for j, (r, s, head, tail, lo, hi) in enumerate(A + B):
        assert torch.equal(ks0[j], torch.from_numpy(bwe_long.window_state(N, L, K, s, head, tail)))
