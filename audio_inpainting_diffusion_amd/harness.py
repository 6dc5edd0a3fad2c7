"""Host-side harness pieces around the sampler.

* ``load_checkpoint(net, path_or_state)`` -- what ``Tester.load_checkpoint`` does for the inpainting tester
  (testing/tester_inpainting.py:195-202 -> utils/training_utils.py:214-289 with ``ema=network``): load
  ``state['ema']`` strictly, else non-strictly, else key-by-key where the shapes agree.  Our network carries the
  reference's state_dict keys, so released checkpoints go through the first strategy; kernel-side weight packs are
  rebuilt from the parameter versions on the next evaluation.
* ``centre_gap_window`` / ``inpaint_long`` -- the long-file path of the tester (:382-418): the gap sits at the centre of
  the file, a window of ``audio_len`` samples centred on it goes through the sampler, the result is stitched back.
  The reference handles one file per sampler call; here B files form one batch with per-item masks.
* ``restore_long`` -- whole files of unequal lengths with gaps anywhere, through ``Sampler.predict_inpainting_long`` (restore.py: two
  batched passes over windows on the autoregressive grid).
No device code here; everything numerical happens in the sampler / network.
"""
from __future__ import annotations

import types
from typing import Callable, NamedTuple, Optional, List, Sequence, Tuple

import torch


def cqt_is_pinned() -> bool:
    """True when a dump of the real ``cqt_nsgt_pytorch`` (tests/golden/cqt_ref_*.npz, made by tests/golden/make_cqt_golden.py)
    sits next to this checkout -- the conformance tests then hold our CQT to the package the checkpoints were trained with."""
    import glob
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return bool(glob.glob(os.path.join(root, "tests", "golden", "cqt_ref_*.npz")))


class UnpinnedCQTError(RuntimeError):
    pass


def load_checkpoint(net, state, key: str = "ema", cqt_pinned: Optional[bool] = None, allow_unpinned_cqt: bool = False) -> Tuple[int, str]:
    """Returns (iteration stored in the checkpoint or 0, strategy used: 'strict' | 'non-strict' | 'shape-matched').

    Trained weights only mean something on the transform they were trained with.  The reference's CQT is the external
    package ``cqt_nsgt_pytorch``; ours follows the same call contract but its frame design is pinned to the package only
    once the conformance fixtures exist (one command: tools/pin_external.sh).  Until then this function
    REFUSES (``UnpinnedCQTError``) unless the caller opts out with ``allow_unpinned_cqt=True``, which still warns."""
    import warnings
    if cqt_pinned is None:
        cqt_pinned = cqt_is_pinned()
    if not cqt_pinned and hasattr(net, "CQTransform") and hasattr(net.CQTransform, "plan"):
        msg = ("loading trained weights into the MI355X network while its CQT is NOT pinned to cqt_nsgt_pytorch "
               f"(rules {net.CQTransform.plan.rules}): outputs are not comparable with the reference until "
               "tools/pin_external.sh (tests/golden/make_cqt_golden.py + tests/test_cqt_conformance.py) has been run where the package is installed")
        if not allow_unpinned_cqt:
            raise UnpinnedCQTError(msg + "; pass allow_unpinned_cqt=True to load anyway")
        warnings.warn(msg, RuntimeWarning, stacklevel=2)
    if isinstance(state, (str, bytes)) or hasattr(state, "__fspath__"):
        state = torch.load(state, map_location="cpu")
    it = int(state["it"]) if "it" in state else 0
    sd = state[key]
    try:
        net.load_state_dict(sd)                                      # attempt 1 (:229-236)
        return it, "strict"
    except Exception:
        pass
    try:
        net.load_state_dict(sd, strict=False)                        # attempt 2 (:242-249): missing / unexpected keys tolerated
        return it, "non-strict"
    except Exception:
        pass
    own = net.state_dict()                                           # attempt 3 (:256-283): copy what matches by name and shape
    n = 0
    for name, param in sd.items():
        if name in own and own[name].shape == param.shape:
            own[name] = param
            n += 1
    if n == 0:
        raise ValueError("No parameters were loaded")
    net.load_state_dict(own)
    return it, "shape-matched"


def centre_gap_window(length: int, audio_len: int, gap: int) -> Tuple[int, int]:
    """(start of the gap, start of the audio_len window) for a file of ``length`` samples (:399-411)."""
    if length < audio_len:
        raise ValueError(f"file shorter ({length}) than the model's segment length ({audio_len})")
    return int(length // 2 - gap // 2), int(length // 2 - audio_len // 2)


def inpaint_long(sampler, files: Sequence[torch.Tensor], gap_ms: float, sample_rate: float, audio_len: int,
                 device="cuda") -> List[torch.Tensor]:
    """Inpaint a centred gap of ``gap_ms`` in every 1-D waveform of ``files`` (any lengths >= audio_len) and return the
    full-length results.  One sampler call for the whole batch."""
    gap = int(gap_ms * sample_rate / 1000)
    segs, masks, where = [], [], []
    for x in files:
        x = x.reshape(-1).float()
        g0, s0 = centre_gap_window(x.numel(), audio_len, gap)
        m = torch.ones(x.numel())
        m[g0:g0 + gap] = 0
        segs.append(x[s0:s0 + audio_len])
        masks.append(m[s0:s0 + audio_len])
        where.append(s0)
    seg, mask = torch.stack(segs).to(device), torch.stack(masks).to(device)
    pred = sampler.predict_inpainting(seg * mask, mask).cpu()
    out = []
    for x, s0, p in zip(files, where, pred):
        x = x.reshape(-1).float()
        out.append(torch.cat((x[:s0], p, x[s0 + audio_len:])))       # (:415)
    return out


def generate_long(sampler, n_items: int, n_windows: int, seeds: Optional[Sequence[int]] = None, max_batch: int = 8,
                  device="cuda") -> torch.Tensor:
    """Generate ``n_items`` independent pieces of ``n_windows`` overlapping windows each (Sampler.predict_autoregressive; the counterpart of
    inpaint_long for producing audio longer than one model segment) -> [n_items, L + (n_windows - 1) * (L - end)] on ``device``.
    The items run in sub-batches of at most ``max_batch``; with an active process group every rank generates dist.shard_range of them and
    one dist.gather_outputs collects the result, as the inpainting path shards segments.  ``seeds``: one RNG seed per item (item i's piece
    then depends on seeds[i] alone, not on the grouping); None: dist.item_seeds(0, ...) under a process group, else the global generator."""
    from . import dist as D
    if n_items < 1 or max_batch < 1:
        raise ValueError("generate_long: n_items and max_batch must be >= 1")
    if seeds is not None and len(seeds) != n_items:
        raise ValueError(f"generate_long: {len(seeds)} seeds for {n_items} items")
    active = D._active()
    rank, world = (torch.distributed.get_rank(), torch.distributed.get_world_size()) if active else (0, 1)
    lo, hi = D.shard_range(n_items, rank, world)
    if seeds is None and active:
        seeds = D.item_seeds(0, 0, n_items)
    L = int(sampler.args.exp.audio_len)
    keep, parts = sampler.seeds, []
    try:
        for b0 in range(lo, hi, max_batch):
            b1 = min(hi, b0 + max_batch)
            sampler.seeds = None if seeds is None else [int(s) for s in seeds[b0:b1]]
            parts.append(sampler.predict_autoregressive((b1 - b0, L), n_windows, device))
    finally:
        sampler.seeds = keep
    if len(parts) == 1:
        local = parts[0]
    elif parts:
        local = torch.cat(parts, dim=0)
    else:                                                            # (a rank without items still takes part in the collective)
        from .sampler import autoregressive_length, autoregressive_overlap
        local = torch.zeros((0, autoregressive_length(L, int(autoregressive_overlap(sampler.args) * L), n_windows)), device=device)
    return D.gather_outputs(local, n_items)


class _LongMode(NamedTuple):
    """One whole-recording mode as ``_long_groups`` drives it, plainly and pooled."""
    method: str                                      # the sampler method, e.g. "predict_bwe_long"
    task: Optional[str]                              # the task of Sampler.predict_long_pooled; None: the mode does not pool
    key: Callable                                    # key(i): the files with equal keys are stacked into one call
    group_of: Callable = lambda y, idx, key: ()      # group_of(y, idx, key) -> the entries of the stack after y, in the order of the method's parameters
    shared: dict = {}                                # the arguments all files share, by name, in the order of the method's parameters after y


def _long_groups(who: str, sampler, files, seeds, max_batch, device, mode: _LongMode, pool: bool = False, flat: bool = True, after=None) -> List[torch.Tensor]:
    """What the *_long functions below are: every file of ``files`` (any lengths) goes through ``mode`` and the full-length results come
    back on ``device``, in the order of ``files``.
    GROUPING.  The files with equal ``mode.key(i)`` (the length, mostly) are stacked on ``device`` (``flat``: each as a 1-D waveform) and go
    through ONE call of the sampler method, ``method(y, *shared, *entries, max_batch, seeds)``, so their windows share the two batched passes;
    every other key is a call of its own (``after(idx)`` follows each).
    SEEDS.  One RNG seed per file: file i's result then depends on seeds[i] alone, not on the grouping.
    PROCESS GROUPS.  Under an active process group (dist.init_distributed; weights made equal with dist.broadcast_parameters first) every
    rank passes the same files and gets the full results: the windows of each pass are shared out over the ranks and exchanged once per
    pass (restore.run_pooled_passes), ``max_batch`` is per rank, and ``seeds`` = None means dist.item_seeds(0, 0, len(files)), as in
    generate_long: a file's result must not depend on the world size.
    POOL.  ``pool`` = True: all stacks go through ONE Sampler.predict_long_pooled(mode.task, [(y, *entries), ...], the seeds in that
    order, **shared), where the windows of ALL files, whatever their lengths, share the two batched passes: a chunk of ``max_batch``
    windows may span files, so a folder of short files of different lengths runs full batches; with seeds the results are those of
    ``pool`` = False."""
    from . import dist as D
    if seeds is not None and len(seeds) != len(files):
        raise ValueError(f"{who}: {len(seeds)} seeds for {len(files)} files")
    if seeds is None and D._active():
        seeds = D.item_seeds(0, 0, len(files))
    groups = {}
    for i in range(len(files)):
        groups.setdefault(mode.key(i), []).append(i)
    seeds_of = lambda idx: None if seeds is None else [int(seeds[i]) for i in idx]                                        # noqa: E731
    stacks = ((torch.stack([(files[i].reshape(-1) if flat else files[i]).float() for i in idx]).to(device), idx, k) for k, idx in groups.items())
    if pool:
        every = sampler.predict_long_pooled(mode.task, [(y, *mode.group_of(y, idx, k)) for y, idx, k in stacks], max_batch=max_batch,
                                            seeds=seeds_of([i for idx in groups.values() for i in idx]), **mode.shared)
    else:
        every = []
        for y, idx, k in stacks:
            every.append(getattr(sampler, mode.method)(y, *mode.shared.values(), *mode.group_of(y, idx, k), max_batch=max_batch, seeds=seeds_of(idx)))
            if after is not None:
                after(idx)
    out: List[Optional[torch.Tensor]] = [None] * len(files)
    for res, idx in zip(every, groups.values()):
        for j, i in enumerate(idx):
            out[i] = res[j]
    return out


def _levels_per_file(who: str, clip_values, n_files: int) -> List[float]:
    """one float for all files, or one per file -> one per file"""
    levels = [float(v) for v in (clip_values.reshape(-1).tolist() if torch.is_tensor(clip_values) else
                                 (list(clip_values) if hasattr(clip_values, "__len__") else [clip_values]))]
    if len(levels) not in (1, n_files):
        raise ValueError(f"{who}: {len(levels)} clip values for {n_files} files")
    return levels * n_files if len(levels) == 1 else levels


def restore_long(sampler, files: Sequence[torch.Tensor], masks: Sequence[torch.Tensor], seeds: Optional[Sequence[int]] = None, max_batch: int = 8,
                 device="cuda", pool: bool = False) -> List[torch.Tensor]:
    """Restore every 1-D waveform of ``files`` (any lengths) where its mask (same length; 1 = observed, 0 = gap, gaps anywhere) is 0 and return the
    full-length results on ``device``, in the order of ``files``.  Files of equal length go through ONE Sampler.predict_inpainting_long call.
    Grouping, seeds, process groups and ``pool`` as ``_long_groups`` states (the pooled task is "inpainting")."""
    if len(masks) != len(files):
        raise ValueError(f"restore_long: {len(masks)} masks for {len(files)} files")

    def key(i):
        if files[i].numel() != masks[i].numel():
            raise ValueError(f"restore_long: file {i} has {files[i].numel()} samples, its mask {masks[i].numel()}")
        return files[i].numel()
    mode = _LongMode("predict_inpainting_long", "inpainting", key, lambda y, idx, k: (torch.stack([masks[i].reshape(-1).float() for i in idx]),))
    return _long_groups("restore_long", sampler, files, seeds, max_batch, device, mode, pool)


def declick_detect(files: Sequence[torch.Tensor], device="cuda", masks: Optional[Sequence[Optional[torch.Tensor]]] = None, settings=None):
    """(masks, reports) of declick.detect over 1-D waveforms of any lengths: the files of equal length are stacked for ONE detect call.
    masks[i] [N_i] on ``device`` is the detected mask times ``masks[i]`` (known gaps, 1 = observed) where one is given; reports[i] is the
    file's declick.Detection -- that mask and ITS counts (known gaps included), the detector's sigma [J_i], no score plane.  A file of which more than
    ``max_fraction`` is masked is refused, by its index.  Needs no model."""
    from . import declick
    cfg = declick.make_settings(**dict(settings or {}))
    if masks is not None and len(masks) != len(files):
        raise ValueError(f"declick_long: {len(masks)} masks for {len(files)} files")
    groups = {}
    for i, f in enumerate(files):
        groups.setdefault(f.numel(), []).append(i)
    out, reports = [None] * len(files), [None] * len(files)
    for n, idx in groups.items():
        det = declick.detect(torch.stack([files[i].reshape(-1).float() for i in idx]).to(device), **cfg._asdict())
        for j, i in enumerate(idx):
            counts = det.n_flagged[j], det.n_gaps[j], det.longest_gap[j]
            m = det.mask[j]
            if masks is not None and masks[i] is not None:                   # (the report describes the mask that is restored)
                m = declick.combine(det.mask[j:j + 1], masks[i].reshape(-1))[0]
                counts = tuple(c[0] for c in declick.report_of(m))
            out[i] = m
            reports[i] = declick.Detection(m, None, det.sigma[j], *counts)
    declick.check_fraction([int(r.n_flagged) for r in reports], [f.numel() for f in files], cfg.max_fraction, "file")
    return out, reports


def declick_long(sampler, files: Sequence[torch.Tensor], seeds: Optional[Sequence[int]] = None, max_batch: int = 8, device="cuda", pool: bool = False,
                 masks: Optional[Sequence[Optional[torch.Tensor]]] = None, **settings):
    """Declick every 1-D waveform of ``files`` (any lengths): ``declick_detect`` finds the clicks and dropouts (settings:
    declick.settings_of(sampler.args), overridden by ``settings``; ``masks``: known gaps per file, or None), then
    restore_long(sampler, files, the detected masks, seeds, max_batch, device, pool) restores them, so grouping, seeds, process groups and
    ``pool`` are restore_long's (the pooled task is "inpainting").  -> (the full-length results on ``device``, the reports of declick_detect),
    both in the order of ``files``."""
    from . import declick
    detected, reports = declick_detect(files, device, masks, declick.settings_of(sampler.args, **settings)._asdict())
    return restore_long(sampler, files, detected, seeds, max_batch, device, pool), reports


def declip_long(sampler, files: Sequence[torch.Tensor], clip_values, seeds: Optional[Sequence[int]] = None, max_batch: int = 8,
                device="cuda", pool: bool = False) -> List[torch.Tensor]:
    """Declip every 1-D waveform of ``files`` (any lengths), clipped at +-clip_values (one float for all files, or one per file), and return the
    full-length results on ``device``, in the order of ``files``.  Files of equal length go through ONE Sampler.predict_declipping_long call.
    Grouping, seeds, process groups and ``pool`` as ``_long_groups`` states (the pooled task is "declipping")."""
    levels = _levels_per_file("declip_long", clip_values, len(files))
    mode = _LongMode("predict_declipping_long", "declipping", lambda i: files[i].numel(), lambda y, idx, k: ([levels[i] for i in idx],))
    return _long_groups("declip_long", sampler, files, seeds, max_batch, device, mode, pool)


def bwe_long(sampler, files: Sequence[torch.Tensor], filt, filt_type: str = "firwin", seeds: Optional[Sequence[int]] = None, max_batch: int = 8,
             device="cuda", pool: bool = False) -> List[torch.Tensor]:
    """Bandwidth-extend every 1-D waveform of ``files`` (any lengths), each low-passed as a whole with the FIR taps ``filt`` (one filter for all
    files), and return the full-length results on ``device``, in the order of ``files``.  Files of equal length go through ONE
    Sampler.predict_bwe_long call.  Grouping, seeds, process groups and ``pool`` as ``_long_groups`` states (the pooled task is "bwe")."""
    mode = _LongMode("predict_bwe_long", "bwe", lambda i: files[i].numel(), shared=dict(filt=filt, filt_type=filt_type))
    return _long_groups("bwe_long", sampler, files, seeds, max_batch, device, mode, pool)


def blind_bwe_long(sampler, files: Sequence[torch.Tensor], probes: int = 4, seeds: Optional[Sequence[int]] = None, max_batch: int = 8,
                   device="cuda") -> List[torch.Tensor]:
    """Bandwidth-extend every 1-D waveform of ``files`` (any lengths), each low-passed as a whole by an unknown low-pass of its own, and return
    the full-length results on ``device``, in the order of ``files``.  Files of equal length go through ONE Sampler.predict_blind_bwe_long
    call: their probe windows share the chunks of stage 1 and their windows the two batched passes of stage 2; every other length is a call
    of its own -- there is no ``pool`` argument.  Afterwards ``sampler.blind_fit`` [len(files), 2], ``sampler.blind_taps`` [len(files), K] and
    ``sampler.blind_probes`` hold every file's filter, in the order of ``files``.  Grouping, seeds (file i's filter, too, depends on seeds[i]
    alone) and process groups as ``_long_groups`` states."""
    held = {}

    def after(idx):
        for j, i in enumerate(idx):
            held[i] = (sampler.blind_fit[j], sampler.blind_taps[j], sampler.blind_probes[j])
    mode = _LongMode("predict_blind_bwe_long", None, lambda i: files[i].numel(), shared=dict(probes=probes))
    out = _long_groups("blind_bwe_long", sampler, files, seeds, max_batch, device, mode, after=after)
    if held:
        sampler.blind_fit = torch.stack([held[i][0] for i in range(len(files))])
        sampler.blind_taps = torch.stack([held[i][1] for i in range(len(files))])
        sampler.blind_probes = [held[i][2] for i in range(len(files))]
    return out


def bwe_iir_long(sampler, files: Sequence[torch.Tensor], filt, filt_type: str = "cheby1", seeds: Optional[Sequence[int]] = None, max_batch: int = 8,
                 device="cuda", pool: bool = False) -> List[torch.Tensor]:
    """Bandwidth-extend every 1-D waveform of ``files`` (any lengths), each low-passed as a whole with the IIR filter ``filt`` ("cheby1": (b, a);
    "biquad": (b0, b1, b2, a0, a1, a2); one filter for all files), and return the full-length results on ``device``, in the order of ``files``.
    Files of equal length go through ONE Sampler.predict_bwe_iir_long call.  Grouping, seeds, process groups and ``pool`` as ``_long_groups``
    states (the pooled task is "bwe_iir")."""
    mode = _LongMode("predict_bwe_iir_long", "bwe_iir", lambda i: files[i].numel(), shared=dict(filt=filt, filt_type=filt_type))
    return _long_groups("bwe_iir_long", sampler, files, seeds, max_batch, device, mode, pool)


def bwe_declip_long(sampler, files: Sequence[torch.Tensor], filt, filt_type: str = "firwin", clip_values=None, masks: Optional[Sequence[Optional[torch.Tensor]]] = None,
                    seeds: Optional[Sequence[int]] = None, max_batch: int = 8, device="cuda", pool: bool = False) -> List[torch.Tensor]:
    """Bandwidth-extend every 1-D waveform of ``files`` (any lengths) that was low-passed as a whole with the FIR taps ``filt`` (one filter for
    all files), THEN clipped at +-clip_values (None: not clipped; one float for all files, or one per file) and THEN dropped where its mask
    (``masks``: None, or per file None or a mask of the file's length; 1 = kept, 0 = dropped) is 0 -- y = mask * clamp(taps * x, -c, c), in this
    order -- and return the full-length results on ``device``, in the order of ``files``.  Files of equal length go through ONE
    Sampler.predict_bwe_declip_long call (a file without a mask gets all ones beside one that has one).  Grouping, seeds, process groups and
    ``pool`` as ``_long_groups`` states (the pooled task is "bwe_declip")."""
    levels = None if clip_values is None else _levels_per_file("bwe_declip_long", clip_values, len(files))
    if masks is not None and len(masks) != len(files):
        raise ValueError(f"bwe_declip_long: {len(masks)} masks for {len(files)} files")

    def key(i):
        if masks is not None and masks[i] is not None and masks[i].numel() != files[i].numel():
            raise ValueError(f"bwe_declip_long: file {i} has {files[i].numel()} samples, its mask {masks[i].numel()}")
        return files[i].numel()

    def mask_of(idx):
        if masks is None or all(masks[i] is None for i in idx):
            return None
        return torch.stack([torch.ones(files[i].numel()) if masks[i] is None else masks[i].reshape(-1).float().cpu() for i in idx])
    mode = _LongMode("predict_bwe_declip_long", "bwe_declip", key, lambda y, idx, k: (None if levels is None else [levels[i] for i in idx], mask_of(idx)),
                     dict(filt=filt, filt_type=filt_type))
    return _long_groups("bwe_declip_long", sampler, files, seeds, max_batch, device, mode, pool)


def bwe_lowrate_long(sampler, files: Sequence[torch.Tensor], factor, filt_type: str = "resample", lengths: Optional[Sequence[Optional[int]]] = None,
                     seeds: Optional[Sequence[int]] = None, max_batch: int = 8, device="cuda", pool: bool = False) -> List[torch.Tensor]:
    """Bandwidth-extend every 1-D low-sample-rate waveform of ``files`` (any lengths; one ``factor`` and ``filt_type`` for all files) and return the
    high-rate results on ``device``, in the order of ``files``.  ``lengths``: the number of high-rate samples per file (None, for all files or for
    one: the largest consistent with the file).  Files of equal (low-rate length, length) go through ONE Sampler.predict_bwe_lowrate_long call.
    Grouping, seeds, process groups and ``pool`` as ``_long_groups`` states (the pooled task is "bwe_lowrate")."""
    if lengths is not None and len(lengths) != len(files):
        raise ValueError(f"bwe_lowrate_long: {len(lengths)} lengths for {len(files)} files")
    mode = _LongMode("predict_bwe_lowrate_long", "bwe_lowrate", lambda i: (files[i].numel(), None if lengths is None or lengths[i] is None else int(lengths[i])),
                     lambda y, idx, k: (k[1],), dict(factor=factor, filt_type=filt_type))
    return _long_groups("bwe_lowrate_long", sampler, files, seeds, max_batch, device, mode, pool)


def pr_long(sampler, spectrograms: Sequence[torch.Tensor], lengths: Optional[Sequence[Optional[int]]] = None, seeds: Optional[Sequence[int]] = None,
            max_batch: int = 8, device="cuda", pool: bool = False) -> List[torch.Tensor]:
    """Retrieve the phase of every 2-D magnitude spectrogram [F, T_rec] of ``spectrograms`` (any numbers of frames) and return the waveforms on
    ``device``, in the order of ``spectrograms``.  ``lengths``: the number of samples per file (None, for all files or for one: the largest
    consistent with the file's frames).  Files of equal (T_rec, length) go through ONE Sampler.predict_pr_long call.  Grouping, seeds,
    process groups and ``pool`` as ``_long_groups`` states (the pooled task is "pr")."""
    if lengths is not None and len(lengths) != len(spectrograms):
        raise ValueError(f"pr_long: {len(lengths)} lengths for {len(spectrograms)} files")

    def key(i):
        if spectrograms[i].dim() != 2:
            raise ValueError(f"pr_long: file {i} must be a magnitude spectrogram [F, T_rec], got {tuple(spectrograms[i].shape)}")
        return tuple(spectrograms[i].shape), None if lengths is None or lengths[i] is None else int(lengths[i])
    mode = _LongMode("predict_pr_long", "pr", key, lambda y, idx, k: (k[1],))
    return _long_groups("pr_long", sampler, spectrograms, seeds, max_batch, device, mode, pool, flat=False)


def spectrogram_inpainting_long(sampler, files: Sequence[torch.Tensor], masks: Sequence[torch.Tensor], seeds: Optional[Sequence[int]] = None,
                                max_batch: int = 8, device="cuda", pool: bool = False) -> List[torch.Tensor]:
    """Restore every waveform of ``files`` (any lengths; each masked as a whole in the STFT domain) under its mask [F, T_rec] of ``masks``
    (masks.spectral_mask(audio_len=len(file), ...)) and return the waveforms on ``device``, in the order of ``files``.  Files of equal length
    go through ONE Sampler.predict_spectrogram_inpainting_long call.  Grouping, seeds and process groups as ``_long_groups`` states.
    ``pool`` = True is refused: aid_stft_mask_observed reads one recording-shaped mask in place, so the windows of files with different
    T_rec cannot share a launch (Sampler.predict_long_pooled says the same)."""
    if pool:
        return sampler.predict_long_pooled("spectrogram_inpainting", [])                   # (raises, with the reason)
    if len(masks) != len(files):
        raise ValueError(f"spectrogram_inpainting_long: {len(masks)} masks for {len(files)} files")

    def key(i):
        if masks[i].dim() != 2:
            raise ValueError(f"spectrogram_inpainting_long: mask {i} must be [F, T_rec], got {tuple(masks[i].shape)}")
        return files[i].numel(), tuple(masks[i].shape)
    mode = _LongMode("predict_spectrogram_inpainting_long", None, key, lambda y, idx, k: (torch.stack([masks[i].float() for i in idx]).to(device),))
    return _long_groups("spectrogram_inpainting_long", sampler, files, seeds, max_batch, device, mode)


def evaluate_long(refs: Sequence[torch.Tensor], ests: Sequence[torch.Tensor], regions: Optional[Sequence[Optional[torch.Tensor]]] = None,
                  device="cuda", evaluate=None, **metric_args):
    """Objective metrics (metrics.py) of every restored 1-D waveform of ``ests`` against the waveform of ``refs`` at the same place, any lengths:
    ``regions[i]`` (same length, non-zero = evaluate here; None = everywhere) is what file i is judged on, ``metric_args`` go to
    metrics.evaluate (sample_rate=, n_fft=, hop=, band=, floor=).  Files of equal length are stacked and go through ONE metrics.evaluate call
    (two launches, one read-back); every other length is a call of its own.  Returns (rows, summary):
    rows: one dict per file, in the order of the input: index, n (its length) and a float per metric (lsd, snr_db, si_sdr_db, max_abs_err,
          n_samples, n_frames);
    summary: per metric of metrics.METRICS the mean and the median over the files where it is finite, and how many were not
             (n_not_finite), plus n_files.
    ``evaluate``: the function called per length in place of metrics.evaluate (tests)."""
    from . import metrics
    import math
    evaluate = metrics.evaluate if evaluate is None else evaluate
    if len(ests) != len(refs) or (regions is not None and len(regions) != len(refs)):
        raise ValueError(f"evaluate_long: {len(refs)} references, {len(ests)} estimates" + ("" if regions is None else f", {len(regions)} regions"))
    for i in range(len(refs)):
        if ests[i].numel() != refs[i].numel() or (regions is not None and regions[i] is not None and regions[i].numel() != refs[i].numel()):
            raise ValueError(f"evaluate_long: file {i} has {refs[i].numel()} reference samples, {ests[i].numel()} estimated ones" +
                             ("" if regions is None or regions[i] is None else f" and a region of {regions[i].numel()}"))
    names = ("lsd", "snr_db", "si_sdr_db", "max_abs_err", "n_samples", "n_frames")

    def call(r, idx, n, max_batch, seeds):
        e = torch.stack([ests[i].reshape(-1).float() for i in idx]).to(device)
        w = None
        if regions is not None and any(regions[i] is not None for i in idx):
            w = torch.stack([torch.ones(n) if regions[i] is None else (regions[i].reshape(-1) != 0).float().cpu() for i in idx]).to(device)
        res = evaluate(r, e, w, **metric_args)
        return [dict({"index": i, "n": n}, **{k: float(res[k][j]) for k in names}) for j, i in enumerate(idx)]
    # (nothing here draws random numbers: the placeholder seeds keep _long_groups from asking a process group for some)
    mode = _LongMode("evaluate", None, lambda i: refs[i].numel(), lambda r, idx, n: (idx, n))
    rows = _long_groups("evaluate_long", types.SimpleNamespace(evaluate=call), refs, [0] * len(refs), None, device, mode)
    summary = {"n_files": len(rows)}
    for k in metrics.METRICS:
        v = sorted(row[k] for row in rows if math.isfinite(row[k]))
        mid = len(v) // 2
        summary[k] = {"mean": sum(v) / len(v) if v else float("nan"),
                      "median": (v[mid] if len(v) % 2 else (v[mid - 1] + v[mid]) / 2) if v else float("nan"),
                      "n_not_finite": len(rows) - len(v)}
    return rows, summary


# ---- waveform pre-/post-processing of the tester --------------------------------------------------------------------------------
# (torchaudio's default resampling kernel: one builder and one table cache, in degrade.py, serve this module and degrade.SincResample)
from .degrade import sinc_kernel as _sinc_kernel  # noqa: E402


def resample(x: torch.Tensor, orig_freq: int, new_freq: int) -> torch.Tensor:
    """x [B, L] on the GPU -> [B, ceil(new*L/orig)]   (aid_resample_poly; replaces torchaudio.functional.resample)"""
    import math
    from . import _lib
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    if o == n:
        return x
    if not x.is_cuda:
        raise _lib.AidError("harness.resample runs on the GPU only (no CPU fallback)")
    from .degrade import resample_poly
    return resample_poly(x.contiguous().float(), o, n)


def _resample_one_rate(audio, f: int, fs_target: int, length_target: int) -> torch.Tensor:
    if fs_target == 22050 and f == 44100:
        return resample(audio, 2, 1)[:, :length_target]
    if fs_target == 22050 and f == 48000:
        return resample(audio, 160 * 2, 147)[:, :length_target]            # the reference's approximation of 48k -> 22.05k (:152)
    if fs_target == 44100 and f == 44100:
        return audio[:, :length_target]
    if fs_target == 44100 and f == 48000:
        return resample(audio, 160, 147)[:, :length_target]
    if f in (44100, 48000):                                                # (:191-196: any other target, from the two rates the datasets have)
        return resample(audio, f, fs_target)[:, :length_target]
    # any other source rate: the reference's `(fs == 44100).all()` / `(fs == 48000).all()` tests fail, its per-item loop prints "WARNING, strange fs" and
    # passes the row through UNRESAMPLED (:165, :186, :207) -- the same rule whether the whole batch or only some rows have that rate
    import warnings
    warnings.warn(f"resample_batch: strange fs {f}: rows passed through unresampled, as the reference does (call harness.resample(x, {f}, {fs_target}) to resample them)")
    return audio[:, :length_target].float()


def resample_batch(audio: torch.Tensor, fs, fs_target: int, length_target: int) -> torch.Tensor:
    """resample_batch (utils/training_utils.py:140-212).  ``fs``: scalar or [B] tensor.  One rate for the whole batch: one batched polyphase launch.
    Mixed rates (the reference's per-item loops, :156-167 / :177-188 / :199-210): one launch per distinct rate, rows written in place -- the reference's
    loops ``return`` inside their first iteration, so only ITEM 0 of its result is filled; item 0 here equals it, the other items are resampled too."""
    f = fs.reshape(-1) if torch.is_tensor(fs) else torch.tensor([fs])
    if bool((f == f[0]).all()):
        y = _resample_one_rate(audio, int(f[0]), fs_target, length_target)
        if y.shape[1] < length_target and int(f[0]) not in (44100, 48000):
            raise ValueError(f"resample_batch: rows at {int(f[0])} Hz passed through give {y.shape[1]} samples, fewer than length_target = {length_target}")
        return y
    if f.numel() != audio.shape[0]:
        raise ValueError(f"fs has {f.numel()} entries for a batch of {audio.shape[0]}")
    out = torch.zeros(audio.shape[0], length_target, device=audio.device, dtype=torch.float32)
    for rate in sorted(set(int(v) for v in f.tolist())):
        rows = torch.nonzero(f.cpu() == rate).reshape(-1).to(audio.device)
        sub = audio.index_select(0, rows)
        y = _resample_one_rate(sub, rate, fs_target, length_target)      # (rates other than 44100 / 48000 pass through with a warning, like the reference)
        if y.shape[1] < length_target:                         # the reference's ``proc_batch[i] = a[0:length_target]`` raises on a short row: no silent zero padding
            raise ValueError(f"resample_batch: rows at {rate} Hz give {y.shape[1]} samples at {fs_target} Hz, fewer than length_target = {length_target}")
        out[rows] = y
    return out


def write_audio_file(x: torch.Tensor, sr: int, string: str, path: str = "tmp") -> str:
    """utils/logging.py:295-319 (mono branch): flatten, rescale when max(x) >= 1, 16-bit PCM wav (soundfile's default subtype for
    .wav; written with the standard library, soundfile is not a dependency here)."""
    import os
    import wave
    import numpy as np
    os.makedirs(path, exist_ok=True)
    fn = os.path.join(path, string + ".wav")
    a = x.detach().flatten().cpu().numpy().astype(np.float64)
    if np.abs(np.max(a)) >= 1:
        a = a / np.abs(np.max(a))                                       # (sic: max, not max-abs -- as the reference)
    pcm = np.clip(np.rint(a * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(fn, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(sr))
        w.writeframes(pcm.tobytes())
    return fn


def read_wav(fn: str):
    """(waveform float32 [1, L] in [-1, 1), sampling rate) of a 16-bit PCM mono wav"""
    import wave
    import numpy as np
    with wave.open(fn, "rb") as w:
        assert w.getsampwidth() == 2 and w.getnchannels() == 1
        sr, n = w.getframerate(), w.getnframes()
        a = np.frombuffer(w.readframes(n), dtype="<i2").astype(np.float32) / 32768.0
    return torch.from_numpy(a).reshape(1, -1), sr
