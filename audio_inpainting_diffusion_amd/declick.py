"""Declicking: find the clicks and the short dropouts of a recording on the GPU and hand them, as a mask, to the inpainter
(include/aid_bwe_long.h: aid_ar_score, aid_click_mask; csrc/aid_declick.hip).  A front end of the "inpainting" task, not a task of its own:
``Sampler.predict_declicking_long`` detects and then calls ``predict_inpainting_long``.

THE SETTINGS (``make_settings``; ``settings_of(args)`` reads args.tester.declicking):
    block 2048 (256, 512, 1024, 2048 or 4096)    order 16 (1 .. 32, 8 order <= block)    threshold 8 (> 0)    pad 16 (0 .. 256)
    min_run 8 (0 = no run rule, otherwise 2 .. max_run)    max_run 1024 (1 .. 1024)    ridge 1e-6 (>= 0)    sigma_floor 1e-6 (> 0)
    max_fraction 0.2 (0 .. 1)
threshold, ridge and sigma_floor are rounded to float32 once, here: they reach the kernels as floats, and the restatements read the same values.

THE SCORE, per recording row.  Block j holds the n samples [j block, min(N, (j + 1) block)).  With n < 8 order it is not scored: score 0.
Otherwise, with x the block's samples in float64:  r[m] = sum_{i = m}^{n - 1} x[i] x[i - m], m = 0 .. order;  r[0] *= 1 + ridge;  r[0] <= 0:
not scored.  Levinson-Durbin on r gives a[1 .. order], a[0] = 1; it stops, the remaining coefficients 0, once the error power is <= 0.
e[q] = sum_{k = 0}^{order} a[k] y[q - k] over the RECORDING's samples (the previous block's where q - k falls there; 0 before the first
sample).  Every sample of the block is scored but the first ``order`` of the recording (the model has nothing to predict them from: they score
up to 51 on a clean signal whose other samples stay below 4.1).  sigma = max(median / 0.6745, sigma_floor), the median being the element of
rank n' // 2 (0-based) of |e| over the n' scored samples in ascending order.  score = |e| / sigma as float32; 0 where not scored.

THE FLAGS.  A sample is flagged when its score is > threshold (float32 against float32), or, with min_run > 0, when it lies in a maximal run
of bit-identical samples of length l, min_run <= l <= max_run, that holds neither the first nor the last sample of the recording (a longer
run is digital silence, and so is one at either end: not a dropout).

THE MASK.  mask[q] = 0 when a sample of [q - pad, q + pad] within [0, N) is flagged, 1 otherwise: 1 = observed, 0 = restore, as
predict_inpainting_long reads it.  THE REPORT, per recording, from one read-back of the mask: n_flagged (its zeros), n_gaps (their maximal
runs), longest_gap.

``score_host`` / ``mask_host`` / ``detect_host`` state this in float64 numpy.  They are the definition -- the project this one follows has no
detector -- and what the kernels are tested against: the mask bit for bit, the score up to what the order of the autocorrelation sums moves
(the kernel adds 256 strided partial sums as a tree, ``score_host`` adds forward; ``autocorr="pairwise"`` is the second order that measures
the distance between two such evaluations).  ``score`` / ``mask`` / ``detect`` are the launches: GPU only, no fallback.

To judge a restoration of the detected gaps, ``metrics.region_of("inpainting", mask=report.mask)`` is the region.

Not covered: restoration quality (it needs trained weights), sample rates other than the 22.05 kHz the defaults were chosen at, damage that
is not impulsive (crackle so dense that it moves the median, hum, wow).
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib

BLOCKS = (256, 512, 1024, 2048, 4096)
MAX_ORDER, MAX_PAD, MAX_RUN, MAX_ROWS = 32, 256, 1024, 65535
NAMES = ("block", "order", "threshold", "pad", "min_run", "max_run", "ridge", "sigma_floor", "max_fraction")


class Settings(NamedTuple):
    block: int = 2048
    order: int = 16
    threshold: float = 8.0
    pad: int = 16
    min_run: int = 8
    max_run: int = 1024
    ridge: float = float(np.float32(1e-6))
    sigma_floor: float = float(np.float32(1e-6))
    max_fraction: float = 0.2

    @property
    def score_args(self) -> dict:
        return dict(block=self.block, order=self.order, ridge=self.ridge, sigma_floor=self.sigma_floor)

    @property
    def mask_args(self) -> dict:
        return dict(threshold=self.threshold, pad=self.pad, min_run=self.min_run, max_run=self.max_run)


class Detection(NamedTuple):
    mask: object                 # [R, N] float32, 1 = observed, 0 = restore
    score: object                # [R, N] float32 (None in Sampler.declick_report)
    sigma: object                # [R, J] the scale of every block, 0 where the block was not scored
    n_flagged: object            # [R] int64 on the host: the zeros of the mask
    n_gaps: object               # [R] the maximal runs of zeros
    longest_gap: object          # [R]


# ---- settings and their refusals (no GPU needed) -------------------------------------------------------------------------------------------
def _whole(name, v, lo, hi, extra=""):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer, float)) or int(v) != v or not lo <= int(v) <= hi:
        raise _lib.AidError(f"declicking: {name} must be a whole number in [{lo}, {hi}]{extra}, got {v!r}")
    return int(v)


def _number(name, v, ok, what):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or not ok(float(v)):
        raise _lib.AidError(f"declicking: {name} must be a finite number {what}, got {v!r}")
    return float(v)


def make_settings(**kw) -> Settings:
    """The settings after every refusal, by name; what is not given is the default."""
    unknown = sorted(set(kw) - set(NAMES))
    if unknown:
        raise _lib.AidError(f"declicking: unknown setting {', '.join(unknown)} (the settings are {', '.join(NAMES)})")
    s = Settings()._asdict()
    s.update(kw)
    if isinstance(s["block"], bool) or s["block"] not in BLOCKS:
        raise _lib.AidError(f"declicking: block must be one of {BLOCKS}, got {s['block']!r}")
    block = int(s["block"])
    order = _whole("order", s["order"], 1, MAX_ORDER)
    if 8 * order > block:
        raise _lib.AidError(f"declicking: order = {order} needs 8 * order <= block = {block}")
    f32 = lambda v: float(np.float32(v))                                                                                  # noqa: E731
    threshold = f32(_number("threshold", s["threshold"], lambda v: v > 0 and f32(v) > 0 and math.isfinite(f32(v)), "> 0"))
    pad = _whole("pad", s["pad"], 0, MAX_PAD)
    max_run = _whole("max_run", s["max_run"], 1, MAX_RUN)
    min_run = _whole("min_run", s["min_run"], 0, max_run, " (0 = no run rule; at most max_run)")
    if min_run == 1:
        raise _lib.AidError("declicking: min_run must be 0 (no run rule) or at least 2: every sample is a run of 1")
    ridge = f32(_number("ridge", s["ridge"], lambda v: v >= 0 and math.isfinite(f32(v)), ">= 0"))
    sigma_floor = f32(_number("sigma_floor", s["sigma_floor"], lambda v: v > 0 and f32(v) > 0 and math.isfinite(f32(v)), "> 0"))
    max_fraction = _number("max_fraction", s["max_fraction"], lambda v: 0 <= v <= 1, "in [0, 1]")
    return Settings(block, order, threshold, pad, min_run, max_run, ridge, sigma_floor, max_fraction)


def settings_of(args, **override) -> Settings:
    """args.tester.declicking when the config has it (any of ``NAMES``), the defaults for the rest; ``override`` wins over both"""
    node = getattr(getattr(args, "tester", None), "declicking", None)
    kw = {} if node is None else {k: node[k] for k in NAMES if k in node and node[k] is not None}
    kw.update(override)
    return make_settings(**kw)


# ---- the float64 restatements ----------------------------------------------------------------------------------------------------------------
def _rows32(y, what="y") -> np.ndarray:
    a = y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
    if a.dtype != np.float32:
        raise _lib.AidError(f"declicking: {what} must be float32 (the run rule compares bits), got {a.dtype}")
    a = a.reshape(1, -1) if a.ndim == 1 else a
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise _lib.AidError(f"declicking: {what} must be [R, N] with R, N >= 1, got {a.shape}")
    return np.ascontiguousarray(a)


def _forward_sum(p: np.ndarray) -> float:
    return float(np.cumsum(p)[-1])                                   # (cumsum adds in index order)


def _pairwise_sum(p: np.ndarray) -> float:
    n = 1 << max(0, int(p.size - 1).bit_length())
    p = np.concatenate([p, np.zeros(n - p.size)])
    while p.size > 1:
        p = p[0::2] + p[1::2]
    return float(p[0])


def levinson_host(r, order: int) -> np.ndarray:
    """a[0 .. order] with a[0] = 1 from the autocorrelation r[0 .. order] (r[0] > 0), operation by operation what the kernel's lane 0 does"""
    r = [float(v) for v in r]
    a = [1.0] + [0.0] * order
    E = r[0]
    for m in range(1, order + 1):
        if not E > 0.0:
            break
        acc = r[m]
        for k in range(1, m):
            acc = acc + a[k] * r[m - k]
        kr = -acc / E
        a[1:m] = [a[k] + kr * a[m - k] for k in range(1, m)]
        a[m] = kr
        E = E * (1.0 - kr * kr)
    return np.asarray(a, dtype=np.float64)


def score_host(y, *, block=2048, order=16, ridge=1e-6, sigma_floor=1e-6, autocorr: str = "forward", store=np.float32):
    """y [R, N] float32 -> (score [R, N] float32, sigma [R, J] float64) as CPU tensors: THE SCORE of the module docstring in float64.
    ``autocorr``: "forward" adds the products of a lag in index order (the definition), "pairwise" as a binary tree; ``store`` =
    numpy.float64 leaves out the float32 store of the score.  Both serve the measurement of what a second summation order moves."""
    cfg = make_settings(block=block, order=order, ridge=ridge, sigma_floor=sigma_floor)
    add = {"forward": _forward_sum, "pairwise": _pairwise_sum}[autocorr]
    y = _rows32(y)
    R, N = y.shape
    B, K = cfg.block, cfg.order
    J = -(-N // B)
    score, sigma = np.zeros((R, N), dtype=store), np.zeros((R, J))
    for b in range(R):
        ypad = np.concatenate([np.zeros(K), y[b].astype(np.float64)])                # ypad[K + q] = y[q]
        for j in range(J):
            base = j * B
            n = min(B, N - base)
            if n < 8 * K:
                continue
            x = ypad[K + base:K + base + n]
            r = [add(x[m:] * x[:n - m]) for m in range(K + 1)]
            r[0] = r[0] * (1.0 + cfg.ridge)
            if not r[0] > 0.0:
                continue
            a = levinson_host(r, K)
            e = np.zeros(n)
            for k in range(K + 1):
                e = e + a[k] * ypad[K + base - k:K + base - k + n]
            e = np.abs(e)
            scored = np.arange(base, base + n) >= K
            srt = np.sort(e[scored])
            sigma[b, j] = max(srt[srt.size // 2] / 0.6745, cfg.sigma_floor)
            score[b, base:base + n] = np.where(scored, e / sigma[b, j], 0.0).astype(store)
    return torch.from_numpy(score), torch.from_numpy(sigma)


def flags_host(y, score, *, threshold=8.0, min_run=8, max_run=1024) -> np.ndarray:
    """[R, N] bool: THE FLAGS of the module docstring"""
    cfg = make_settings(threshold=threshold, min_run=min_run, max_run=max_run)
    y, s = _rows32(y), _rows32(score, "score")
    if y.shape != s.shape:
        raise _lib.AidError(f"declicking: y {y.shape} and score {s.shape} differ in shape")
    R, N = y.shape
    flags = s > np.float32(cfg.threshold)
    if cfg.min_run > 0:
        bits = y.view(np.uint32)
        for b in range(R):
            starts = np.flatnonzero(np.concatenate([[True], bits[b, 1:] != bits[b, :-1]]))
            ends = np.concatenate([starts[1:], [N]]) - 1
            lens = ends - starts + 1
            ok = (lens >= cfg.min_run) & (lens <= cfg.max_run) & (starts > 0) & (ends < N - 1)
            flags[b] |= np.repeat(ok, lens)
    return flags


def mask_host(y, score, *, threshold=8.0, pad=16, min_run=8, max_run=1024) -> torch.Tensor:
    """y, score [R, N] float32 -> mask [R, N] float32 on the CPU: THE FLAGS and THE MASK of the module docstring, exactly"""
    cfg = make_settings(threshold=threshold, pad=pad, min_run=min_run, max_run=max_run)
    flags = flags_host(y, score, threshold=cfg.threshold, min_run=cfg.min_run, max_run=cfg.max_run)
    R, N = flags.shape
    c = np.concatenate([np.zeros((R, 1), dtype=np.int64), np.cumsum(flags, axis=1, dtype=np.int64)], axis=1)      # c[q] = the flags before q
    q = np.arange(N)
    near = c[:, np.minimum(N, q + cfg.pad + 1)] - c[:, np.maximum(0, q - cfg.pad)]
    return torch.from_numpy((near == 0).astype(np.float32))


def report_of(mask):
    """(n_flagged, n_gaps, longest_gap), int64 tensors [R] on the host, of a mask [R, N] (any device; read back once)"""
    z = (mask.detach().cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)) == 0
    z = z.reshape(1, -1) if z.ndim == 1 else z
    R, N = z.shape
    out = np.zeros((3, R), dtype=np.int64)
    for b in range(R):
        edge = np.diff(np.concatenate([[0], z[b].astype(np.int8), [0]]))
        starts, ends = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
        out[:, b] = z[b].sum(), starts.size, (ends - starts).max() if starts.size else 0
    return tuple(torch.from_numpy(o.copy()) for o in out)


def detect_host(y, **settings) -> Detection:
    """``detect`` restated in float64 on the CPU: the definition, not a fallback"""
    cfg = make_settings(**settings)
    s, sigma = score_host(y, **cfg.score_args)
    m = mask_host(y, s, **cfg.mask_args)
    return Detection(m, s, sigma, *report_of(m))


# ---- helpers of the tests, the tool and the benchmark (host only) ----------------------------------------------------------------------------
def add_clicks(x, n, seed, width=(1, 5), amplitude=(0.1, 0.5), dropouts=0, dropout_len=(8, 64)):
    """Damage x ([N] or [R, N]) with ``n`` clicks per recording -- ``width`` samples wide (a whole number drawn from the closed range), one
    level of ``amplitude`` (drawn from the range, either sign) added to each of them -- and ``dropouts`` dropouts per recording of
    ``dropout_len`` samples set to 0, neither touching the first or the last sample.  -> (y float32, truth bool: the damaged samples), of the
    kind (tensor or array) and shape of x.  Seeded with numpy.random.default_rng(seed): the same arguments give the same bits."""
    as_tensor = torch.is_tensor(x)
    a = np.array(x.detach().cpu().numpy() if as_tensor else x, dtype=np.float32)
    rows = a.reshape(1, -1) if a.ndim == 1 else a
    if rows.ndim != 2 or rows.shape[1] < max(width[1], dropout_len[1] if dropouts else 0) + 2:
        raise _lib.AidError(f"add_clicks: x must be [N] or [R, N] and longer than the widest defect, got {a.shape}")
    rng = np.random.default_rng(seed)
    truth = np.zeros(rows.shape, dtype=bool)
    N = rows.shape[1]
    for b in range(rows.shape[0]):
        for _ in range(int(n)):
            w = int(rng.integers(width[0], width[1] + 1))
            q = int(rng.integers(1, N - w))
            rows[b, q:q + w] += np.float32(rng.uniform(amplitude[0], amplitude[1]) * (1 if rng.random() < 0.5 else -1))
            truth[b, q:q + w] = True
        for _ in range(int(dropouts)):
            w = int(rng.integers(dropout_len[0], dropout_len[1] + 1))
            q = int(rng.integers(1, N - w))
            rows[b, q:q + w] = 0.0
            truth[b, q:q + w] = True
    y, truth = rows.reshape(a.shape), truth.reshape(a.shape)
    return (torch.from_numpy(y), torch.from_numpy(truth)) if as_tensor else (y, truth)


def detection_scores(mask, truth, pad: int = 16) -> dict:
    """recall: the fraction of the truth samples under the mask (mask == 0); precision: the fraction of the masked samples within ``pad`` of a
    truth sample (nan where the denominator is 0)"""
    m = (mask.detach().cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)) == 0
    t = (truth.detach().cpu().numpy() if torch.is_tensor(truth) else np.asarray(truth)).astype(bool)
    m, t = m.reshape(-1, m.shape[-1]), t.reshape(-1, t.shape[-1])
    near = mask_host(np.zeros(t.shape, dtype=np.float32), t.astype(np.float32), threshold=0.5, pad=pad, min_run=0).numpy() == 0
    nan = float("nan")
    return {"recall": float((m & t).sum() / t.sum()) if t.any() else nan, "precision": float((m & near).sum() / m.sum()) if m.any() else nan}


# ---- the kernels -----------------------------------------------------------------------------------------------------------------------------
def _device_rows(t, what, like=None):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.AidError(f"declicking: {what} must be a tensor on the GPU (no CPU fallback; detect_host restates the detector in float64)")
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise _lib.AidError(f"declicking: {what} must be float32 [R, N] with R, N >= 1, got {t.dtype} {tuple(t.shape)}")
    if t.shape[0] > MAX_ROWS:
        raise _lib.AidError(f"declicking: {t.shape[0]} recordings in one call, at most {MAX_ROWS}")
    if like is not None and (tuple(t.shape) != tuple(like.shape) or t.device != like.device):
        raise _lib.AidError(f"declicking: {what} must be {tuple(like.shape)} on {like.device}, got {tuple(t.shape)} on {t.device}")
    return t


def _in_place(t) -> bool:
    """rows of a wider buffer are read and written in place"""
    return (t.stride(1) == 1 or t.shape[1] == 1) and (t.shape[0] == 1 or t.stride(0) >= t.shape[1])


def _ld(t) -> int:
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _out(out, like, what):
    if out is None:
        return torch.empty(tuple(like.shape), dtype=torch.float32, device=like.device)
    if not _in_place(_device_rows(out, what, like)):
        raise _lib.AidError(f"declicking: {what} must have unit stride along N and a row stride of at least N")
    return out


def score(y, *, block=2048, order=16, ridge=1e-6, sigma_floor=1e-6, out=None, sigma_out=None):
    """One aid_ar_score launch on the current stream: y [R, N] (float32, GPU; rows of a wider buffer are read in place) ->
    (score [R, N] float32, sigma [R, J] float32, J = ceil(N / block)).  ``out`` / ``sigma_out``: write there (sigma contiguous)."""
    cfg = make_settings(block=block, order=order, ridge=ridge, sigma_floor=sigma_floor)
    y = _device_rows(y, "y")
    y = y if _in_place(y) else y.contiguous()
    R, N = y.shape
    J = -(-N // cfg.block)
    if J > 2 ** 31 - 1:
        raise _lib.AidError(f"declicking: {J} blocks per recording are 2^31 or more")
    s = _out(out, y, "out")
    sigma = torch.empty((R, J), dtype=torch.float32, device=y.device) if sigma_out is None else sigma_out
    if not (torch.is_tensor(sigma) and sigma.is_cuda and sigma.dtype == torch.float32 and tuple(sigma.shape) == (R, J) and sigma.is_contiguous()
            and sigma.device == y.device):
        raise _lib.AidError(f"declicking: sigma_out must be a contiguous float32 tensor [{R}, {J}] on {y.device}")
    scalars = (ctypes.c_float * 2)(cfg.ridge, cfg.sigma_floor)                       # (host memory: read by the launcher)
    _lib.call("aid_ar_score", _lib.BweGatherParams(y.data_ptr(), ctypes.addressof(scalars), s.data_ptr(), sigma.data_ptr(), None,
                                                   J, R, cfg.order, cfg.block, N, _ld(y), _ld(s)))
    return s, sigma


def mask(y, score, *, threshold=8.0, pad=16, min_run=8, max_run=1024, out=None):
    """One aid_click_mask launch on the current stream: y, score [R, N] (float32, GPU) -> mask [R, N] float32, 1 = observed, 0 = restore"""
    cfg = make_settings(threshold=threshold, pad=pad, min_run=min_run, max_run=max_run)
    y = _device_rows(y, "y")
    sc = _device_rows(score, "score", y)
    y, sc = (t if _in_place(t) else t.contiguous() for t in (y, sc))
    R, N = y.shape
    m = _out(out, y, "out")
    scalars = (ctypes.c_float * 4)(cfg.threshold, cfg.pad, cfg.min_run, cfg.max_run)  # (host memory: read by the launcher)
    _lib.call("aid_click_mask", _lib.FirObservedParams(y.data_ptr(), sc.data_ptr(), None, ctypes.addressof(scalars), m.data_ptr(),
                                                       R, 0, 0, N, _ld(y), _ld(sc), 0, _ld(m)))
    return m


def detect(y, **settings) -> Detection:
    """y [R, N] float32 on the GPU (any N >= 1) -> Detection: mask, score and sigma on the GPU, the report as int64 tensors [R] on the host.
    Two launches on the current stream and one read-back, of the mask.  Deterministic: the same recording gives the same bits, alone or in a
    batch, on every rank."""
    cfg = make_settings(**settings)
    s, sigma = score(y, **cfg.score_args)
    m = mask(y, s, **cfg.mask_args)
    return Detection(m, s, sigma, *report_of(m))


def check_fraction(n_masked, N, max_fraction: float, what: str = "recording") -> None:
    """Refuse, by index, every recording of which more than ``max_fraction`` is masked (``N``: the length of all, or one per recording): a
    detector that flags that much is looking at something that is not click damage."""
    N = [int(N)] * len(n_masked) if isinstance(N, (int, np.integer)) else [int(v) for v in N]
    bad = [(i, int(n), N[i]) for i, n in enumerate(n_masked) if int(n) > max_fraction * N[i]]
    if bad:
        raise _lib.AidError("declicking: " + "; ".join(f"{what} {i}: {n} of {tot} samples ({n / tot:.1%}) are masked" for i, n, tot in bad) +
                            f", more than max_fraction = {max_fraction:g}: this is not click damage (raise max_fraction or the threshold to go on)")


def combine(det_mask, mask: Optional[torch.Tensor]):
    """the detected mask [R, N] times the known gaps ``mask`` ([N], [1, N] or [R, N]; 1 = observed), or itself without one"""
    if mask is None:
        return det_mask
    R, N = det_mask.shape
    m = torch.as_tensor(mask)
    m = m.reshape(1, -1) if m.dim() == 1 else m
    if m.dim() != 2 or m.shape[1] != N or m.shape[0] not in (1, R):
        raise _lib.AidError(f"declicking: mask must be [{N}], [1, {N}] or [{R}, {N}], got {tuple(m.shape)}")
    return det_mask * m.to(device=det_mask.device, dtype=det_mask.dtype)
