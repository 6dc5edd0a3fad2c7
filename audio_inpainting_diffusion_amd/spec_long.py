"""Spectrogram inpainting of whole recordings, longer than one model segment -- in two batched sampler passes (include/aid_spec_long.h).

The recording was masked as a whole: y = A(x) = crop(istft(mask . stft(zero-pad(x)))), the reference's Sampler.apply_spectral_mask
(stft.SpectralMask) over all N samples.  In recording coordinates: Np = N + (n_fft - N % n_fft), T_rec = 1 + Np // hop, half = n_fft // 2;
frame t reads the positions q = t hop - half + j, j in [0, n_fft), through  q < 0 -> -q,  q >= Np -> 2 (Np - 1) - q,  x[q] if q < N else 0,  and

    A(x)[n] = 1/env[n] * sum_t w[n + half - t hop] * (F^-1 diag(mask[:, t]) F (w . frame_t))[n + half - t hop]

over the frames t in [0, T_rec) that cover n (env: the overlap-added squared window over the same frames).  A window cut out of y is NOT the
masked window: within n_fft of a border the recording's frames read samples the window does not hold, and SpectralMask reflect-pads at its
own ends.  So the grid of restore.py is used with the requested overlap end = int(overlap * L) widened to

    end' = end + ((L - end) % hop)              so that every window start s is a multiple of hop (restore.aligned_end):

window frame j is then recording frame s // hop + j, and Tw = 1 + (L + n_fft) // hop covers every frame a window can compute.  Frame t is
COMPUTABLE in the window when every position it reads, after the two reflections, is either >= N or inside [s, s + L) -- one rule for the
reflect padding at the start of the recording, the appended zeros at its end and the reflection about Np, which reads real samples when
N % n_fft >= half (its lowest position is Np - half - 1).  A sample of a window is in one of four STATES (``window_state``, first match): -2 absent (s + i >= N; it enters as 0), 1
known (head / tail, taken from the result so far), 0 observed (every frame of the recording that covers s + i is computable: y = the
recording's y), -1 unobserved (it exists and feeds frames, but its own y depends on samples outside the window).  At a state-0 sample the
window operator performs the recording's arithmetic on the recording's numbers; nothing is subtracted or approximated.  Windows, heads, tails
and owned ranges are restore.trimmed_windows(N, L, end', K = 2 n_fft - 1): the reach of A is n_fft - 1 to either side, so ownership is trimmed by
m = 2 (n_fft - 1), and more than one window needs end' >= 2 m.

JOBS.  A frame is touched when a bin of its mask column differs from 1; a sample is affected when a touched frame covers it; a window is a job
when its owned range holds an affected sample.  Unaffected samples of y are the signal itself, so the result starts as a copy of y and windows
without a masked bin cost nothing.  The touched-frame flags are reduced on the GPU and come to the host once, before pass A.

``SpectralMaskObserved`` is the operator, on the HIP kernels of csrc/aid_spec_long.hip (aid_stft_mask_observed: the frame and overlap-add
bodies of aid_stft_frames / aid_stft_ola with selects); ``spec_gather`` builds the observations, states and items of all windows of a pass in
one launch; ``spec_passes`` is the pass code, driven with anything that has ``predict_resample``.  GPU only; no fallback.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import restore
from .restore import aligned_end
from .stft import stft_tables


def check_sizes(n_fft, hop):
    """(n_fft, hop) as ints: n_fft a power of two in [16, 8192], hop a divisor of it"""
    if isinstance(n_fft, bool) or not isinstance(n_fft, int) or n_fft & (n_fft - 1) or not 16 <= n_fft <= 8192:
        raise _lib.AidError(f"n_fft must be a power of two in [16, 8192], got {n_fft!r}")
    if isinstance(hop, bool) or not isinstance(hop, int) or hop < 1 or n_fft % hop:
        raise _lib.AidError(f"hop_length must divide n_fft = {n_fft} (every window then starts on the hop grid and the padded length is a multiple of "
                            f"it), got {hop!r}")
    return n_fft, hop


def padded_length(N: int, n_fft: int) -> int:
    """Np: the reference pads to a multiple of n_fft, by a full block when N already is one"""
    return int(N) + (int(n_fft) - int(N) % int(n_fft))


def rec_frames(N: int, n_fft: int, hop: int) -> int:
    """T_rec: the number of STFT frames of a recording of N samples"""
    return 1 + padded_length(N, n_fft) // int(hop)


def window_frames(L: int, n_fft: int, hop: int) -> int:
    """Tw: the number of frame slots of a window of L samples"""
    return 1 + (int(L) + int(n_fft)) // int(hop)


def spec_windows(N: int, L: int, end: int, n_fft: int, hop: int):
    """(start s, head, tail, lo, hi) of every window, as restore.trimmed_windows(N, L, end', 2 n_fft - 1) with the aligned overlap end':
    every s is a multiple of hop."""
    return restore.trimmed_windows(N, L, aligned_end(L, end, hop), 2 * int(n_fft) - 1)


def computable(t, N: int, L: int, n_fft: int, hop: int, s: int) -> np.ndarray:
    """frames t (an int array, every t in [0, T_rec)) of the recording are computable in the window [s, s + L): in closed form.  The positions
    of frame t are [a, a + n_fft), a = t hop - half; folded at 0 they are [max(a, 0), max(a + n_fft - 1, -a)]; folded at Np the part at and
    past Np lands next to the part below it; what lies below N must lie in the window."""
    t = np.asarray(t, dtype=np.int64)
    Np = padded_length(N, n_fft)
    a = t * hop - n_fft // 2
    b = a + n_fft - 1
    lo, hi = np.maximum(a, 0), np.maximum(b, -a)
    over = hi >= Np
    lo = np.where(over, np.minimum(lo, 2 * (Np - 1) - hi), lo)
    hi = np.minimum(np.where(over, Np - 1, hi), N - 1)
    return (lo > hi) | ((lo >= s) & (hi < s + L))


def window_state(N: int, L: int, n_fft: int, hop: int, s: int, head: int, tail: int) -> np.ndarray:
    """The state of every sample and every frame of the window that starts at s (float32 [L + Tw]; host reference of aid_spec_gather).
    Sample i: -2 absent, 1 known, 0 observed, -1 unobserved.  Frame j: -2 absent, -1 not computable, 0 computable.  The first match decides."""
    if s % hop:
        raise _lib.AidError(f"window_state: the window start {s} is no multiple of hop_length {hop}")
    half, T_rec, Tw = n_fft // 2, rec_frames(N, n_fft, hop), window_frames(L, n_fft, hop)
    ok = computable(np.arange(T_rec), N, L, n_fft, hop, s)
    bad = np.concatenate([[0], np.cumsum(~ok)])                                 # frames before t that are not computable
    i = np.arange(L)
    q = s + i + half
    t1 = np.minimum(q // hop, T_rec - 1)
    t0 = np.minimum(np.where(q - (n_fft - 1) < 0, 0, -(-(q - (n_fft - 1)) // hop)), T_rec)       # (past T_rec only where the sample is absent)
    observed = bad[np.maximum(t1 + 1, t0)] == bad[t0]
    known = (i < head) | (i >= L - tail)
    samples = np.where(s + i >= N, -2.0, np.where(known, 1.0, np.where(observed, 0.0, -1.0)))
    t = s // hop + np.arange(Tw)
    frames = np.where(t >= T_rec, -2.0, np.where(ok[np.minimum(t, T_rec - 1)], 0.0, -1.0))
    return np.concatenate([samples, frames]).astype(np.float32)


def touched_frames(mask: torch.Tensor) -> torch.Tensor:
    """mask [F, T_rec] or [R, F, T_rec] on any device -> bool [1|R, T_rec] on the same device: the frame has a bin that differs from 1"""
    if mask.dim() == 2:
        mask = mask.unsqueeze(0)
    return (mask != 1).any(dim=1)


def spec_plan(touched, R: int, N: int, L: int, end: int, n_fft: int, hop: int):
    """touched [1|R, T_rec] (bool, host: frame t of the recording has a mask bin that differs from 1) -> (jobs_A, jobs_B): the even / odd
    windows whose owned range holds a sample that a touched frame covers, as (r, s, head, tail, lo, hi), ordered by recording and window.  A
    one-row ``touched`` is shared: its jobs are repeated for every recording."""
    touched = np.asarray(touched.cpu() if torch.is_tensor(touched) else touched, dtype=bool)
    T_rec, half = rec_frames(N, n_fft, hop), n_fft // 2
    if touched.ndim != 2 or touched.shape[0] not in (1, int(R)) or touched.shape[1] != T_rec:
        raise _lib.AidError(f"spec_plan: touched {touched.shape} is no [1|{R}, {T_rec}]")
    wins = spec_windows(N, L, end, n_fft, hop)
    jobs = ([], [])
    cums = []
    for row in touched:
        d = np.zeros(N + 1, dtype=np.int64)                                     # frame t covers the samples [t hop - half, t hop + half) of [0, N)
        for t in np.flatnonzero(row):
            a, b = max(0, t * hop - half), min(N, t * hop + half)
            if a < b:
                d[a] += 1
                d[b] -= 1
        affected = np.cumsum(d[:N]) > 0
        cums.append(np.concatenate([[0], np.cumsum(affected)]))                 # affected samples before q
    for r in range(int(R)):
        c = cums[r if len(cums) > 1 else 0]
        for w, (s, head, tail, lo, hi) in enumerate(wins):
            if c[s + hi] > c[s + lo]:
                jobs[w % 2].append((r, s, head, tail, lo, hi))
    return jobs


def spec_tables(N: int, n_fft: int, hop: int, win_length: Optional[int], device):
    """(window [n_fft], 1 / envelope [Np], twiddle [n_fft/2, 2]) of the recording as float32 on ``device``: stft.stft_tables over all N samples
    (float64 on the host, from the fp32-rounded window)"""
    w, env, tw = stft_tables(int(N), n_fft, hop, n_fft if win_length is None else int(win_length))
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device) for a in (w, 1.0 / env, tw))


class SpectralMaskObserved(restore.WindowOperator):
    """Observation of x[B, L] through the recording's STFT-domain masking operator: mask [1|R, F, T_rec] (float32 on the GPU, unit stride
    along T_rec; read in place), state [B, L + Tw] and items [B, 3] = (r, s, N) as ``spec_gather`` builds them, tables = spec_tables(N, ...).
    With kh the first L states, kf the rest, xin = 0 where kh is absent, x elsewhere, and c = the recording's operator over the frames with
    kf == 0 (window frame j is recording frame s // hop + j and multiplies by column s // hop + j of the mask of recording r):

        apply(x)       x where known, c where observed, 0 where unobserved or absent
        adjoint(g)     with a = the transpose over the same frames of (g where observed, else 0): 0 where absent, a + g where known, a elsewhere
        project(x, y)  y where known, (-c + y) + x where observed (the order of SpectralMask.project), x where unobserved or absent

    The operator protocol of degrade.py over restore.WindowOperator (``rows(lo, hi)``; the mask and the tables stay shared; the frame
    scratch per (B, stream)).  Every item has its own (r, s, N), so the state has one row per item, never a shared one.  Linear: it keeps
    nothing else between calls.  With N = L, s = 0 and every sample observed the three give SpectralMask's bits."""

    def __init__(self, mask: torch.Tensor, n_fft: int, hop: int, state: torch.Tensor, items: torch.Tensor, tables):
        self.N, self.hop = check_sizes(n_fft, hop)
        self.F = self.N // 2 + 1
        if not (torch.is_tensor(mask) and mask.is_cuda and mask.dtype == torch.float32 and mask.dim() == 3 and mask.shape[1] == self.F
                and mask.shape[2] >= 2 and mask.stride(2) == 1 and (mask.shape[2] - 1) * self.hop % self.N == 0):
            raise _lib.AidError(f"SpectralMaskObserved: mask must be a float32 GPU tensor [1|R, {self.F}, T_rec] with unit stride along T_rec and "
                                "(T_rec - 1) hop a multiple of n_fft (no CPU fallback)")
        super().__init__(state, "[B, L + Tw]")
        self.T_rec = mask.shape[2]
        self.Np = (self.T_rec - 1) * self.hop
        q, m = divmod(state.shape[1] - 1 - self.N // self.hop, self.hop + 1)     # L = q hop + m, m < hop  <=>  L + (L + n_fft) // hop = q (hop + 1) + m + n_fft / hop
        self.L = q * self.hop + m
        if m == self.hop or self.L < 1:
            raise _lib.AidError(f"SpectralMaskObserved: a state row of {state.shape[1]} entries is no L + 1 + (L + {self.N}) // {self.hop} for any L >= 1")
        self.Tw = window_frames(self.L, self.N, self.hop)
        B = state.shape[0]
        if not (torch.is_tensor(items) and items.is_cuda and items.dtype == torch.int64 and tuple(items.shape) == (B, _lib.AID_SPEC_ITEM_FIELDS)
                and items.is_contiguous()):
            raise _lib.AidError(f"SpectralMaskObserved: items must be a contiguous int64 GPU tensor [{B}, {_lib.AID_SPEC_ITEM_FIELDS}] (spec_gather)")
        self.window, self.inv_env, self.twiddle = tables
        if self.window.numel() != self.N or self.inv_env.numel() != self.Np:
            raise _lib.AidError(f"SpectralMaskObserved: the tables are not those of n_fft = {self.N} and a padded length of {self.Np} (spec_tables)")
        self.mask, self.items, self.tables = mask, items, tables

    @property
    def items_held(self) -> int:
        return self.state.shape[0]

    def _slice(self, lo: int, hi: int) -> "SpectralMaskObserved":
        return SpectralMaskObserved(self.mask, self.N, self.hop, self.state[lo:hi], self.items[lo:hi], self.tables)

    def _run(self, mode, x, y=None):
        x = self._signal(x, self.L)
        B, L = x.shape[0], self.L
        fr = self._scratch(B, self.Tw, self.N, device=x.device)
        out = torch.empty_like(x)
        m = self.mask
        _lib.call("aid_stft_mask_observed", _lib.StftMaskObservedParams(
            x.data_ptr(), _lib.ptr(y), self.state.data_ptr(), self.items.data_ptr(), self.window.data_ptr(), self.twiddle.data_ptr(),
            self.inv_env.data_ptr(), m.data_ptr(), fr.data_ptr(), out.data_ptr(), L, self.Np, L, L, self.state.stride(0), L,
            m.stride(0) if m.shape[0] > 1 else 0, m.stride(1), B, m.shape[0], self.N, self.hop, self.Tw, mode))
        return out

    def apply(self, x):
        return self._run(0, x)

    def adjoint(self, g):
        return self._run(1, g)

    def project(self, x, y):
        return self._run(2, x, y=self._observation(x, y, self.L))


def spec_gather(rec: torch.Tensor, out: torch.Tensor, jobs: torch.Tensor, L: int, n_fft: int, hop: int):
    """One aid_spec_gather launch on the current stream -> (y [J, L], state [J, L + Tw], items [J, 3]): the observations, the states
    (``window_state``) and the (r, s, N) of every job's window; known samples from ``out`` [R, N], observed ones from ``rec`` [R, N], 0
    where there is no observation."""
    for t, what in ((rec, "rec"), (out, "out")):
        restore._rows(t, what)
    restore._table(jobs)
    n_fft, hop = check_sizes(n_fft, hop)
    L = int(L)
    R, N = rec.shape
    if out.shape != rec.shape or L < 1 or N < 1:
        raise _lib.AidError(f"spec_gather: rec {tuple(rec.shape)} and out {tuple(out.shape)} do not match, or are empty, or L = {L} is below 1")
    J, Tw = jobs.shape[0], window_frames(L, n_fft, hop)
    y = torch.empty((J, L), dtype=torch.float32, device=rec.device)
    k = torch.empty((J, L + Tw), dtype=torch.float32, device=rec.device)
    items = torch.empty((J, _lib.AID_SPEC_ITEM_FIELDS), dtype=torch.int64, device=rec.device)
    if J:
        _lib.call("aid_spec_gather", _lib.SpecGatherParams(rec.data_ptr(), out.data_ptr(), y.data_ptr(), k.data_ptr(), items.data_ptr(), jobs.data_ptr(),
                                                           L, N, padded_length(N, n_fft), rec.stride(0), out.stride(0), J, R, n_fft, hop, Tw))
    return y, k, items


def check_spec_args(y: torch.Tensor, mask: torch.Tensor, n_fft, hop, win_length, window, L: int, end: int, max_batch: int, seeds):
    """The refusals of a spectrogram inpainting of whole recordings, all raised before anything is launched -> (n_fft, hop, mask as
    [1|R, F, T_rec]).  What can be judged without a GPU is judged first; the device of y last."""
    if window != "hann":
        raise NotImplementedError(f"Only hann window is implemented for now, got {window!r}")                 # as the reference (:276)
    n_fft, hop = check_sizes(n_fft, hop)
    if win_length is not None and (isinstance(win_length, bool) or not isinstance(win_length, int) or not 1 <= win_length <= n_fft):
        raise _lib.AidError(f"win_length must be an integer in [1, n_fft = {n_fft}], got {win_length!r}")
    restore.check_rows(y, "recordings [R, N]", nonempty=True)
    R, N = y.shape
    F, T_rec = n_fft // 2 + 1, rec_frames(N, n_fft, hop)
    if torch.is_tensor(mask) and mask.dim() == 2:
        mask = mask.unsqueeze(0)
    if not (torch.is_tensor(mask) and mask.dim() == 3 and mask.shape[0] in (1, R) and tuple(mask.shape[1:]) == (F, T_rec)):
        raise _lib.AidError(f"the spectral mask of recordings of {N} samples must be [{F}, {T_rec}] or [{R}, {F}, {T_rec}] (F = n_fft / 2 + 1, "
                            f"T_rec = 1 + Np // hop_length with Np = {padded_length(N, n_fft)}: masks.spectral_mask(audio_len = {N})), "
                            f"got {tuple(mask.shape) if torch.is_tensor(mask) else type(mask).__name__}")
    spec_windows(N, L, end, n_fft, hop)                                    # (end' in [1, L/2); end' >= 4 (n_fft - 1) with more than one window)
    restore.check_batch(y, max_batch, seeds, "spectrogram inpainting of whole recordings")
    return n_fft, hop, mask


def spec_passes(sampler, y: torch.Tensor, mask: torch.Tensor, n_fft, hop, L: int, end: int, win_length=None, window: str = "hann",
                max_batch: int = 8, seeds: Optional[Sequence[int]] = None) -> torch.Tensor:
    """The two passes over ``sampler.predict_resample(yw [B, L], (B, L), SpectralMaskObserved(...)) -> [B, L]`` with B <= max_batch:
    y [R, N] recordings masked as a whole, on the GPU (rows contiguous, any row stride), mask [F, T_rec] or [R, F, T_rec] (any dtype and
    device; used in place when it is float32 on y's device with unit stride along T_rec) -> restored [R, N].  The touched-frame flags are
    reduced on the GPU and read once, the plan is made on the host (``spec_plan``); then per pass one aid_spec_gather launch, the sampler
    calls, one aid_window_scatter launch per call (restore.run_passes, with the aligned step L - end').  Seeds as restore.restore_passes."""
    n_fft, hop, mask = check_spec_args(y, mask, n_fft, hop, win_length, window, L, end, max_batch, seeds)
    R, N = y.shape
    dmask = mask.detach().to(y.device, torch.float32)
    if dmask.stride(2) != 1 or dmask.stride(1) < dmask.shape[2] or (dmask.shape[0] > 1 and dmask.stride(0) < dmask.shape[1] * dmask.stride(1)):
        dmask = dmask.contiguous()                                         # (one copy per call, never one per window)
    touched = touched_frames(dmask).cpu().numpy()                          # [1|R, T_rec]: reduced on the GPU; the one read-back, before pass A
    jobs_A, jobs_B = spec_plan(touched, R, N, L, end, n_fft, hop)
    out = y.clone(memory_format=torch.contiguous_format)
    if restore.no_jobs(jobs_A, jobs_B):
        return out
    tables = spec_tables(N, n_fft, hop, win_length, y.device)

    def predict(win, c0, c1):
        yw, kw, iw = (t[c0:c1] for t in win)
        return sampler.predict_resample(yw, (c1 - c0, L), SpectralMaskObserved(dmask, n_fft, hop, kw, iw, tables))
    restore.run_passes(sampler, out, (jobs_A, jobs_B), L - aligned_end(L, end, hop), max_batch, seeds,
                       lambda table: spec_gather(y, out, table, L, n_fft, hop), predict, L=L)
    return out
