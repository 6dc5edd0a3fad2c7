"""EDM inpainting sampler on MI355X -- drop-in for ``testing.edm_sampler_inpainting.Sampler``.

Call surface kept from the reference (testing/edm_sampler_inpainting.py): ``Sampler(model, diff_params, args,
rid=False)`` (:10), public attributes ``xi / nb_steps / order`` (:19-32), ``predict_inpainting(y_masked, mask)``
(:327), ``predict_spectrogram_inpainting(y_masked, mask[F,T])`` (:348), ``predict_unconditional(shape, device)`` (:155),
``update_diff_params`` (:43).  The loop (:178-262) stays
in Python but is sync-free: the schedule, gamma and every per-step scalar live on the host (float32 torch
arithmetic identical to the reference), noise is drawn from the CPU generator in the reference's order and
copied asynchronously, and each step costs two fused element-wise launches besides the denoiser evaluations.

Batch semantics (new; the reference only ever runs B=1 and its guided branch raises for B>1, :75-:78): every
reduction the reference takes over the whole batch -- the guidance norm (:75), ``normguide`` (:83) and the mask
row used for smoothing (:307) -- is taken PER ITEM, so item b of a batch reproduces the reference's B=1 run.
``seeds=[...]`` gives every item its own CPU generator (prior draw, then one draw per churned step), making
results independent of batch composition and of how segments are sharded over GPUs.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from . import bwe_declip_long, bwe_iir_long, bwe_long, declip_long, lowrate_long, phase_long, restore    # noqa: F401  (each declares its mode in restore.LONG_TASKS)
from .degrade import Decimate, FIRFilter, HardClip, IIRFilter, SincResample
from .phase import STFTMagnitude, observation_shape
from .stft import SpectralMask


def prepare_smooth_mask(mask: torch.Tensor, size: int) -> torch.Tensor:
    """Hann cross-fade of the mask edges, row by row (vectorised form of :302-325; the reference walks all L
    samples of row 0 in a Python loop and re-uses the result for every item).  A ramp that would reach past an end of the row -- where the
    reference's slice assignment raises -- is cut there: the windows of a whole-recording restoration (restore.py) have gaps anywhere."""
    hann = torch.hann_window(size * 2)
    left, right = hann[0:size], hann[size:]
    m = mask.detach().to("cpu", torch.float32)
    out = m.clone()
    n = m.shape[1]
    for r in range(m.shape[0]):
        row = m[r].numpy()
        prev = np.concatenate(([1.0], row[:-1]))
        for i in np.nonzero(row != prev)[0]:
            i = int(i)
            if row[i] == 0:
                a = max(i - size, 0)
                out[r, a:i] = right[size - (i - a):]
            if row[i] == 1:
                b = min(i + size, n)
                out[r, i:b] = left[:b - i]
    return out


class LambdaDegradation:
    """A degradation given as a torch callable (the ``degradation`` lambda of ``Sampler.predict_resample``, :164-173; the reference
    differentiates ``norm(y - degradation(x_hat))`` through it with torch.autograd, :65-81).  Here the callable and its VJP at x_hat are the
    only torch-eager pieces of a guided evaluation: ``apply`` evaluates it on a leaf copy of x_hat, ``adjoint`` pulls the analytic seed
    d norm / d degradation(x_hat) (aid_guidance_seed) back through it -- for a linear operator that is its adjoint, for any other one exactly
    the Jacobian-transpose product the reference's autograd forms -- and the network's hand-written input-VJP takes over from there.
    The reference defines no projection for it (``proj_convex_set`` only exists after predict_inpainting / predict_spectrogram_inpainting)."""
    shared_mask = False                              # (network.denoise_guided: one stream, no graph replay -- the callable is opaque)

    def __init__(self, fn):
        self.fn = fn
        self._leaf = self._den = None

    def apply(self, x_hat):
        with torch.enable_grad():
            self._leaf = x_hat.detach().requires_grad_(True)
            self._den = self.fn(self._leaf)
        if not torch.is_tensor(self._den) or self._den.shape[0] != x_hat.shape[0]:
            raise _lib.AidError("predict_resample: degradation(x_hat) must return a tensor with the batch axis first")
        return self._den.detach().float().contiguous()

    def adjoint(self, g):
        if self._den is None:
            raise _lib.AidError("LambdaDegradation.adjoint before apply")
        den, leaf, self._den, self._leaf = self._den, self._leaf, None, None
        if not den.requires_grad:                    # a degradation that does not depend on x_hat: the reference's autograd.grad raises as well
            raise RuntimeError("degradation(x_hat) does not depend on x_hat: reconstruction guidance has no gradient")
        (gx,) = torch.autograd.grad(den, leaf, g.reshape(den.shape).to(den.dtype))
        return gx.float().contiguous()

    def project(self, x, y):
        raise AttributeError("proj_convex_set is undefined for predict_resample (the reference defines it in predict_inpainting / "
                             "predict_spectrogram_inpainting only): set tester.data_consistency.use = False")


def as_operator(degradation):
    """An operator object (anything with ``apply`` and ``adjoint``: stft.SpectralMask, degrade.FIRFilter, ...) is installed as it is;
    any other callable goes through LambdaDegradation."""
    if hasattr(degradation, "apply") and hasattr(degradation, "adjoint"):
        return degradation
    return LambdaDegradation(degradation)


def phase_retrieval_sizes(args):
    """(win_size, hop_size) of phase retrieval: args.inference.phase_retrieval (where the reference reads them, edm_sampler.py:326-327)
    when the config has it, else args.tester.phase_retrieval (where the shipped conf/tester yaml puts them)."""
    node = getattr(getattr(args, "inference", None), "phase_retrieval", None)
    if node is None:
        node = getattr(args.tester, "phase_retrieval", None)
    if node is None:
        raise _lib.AidError("predict_pr: no phase_retrieval config (args.inference.phase_retrieval or args.tester.phase_retrieval)")
    return node.win_size, node.hop_size


def autoregressive_overlap(args):
    """Overlap fraction of autoregressive generation: args.inference.autoregressive.overlap (where the reference reads it, edm_sampler.py:391)
    when the config has it, else args.tester.autoregressive.overlap (where the shipped conf/tester yaml puts it)."""
    node = getattr(getattr(args, "inference", None), "autoregressive", None)
    if node is None:
        node = getattr(args.tester, "autoregressive", None)
    if node is None:
        raise _lib.AidError("predict_autoregressive: no autoregressive config (args.inference.autoregressive or args.tester.autoregressive)")
    return node.overlap


def autoregressive_length(L: int, end: int, N: int) -> int:
    """Samples produced by N windows of L samples that share ``end`` samples with their predecessor (hard concatenation, edm_sampler.py:416)."""
    return L + (N - 1) * (L - end)


class Sampler:
    def __init__(self, model, diff_params, args, rid=False):
        self.model = model
        self.diff_params = diff_params
        self.args = args
        if not self.args.tester.diff_params.same_as_training:
            self.update_diff_params()
        self.order = self.args.tester.order
        self.xi = self.args.tester.posterior_sampling.xi
        dc = self.args.tester.data_consistency
        self.data_consistency = dc.use and dc.type == "always"
        self.data_consistency_end = dc.use and dc.type == "end"
        if self.data_consistency or self.data_consistency_end:
            self.smooth = bool(dc.smooth)
        self.nb_steps = self.args.tester.T
        self.rid = rid                              # True: predict_* return the reference's 8-tuple of per-step buffers (:185-191, :260)
        self.spectral = None
        self.y = self.mask = self.smask = self.degradation = None      # installed by predict_* / setup_*
        self.seeds: Optional[List[int]] = None      # per-item RNG seeds; None -> global torch CPU generator
        self._gens = None                           # the per-item generators of the run in progress (begin)
        self._keep_gens = False                     # predict_autoregressive: begin() keeps the generators the run already made
        self.trace = None                           # set to [] to record every projected x_hat (tests)
        self.trace_in = None                        # set to [] to record (x, t) handed to every denoiser evaluation (teacher-forced tests)
        self.n_evals = 0

    def update_diff_params(self):
        dp, tp = self.diff_params, self.args.tester.diff_params
        dp.sigma_min, dp.sigma_max, dp.ro, dp.sigma_data = tp.sigma_min, tp.sigma_max, tp.ro, tp.sigma_data
        dp.Schurn, dp.Stmin, dp.Stmax, dp.Snoise = tp.Schurn, tp.Stmin, tp.Stmax, tp.Snoise

    # ---------------------------------------------------------------------------------------------------
    def _check_model(self):
        """The loop drives the model through the fused entry points ``denoise`` / ``denoise_guided`` of the MI355X network (network.py).
        A foreign torch model has to be wrapped explicitly: ``Sampler(model=generic.GenericModelAdapter(model, diff_params), ...)``."""
        if not (hasattr(self.model, "denoise") and hasattr(self.model, "denoise_guided")):
            raise _lib.AidError("Sampler needs a model with the fused entry points denoise / denoise_guided (the MI355X network); wrap any other "
                                "torch model in audio_inpainting_diffusion_amd.generic.GenericModelAdapter -- there is no implicit eager path")

    def _draw(self, shape, scale):
        """scale * randn(shape) from the CPU generator(s) in the reference's order (:212, edm.py:94), drawn straight into one of two
        pinned staging buffers (re-used alternately; an event guards the one still in flight) -> host tensor ready for an async copy."""
        ring = self.__dict__.setdefault("_pin_ring", {"shape": None})
        if ring["shape"] != tuple(shape):
            ring.update(shape=tuple(shape), bufs=[torch.empty(shape, dtype=torch.float32).pin_memory() for _ in range(2)], ev=[None, None], k=0)
        k = ring["k"] = ring["k"] ^ 1
        if ring["ev"][k] is not None:
            ring["ev"][k].synchronize()                   # the copy issued two draws ago (long finished; never blocks in steady state)
        buf = ring["bufs"][k]
        if self.seeds is None:
            torch.randn(shape, out=buf)
        else:
            for b, g in enumerate(self._gens):
                torch.randn([1, shape[1]], generator=g, out=buf[b:b + 1])
        if float(scale) != 1.0:
            buf.mul_(scale)
        return buf, k

    def _draw_to(self, shape, scale, device):
        buf, k = self._draw(shape, scale)
        out = buf.to(device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._pin_ring["ev"][k] = ev
        return out

    # ---- one denoiser evaluation -> projected x_hat --------------------------------------------------------
    def _scalars(self, t_i):
        """c_noise, c_in, c_skip, c_out of this evaluation as host floats, computed by diff_params in float32 torch arithmetic (edm.py:97-128)"""
        dp = self.diff_params
        s = t_i.reshape(1)
        return float(dp.cnoise(s)), float(dp.cin(s)), float(dp.cskip(s)), float(dp.cout(s))

    def _denoise(self, x, t_i):
        """x_hat = D(x; t_i) [+ guidance step] ; data-consistency projection is applied by the caller's fused
        step kernel.  t_i: 0-d float32 CPU tensor."""
        B = x.shape[0]
        self.n_evals += B
        if self.trace_in is not None:
            self.trace_in.append((x.clone(), float(t_i)))
        if self.y is not None and self.xi > 0:
            return self._denoise_guided(x, t_i)
        hpf = bool(self.y is None and self.args.tester.filter_out_cqt_DC_Nyq)   # (:122-123) unconditional only
        return self.model.denoise(x, *self._scalars(t_i), hpf)

    def _denoise_guided(self, x, t_i):
        """Reconstruction guidance (:57-105), per item: analytic seed of the chosen norm, the network's hand-written input-VJP,
        then the normalised step x_hat - t*xi/(||g||/sqrt(L) + 1e-6) * g in one launch (aid_guidance_step)."""
        B, L = x.shape
        ps = self.args.tester.posterior_sampling
        hpf = bool(self.args.tester.filter_out_cqt_DC_Nyq)
        x_hat, rec_grads, _ = self.model.denoise_guided(x, *self._scalars(t_i), hpf, self.y, self.mask, self.spectral,
                                                        norm_type=ps.norm, beta=float(getattr(ps, "smoothl1_beta", 1.0)))
        out = torch.empty_like(x_hat)
        upd = torch.empty_like(x_hat) if self.rid else None
        inv = float(np.float32(1.0) / np.float32(self.args.exp.audio_len ** 0.5))
        p = _lib.GuidanceStepParams(x_hat.data_ptr(), rec_grads.data_ptr(), out.data_ptr(), _lib.ptr(upd), None, B, L,
                                    float(t_i) * self.xi, inv, 1e-6)                # (:83, :87, :97)
        _lib.call("aid_guidance_step", p)
        if self.rid:                                                                 # (:92-99: denoised estimate, s*rec_grads, updated estimate)
            self._rid_last = (x_hat, upd, out)
        return out

    def _score_step(self, x, x_hat, t_i, h, mode, x0=None, d0=None):
        """fused: projection (:343) + d = -t*score (:105,:230) + Euler proposal (:240) or Heun combine (:247)."""
        B, L = x.shape
        xnext = torch.empty_like(x)
        dout = torch.empty_like(x) if mode == 0 else None
        # guided branch: project only with data_consistency.type == "always" (:100); replacement branch (xi == 0):
        # at EVERY evaluation whatever the type (:141-147) -- like the reference, which fails there when no projection
        # was ever defined (data_consistency.use False, :338)
        proj = self.y is not None and (self.data_consistency or self.xi == 0)
        if proj and not (self.data_consistency or self.data_consistency_end):
            raise AttributeError("proj_convex_set is undefined: the replacement branch (xi = 0) needs tester.data_consistency.use")
        if proj and self.spectral is not None:                     # y + x_hat - A(x_hat)   (:360)
            x_hat, proj = self.spectral.project(x_hat, self.y), False
        xh_out = torch.empty_like(x) if (self.trace is not None or self.rid) else None
        p = _lib.ScoreStepParams(x.data_ptr(), x_hat.data_ptr(), _lib.ptr(self.y) if proj else None,
                                 _lib.ptr(self.smask) if proj else None, (self.smask.stride(0) if self.smask.shape[0] > 1 else 0) if proj else 0,
                                 _lib.ptr(x0), _lib.ptr(d0), None, None,
                                 xnext.data_ptr(), _lib.ptr(dout), _lib.ptr(xh_out), B, L, mode, float(t_i), float(h))
        _lib.call("aid_score_step", p)
        if self.trace is not None:
            self.trace.append(xh_out)
        self._rid_pocs = xh_out
        return xnext, dout

    def _project(self, x):
        """smask * y + (1 - smask) * x (:343) by the projection stage of aid_score_step (its xh_out output; the step outputs go to scratch)."""
        B, L = x.shape
        out, scratch = torch.empty_like(x), torch.empty_like(x)
        p = _lib.ScoreStepParams(x.data_ptr(), x.data_ptr(), self.y.data_ptr(), self.smask.data_ptr(),
                                 self.smask.stride(0) if self.smask.shape[0] > 1 else 0, None, None, None, None,
                                 scratch.data_ptr(), None, out.data_ptr(), B, L, 0, 1.0, 0.0)
        _lib.call("aid_score_step", p)
        return out

    # ---------------------------------------------------------------------------------------------------
    def predict_unconditional(self, shape, device):
        self.y = self.degradation = None
        self.mask = self.smask = self.spectral = None
        return self.predict(shape, device)

    def begin(self, shape, device):
        """Draw the prior and set up the schedule; returns the loop state consumed by ``step``."""
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.AidError("the MI355X sampler runs on the GPU only (no CPU fallback)")
        self._check_model()
        dp = self.diff_params
        if self.seeds is None:
            self._gens = None
        elif not (self._keep_gens and self._gens is not None):   # (an autoregressive run carries ONE generator per item across its windows)
            self._gens = [torch.Generator().manual_seed(int(s)) for s in self.seeds]
        t = dp.create_schedule(self.nb_steps)                 # host, float32
        gamma = dp.get_gamma(t)
        x = self._draw_to(shape, t[0], device)                # prior (edm.py:94)
        return dict(x=x, t=t, gamma=gamma, shape=tuple(shape), device=device)

    def step(self, state, i: int):
        """One iteration of the sampling loop (:201-251): churn, denoiser evaluation, Heun correction."""
        dp = self.diff_params
        t, gamma, x, shape, device = state["t"], state["gamma"], state["x"], state["shape"], state["device"]
        B, L = shape
        if gamma[i] == 0:
            t_hat = t[i]
        else:
            t_hat = t[i] + gamma[i] * t[i]
            eps = self._draw_to(shape, dp.Snoise, device)
            coef = (t_hat ** 2 - t[i] ** 2) ** (1 / 2)
            xn = torch.empty_like(x)
            p = _lib.AxpbyParams(x.data_ptr(), eps.data_ptr(), xn.data_ptr(), None, None, B, L, 1.0, float(coef))
            _lib.call("aid_axpby", p)                      # x + sqrt(t_hat^2 - t_i^2) * eps   (:214)
            x = xn
        rid = state.get("rid")
        if rid is not None:
            rid["xt"][i] = x.cpu()
        x_hat = self._denoise(x, t_hat)
        h = t[i + 1] - t_hat
        x_prime, d = self._score_step(x, x_hat, t_hat, h, mode=0)
        if rid is not None:
            rid["denoised"][i], rid["grads"][i], rid["grad_update"][i] = (v.cpu() for v in self._rid_last)
            rid["pocs"][i] = self._rid_pocs.cpu()
        if t[i + 1] != 0 and self.order == 2:
            x_hat2 = self._denoise(x_prime, t[i + 1])
            x, _ = self._score_step(x_prime, x_hat2, t[i + 1], h, mode=1, x0=x, d0=d)
        else:
            x = x_prime
        if rid is not None:
            rid["xt2"][i] = x.cpu()
        state["x"] = x
        return state

    def predict(self, shape, device):
        state = self.begin(shape, device)
        if self.rid:
            if not (self.y is not None and self.xi > 0):
                raise _lib.AidError("rid=True needs the reconstruction-guidance branch (the reference unpacks its 5-tuple only there, :217)")
            state["rid"] = {k: torch.zeros((self.nb_steps,) + tuple(shape)) for k in ("denoised", "grads", "grad_update", "pocs", "xt", "xt2")}
        for i in range(self.nb_steps):
            self.step(state, i)
        x = state["x"]
        if self.data_consistency_end and self.y is not None:                     # (:252) one last projection of the final state
            x = self._project(x) if self.spectral is None else self.spectral.project(x, self.y)
        if self.rid:                                                             # (:260)
            r = state["rid"]
            return x.detach(), r["denoised"], r["grads"], r["grad_update"], r["pocs"], r["xt"], r["xt2"], state["t"]
        return x.detach()

    def setup_inpainting(self, y_masked, mask):
        """Install observations y_masked[B,L] and mask[1|B,L] (any dtype / device / strides) for the time-domain
        degradation; ``predict`` / ``begin`` + ``step`` then run the loop."""
        if mask.dim() == 1:
            mask = mask.reshape(1, -1)
        dev = y_masked.device
        self.y = y_masked.contiguous().float()
        self.mask = mask.to(dev, torch.float32).contiguous()         # read as a raw float* by aid_guidance_seed
        if self.mask.shape[-1] != self.y.shape[-1] or self.mask.shape[0] not in (1, self.y.shape[0]):
            raise ValueError(f"mask {tuple(mask.shape)} does not match observations {tuple(y_masked.shape)}")
        self.spectral = None
        self.smask = None
        self.degradation = self.apply_mask                            # (:335)
        if self.data_consistency or self.data_consistency_end:
            sm = prepare_smooth_mask(mask, self.args.tester.data_consistency.hann_size) if self.smooth else mask
            self.smask = sm.to(dev, torch.float32).contiguous()

    def predict_inpainting(self, y_masked, mask):
        """y_masked[B,L], mask[1|B,L] -> inpainted [B,L] on y_masked.device   (:327-346)"""
        self.setup_inpainting(y_masked, mask)
        return self.predict(self.y.shape, self.y.device)

    def setup_spectrogram_inpainting(self, y, mask, observed_is_clean=False):
        """Install the STFT-domain degradation (mask[F,T] or [B,F,T]).  observed_is_clean: ``y`` is the clean signal
        and the observation is A(y) (what the tester computes before calling predict_spectrogram_inpainting)."""
        st = self.args.tester.spectrogram_inpainting.stft
        y = y.contiguous().float()
        self.mask = self.smask = None
        self.spectral = SpectralMask(mask, y.shape[-1], st.n_fft, st.hop_length, st.win_length, st.window, y.device)
        self.y = self.spectral.apply(y) if observed_is_clean else y
        self.degradation = self.apply_spectral_mask                   # (:359)

    def predict_resample(self, y, shape, degradation):
        """y[B, ...] = observations, shape = (B, L) of the signal, degradation = torch callable x[B, L] -> y-shaped tensor   (:164-173): reconstruction
        guidance through an arbitrary degradation (the reference's generic entry point; its inpainting methods are special cases of it).
        An operator object with ``apply`` / ``adjoint`` (degrade.py, stft.SpectralMask, phase.STFTMagnitude) is used directly, without torch autograd."""
        if (y.dim() == 3 and self.args.tester.posterior_sampling.norm != "smoothl1" and type(self.model).__name__ != "GenericModelAdapter"
                and getattr(degradation, "matrix_obs", None) is None):       # (operators that declare matrix_obs get the induced-norm seed, phase.py)
            # (:67-70: torch.linalg.norm(y - den, dim=(1, 2), ord=norm) over 3-D observations is the INDUCED matrix norm -- ord = 2 the largest singular
            #  value, ord = 1 the largest column sum -- not the element-wise norm aid_guidance_seed computes over the flattened item)
            raise _lib.AidError("predict_resample: norm = 2 / 1 over 3-D observations is the induced matrix norm (spectral / max column sum) in the reference "
                                "(edm_sampler_inpainting.py:67-75); the HIP guidance seed implements the element-wise norms only: use norm = 'smoothl1', "
                                "flatten the observations to [B, N], or wrap the model in generic.GenericModelAdapter (torch autograd, reference semantics)")
        self.y = y.contiguous().float()
        self.mask = self.smask = None
        self.spectral = as_operator(degradation)
        self.degradation = degradation
        return self.predict(tuple(shape), self.y.device)

    def predict_conditional(self, y, degradation):
        """(edm_sampler.py:157-164) predict_resample with the signal shape y.shape"""
        return self.predict_resample(y, tuple(y.shape), degradation)

    def predict_bwe(self, ylpf, filt, filt_type):
        """Bandwidth extension (edm_sampler.py:266-300) through the native operators of degrade.py:
        "firwin" / "firwin_hpf": taps [K], [1, K] or [1, 1, K] (conv1d padding="same");  "cheby1": (b, a) (lfilter, clamp=False);
        "biquad": (b0, b1, b2, a0, a1, a2) (torchaudio's biquad, clamp=True);  "decimate": an integer factor, ylpf [B, ceil((L-1)/f)]
        with L = args.exp.audio_len;  "resample": a factor in (0, 16] -- torchaudio's default resampler from int(100 * factor) to 100
        (degrade.SincResample.from_factor: 2 -> 2:1, 1.47 -> 147:100), ylpf [B, ceil(new*L/orig)] on the GPU."""
        dev = ylpf.device
        L = ylpf.shape[-1]
        if filt_type in ("firwin", "firwin_hpf"):
            op = FIRFilter(filt, L, device=dev)
        elif filt_type == "cheby1":
            b, a = filt
            op = IIRFilter(b, a, L, clamp=False, device=dev)
        elif filt_type == "biquad":
            op = IIRFilter.biquad(*filt, audio_len=L, device=dev)
        elif filt_type == "decimate":
            op = Decimate(filt, self.args.exp.audio_len, device=dev)
            return self.predict_resample(ylpf, (ylpf.shape[0], self.args.exp.audio_len), op)
        elif filt_type == "resample":
            if not ylpf.is_cuda:
                raise _lib.AidError("predict_bwe: filt_type 'resample' is not built for CPU tensors: the resampling operator runs on the GPU only")
            op = SincResample.from_factor(filt, self.args.exp.audio_len, device=dev)
            if ylpf.dim() != 2 or ylpf.shape[1] != op.L_out:
                raise _lib.AidError(f"predict_bwe: 'resample' at factor {filt!r} ({op.orig}:{op.new}) observes [B, {op.L_out}] of the "
                                    f"{op.L} samples of args.exp.audio_len, got ylpf {tuple(ylpf.shape)}")
            return self.predict_resample(ylpf, (ylpf.shape[0], self.args.exp.audio_len), op)
        else:
            raise NotImplementedError(f"predict_bwe: unknown filt_type {filt_type!r}")
        return self.predict_conditional(ylpf, op)

    def predict_blind_bwe(self, y, frozen_taps=None):
        """Blind bandwidth extension (blind.py): y [B, L = args.exp.audio_len] on the GPU went through an UNKNOWN zero-phase low-pass -> x [B, L].
        One predict_resample through blind.BlindLowpass, which fits a one-knee low-pass per item to the current estimate inside every guided
        evaluation (statistics, fit, filter: three launches, no host round trip) and guides through the taps it found.  Afterwards
        ``blind_fit`` [B, 2] holds the cut-off in Hz and the slope in dB per octave of the last evaluation, ``blind_taps`` [B, K] its taps and
        ``blind_operator`` the operator.  Settings: args.tester.blind_bwe where the config has it (n_fft, hop, K, floor_dB, k_lo, eps, cutoffs,
        slopes), else the defaults of blind.py.  ``frozen_taps`` [B, K] or [K]: no fit, guidance through these taps (equal rows: predict_bwe
        "firwin" bit for bit).  Guidance only -- xi > 0, data consistency off, rid False -- checked before anything is installed.  A whole
        recording goes through predict_blind_bwe_long, which fits one filter per recording pooled over several of its windows."""
        from . import blind
        if self.rid:
            raise _lib.AidError("predict_blind_bwe returns the restored segments only: rid must be False")
        if not self.xi > 0:
            raise _lib.AidError("predict_blind_bwe needs reconstruction guidance: tester.posterior_sampling.xi must be > 0 (the filter is fitted inside "
                                "the guided evaluation)")
        if self.data_consistency or self.data_consistency_end:
            raise _lib.AidError("predict_blind_bwe runs without data consistency (a projection onto the consistent set of an estimated filter is not a "
                                "projection onto the data): set tester.data_consistency.use = False")
        cfg = blind.settings_of(self.args)
        L = int(self.args.exp.audio_len)
        if not (torch.is_tensor(y) and y.dtype == torch.float32 and y.dim() == 2 and y.shape[0] >= 1 and y.shape[1] == L):
            raise _lib.AidError(f"predict_blind_bwe: y must be float32 [B, {L}] (args.exp.audio_len samples), got "
                                f"{tuple(y.shape) if torch.is_tensor(y) else type(y).__name__}")
        if frozen_taps is not None:
            frozen_taps = blind.frozen_rows(frozen_taps, y.shape[0], cfg.K)
        if not y.is_cuda:
            raise _lib.AidError("predict_blind_bwe runs on the GPU only (no CPU fallback): y must be a float32 tensor on the GPU")
        self._check_model()
        y = y.contiguous()
        op = blind.BlindLowpass(y, cfg, taps=frozen_taps, frozen=frozen_taps is not None)
        op.log = self.blind_log
        self.blind_operator = op
        x = self.predict_resample(y, tuple(y.shape), op)
        self.blind_taps = op.taps
        self.blind_fit = blind.fit_in_hz(op.fit, cfg, self.args.exp.sample_rate)
        return x

    blind_log = None            # set to [] before predict_blind_bwe to record (taps, fit) of every evaluation (blind.BlindLowpass.log)
    blind_fit = blind_taps = blind_operator = None

    def predict_declipping(self, y_clipped, clip_value):
        """(SamplerDeclipping.predict_declipping, edm_sampler.py:370-385) guidance through hard clipping at +-clip_value; the reference
        asserts data consistency off -- with tester.data_consistency.use the first projection raises."""
        return self.predict_conditional(y_clipped, HardClip(clip_value))

    def predict_pr(self, y):
        """Phase retrieval (SamplerPhaseRetrieval.predict_pr, edm_sampler.py:308-335): y [B, F, T] = |STFT| of the signal (win_size zeros
        appended, periodic Hamming window, center=False), signal shape (B, args.exp.audio_len), through phase.STFTMagnitude.  win_size /
        hop_size from args.inference.phase_retrieval when present, else args.tester.phase_retrieval.  The reference asserts xi > 0."""
        if not self.xi > 0:
            raise _lib.AidError("predict_pr needs reconstruction guidance: tester.posterior_sampling.xi must be > 0 (the reference asserts xi > 0)")
        win, hop = phase_retrieval_sizes(self.args)
        L = int(self.args.exp.audio_len)
        F, T = observation_shape(win, hop, L)
        if y.dim() != 3 or tuple(y.shape[1:]) != (F, T):
            raise _lib.AidError(f"predict_pr: y must be [B, {F}, {T}] (|STFT| with win_size {win}, hop_size {hop} of {L} samples), got {tuple(y.shape)}")
        return self.predict_resample(y, (y.shape[0], L), STFTMagnitude(win, hop, L, device=y.device))

    def predict_compsens(self, y_masked, mask):
        """Compressed sensing (SamplerCompSens.predict_compsens, edm_sampler.py:337-357): reconstruction from the few samples a mask keeps
        (masks.compsens_mask).  The operator is inpainting's time-domain mask; the contract is guidance only -- the reference asserts
        xi > 0 and data consistency off (:341-342) -- and is checked before anything is installed."""
        if not self.xi > 0:
            raise _lib.AidError("predict_compsens needs reconstruction guidance: tester.posterior_sampling.xi must be > 0 (the reference asserts xi > 0)")
        if self.data_consistency or self.data_consistency_end:
            raise _lib.AidError("predict_compsens runs without data consistency (the reference asserts data_consistency == False): "
                                "set tester.data_consistency.use = False")
        return self.predict_inpainting(y_masked, mask)

    def ar_carry(self, x, end, y, out, off, first):
        """One aid_ar_carry launch on the current stream: y[B, L] (or None) := the last ``end`` samples of window x[B, L], then zeros;
        out[:, off:off + L - skip] := x[:, skip:], skip = 0 for the first window, ``end`` after it (include/aid_autoregressive.h)."""
        B, L = x.shape
        for t in (x, out) + (() if y is None else (y,)):
            _lib._req(t)
        if not (x.is_contiguous() and out.dim() == 2 and out.stride(1) == 1 and out.shape[0] == B and (y is None or (y.is_contiguous() and y.shape == x.shape))):
            raise _lib.AidError("ar_carry: x / y contiguous [B, L], out [B, >= off + L - skip] with contiguous rows")
        if off + L - (0 if first else end) > out.shape[1]:
            raise _lib.AidError("ar_carry: the appended part does not fit into out")
        _lib.call("aid_ar_carry", _lib.ArCarryParams(x.data_ptr(), _lib.ptr(y), out.data_ptr(), B, int(bool(first)), L, int(end), int(off), out.stride(0)))

    def predict_autoregressive(self, shape, N, device):
        """Autoregressive generation (SamplerAutoregressive.predict_autoregressive, edm_sampler.py:386-418): a piece of N windows, longer than one
        model segment.  Window 0 is sampled unconditionally; every later window is inpainted (as predict_inpainting does it: guidance, and the
        projection tester.data_consistency configures) with its first end = int(overlap * L) samples observed -- the tail of the window before it.
        shape = (B, L) with L = args.exp.audio_len -> [B, L + (N - 1) * (L - end)] on ``device`` (hard concatenation, as the reference).
        The B pieces advance together; between two windows ONE aid_ar_carry launch writes the next observations and appends to the result, which
        never leaves the GPU.  RNG: seeds None -> the global CPU generator in the reference's order (prior, churn draws, next prior, ...);
        seeds [...] -> item b owns one generator for the WHOLE piece, so it equals the B = 1 run with seeds [seeds[b]]."""
        B, L = (int(v) for v in shape)
        N = int(N)
        if self.rid:
            raise _lib.AidError("predict_autoregressive returns the piece only: rid must be False (the reference asserts rid == False)")
        if N < 1:
            raise _lib.AidError(f"predict_autoregressive: N must be >= 1, got {N}")
        if L != int(self.args.exp.audio_len):
            raise _lib.AidError(f"predict_autoregressive: shape[-1] = {L} must equal args.exp.audio_len = {self.args.exp.audio_len} "
                                "(the reference builds the mask with audio_len and indexes it with shape[-1])")
        end = int(autoregressive_overlap(self.args) * L)
        if end < 1 or end >= L:
            raise _lib.AidError(f"predict_autoregressive: int(overlap * L) = {end} must lie in [1, L - 1]")
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.AidError("the MI355X sampler runs on the GPU only (no CPU fallback)")
        self._check_model()
        if N == 1:
            return self.predict_unconditional((B, L), device)
        step = L - end
        out = torch.empty((B, autoregressive_length(L, end, N)), dtype=torch.float32, device=device)
        y = torch.empty((B, L), dtype=torch.float32, device=device)
        mask = torch.ones((1, L))
        mask[:, end:] = 0
        self._gens, self._keep_gens = None, True
        try:
            x = self.predict_unconditional((B, L), device)
            self.ar_carry(x, end, y, out, 0, True)
            self.setup_inpainting(y, mask)                    # once: mask and smoothed mask do not change; y is refilled in place by the carry
            for w in range(1, N):
                x = self.predict((B, L), device)
                self.ar_carry(x, end, y if w < N - 1 else None, out, L + (w - 1) * step, False)
        finally:
            self._keep_gens = False
        return out

    def _long_grid(self, who: str, what: str = "restored", consistency: Optional[str] = None):
        """(L, end) of the window grid of the predict_*_long methods, after the refusals they share: rid, and -- for an operator without a
        projection, ``consistency`` saying why -- tester.data_consistency in use."""
        if self.rid:
            raise _lib.AidError(f"{who} returns the {what} recordings only: rid must be False")
        if consistency and (self.data_consistency or self.data_consistency_end):
            raise _lib.AidError(f"{who} runs without data consistency ({consistency}): set tester.data_consistency.use = False")
        L = int(self.args.exp.audio_len)
        return L, int(autoregressive_overlap(self.args) * L)

    def _long(self, name, groups, max_batch, seeds, **call_args):
        """Run the whole-recording mode ``name`` (its record in restore.LONG_TASKS) over ``groups``, one set of equal-length recordings each
        -> one result per group.  What every predict_*_long method and predict_long_pooled are: the refusals of ``_long_grid``, the refusal
        of xi <= 0 where the mode is guided only, the record's ``prepare`` of what the groups share, then restore.run_task -- every group
        checked, ``_check_model``, every group built, the pooled passes.  All refusals are raised before anything is launched."""
        task = restore.LONG_TASKS[name]
        L, end = self._long_grid(task.method, task.what, task.consistency)
        if task.guided and not self.xi > 0:
            raise _lib.AidError(f"{task.method} needs reconstruction guidance: tester.posterior_sampling.xi must be > 0 ({task.guided})")
        return restore.run_task(task, self, task.prepare(self.args, **call_args), groups, L, end, max_batch, seeds, ready=self._check_model)

    def predict_inpainting_long(self, y, mask, max_batch=8, seeds=None):
        """Restore whole recordings y[R, N] -- N any length, gaps wherever mask[1|R, N] is 0 -> [R, N] on y.device (restore.py).  Windows of
        L = args.exp.audio_len samples on the autoregressive grid (end = int(overlap * L) shared samples, 1 <= end < L/2); the even windows that
        hold a gap are inpainted as one batch, then the odd ones, conditioned on their neighbours' restored overlaps: two rounds of
        predict_inpainting in chunks of at most ``max_batch`` windows, one aid_window_gather launch per round and one aid_window_scatter launch per
        chunk.  Windows without a gap cost nothing; samples outside every gap's window stay the recording's.  ``seeds`` [R]: window w of recording
        r runs with seed seeds[r] * 65536 + w, so a recording's result depends neither on the other recordings nor on max_batch.
        Under an active process group (dist._active(); call dist.broadcast_parameters first, so that the ranks hold the same weights) every rank
        calls with the same y, mask and seeds and gets the full [R, N]: rank k runs dist.shard_range of each round's windows in chunks of at most
        ``max_batch`` (per rank), one dist.gather_outputs per round brings all windows to every rank, and each rank scatters the whole round
        (restore.run_passes).  ``seeds`` = None is then refused, and ranks that were given different work raise before anything is launched."""
        return self._long("inpainting", [(y, mask)], max_batch, seeds)[0]

    def predict_declicking_long(self, y, max_batch=8, seeds=None, mask=None, **settings):
        """Declick whole recordings y[R, N] on the GPU -- N any length, clicks and short dropouts at unknown places -> [R, N] (declick.py).
        A front end of predict_inpainting_long, not a task of its own: declick.detect finds the damage (two launches and one read-back of the
        mask; settings: declick.settings_of(args), overridden by ``settings``), the detected mask is multiplied by ``mask`` ([N], [1, N] or
        [R, N]; known gaps, 1 = observed) when one is given, and the result is predict_inpainting_long(y, that mask, max_batch, seeds) --
        its refusals, grid, seeds and behaviour under a process group, word for word.  Before that call a recording of which more than
        ``max_fraction`` is masked is refused, by its index.  With nothing flagged the result is a copy of y and no evaluation runs.
        Afterwards ``declick_report`` holds the declick.Detection without the score plane: the mask that was restored, its counts (known
        gaps included when ``mask`` was given) and the detector's sigma.  Under a process group every rank detects for itself: the detector is deterministic, nothing is exchanged."""
        from . import declick
        cfg = declick.settings_of(self.args, **settings)
        det = declick.detect(y, **cfg._asdict())
        m = declick.combine(det.mask, mask)
        if mask is not None:                                                     # (the report describes the mask that is restored)
            det = declick.Detection(m, det.score, det.sigma, *declick.report_of(m))
        declick.check_fraction(det.n_flagged.tolist(), m.shape[1], cfg.max_fraction)
        self.declick_report = det._replace(score=None)
        return self.predict_inpainting_long(y, m, max_batch, seeds)

    declick_report = None       # after predict_declicking_long: the declick.Detection of the call, without its score plane

    def predict_declipping_long(self, y, clip_value, max_batch=8, seeds=None):
        """Declip whole recordings y[R, N] -- N any length, clipped at +-clip_value (a float, or R floats: one level per recording; rounded to
        float32 as HardClip does) -> [R, N] on y.device (declip_long.py).  The window grid, the two batched passes and the seeds are those of
        predict_inpainting_long; a window is a job when its owned range holds a sample with |y| >= c.  Each chunk of at most ``max_batch`` windows
        is one predict_resample through declip_long.ClipObserved, which sees the recording through the clipper and takes the overlaps its
        neighbours restored as known.  tester.data_consistency off: guidance only, as the reference's declipping; "always" / "end": the
        projection onto the signals consistent with the clipped recording at every evaluation / once on the final state.  Windows without a
        clipped sample cost nothing and keep the recording's samples.
        Under an active process group the windows of each pass are shared out over the ranks as predict_inpainting_long states: the same
        arguments and weights (dist.broadcast_parameters) on every rank, ``seeds`` required, ``max_batch`` per rank, the full result on every rank."""
        return self._long("declipping", [(y, clip_value)], max_batch, seeds)[0]

    def predict_bwe_long(self, y, filt, filt_type, max_batch=8, seeds=None):
        """Bandwidth-extend whole recordings y[R, N] -- N any length, low-passed as a whole with the FIR taps ``filt`` ([K], [1, K] or [1, 1, K],
        conv1d padding="same", as predict_bwe takes them) -> [R, N] on y.device (bwe_long.py).  filt_type "firwin" / "firwin_hpf" only: an IIR
        filter ("cheby1", "biquad") carries state from the start of the recording and a decimator's phase ("decimate", "resample") depends on
        the window start, so neither windows here; they are refused (an IIR-filtered recording goes through predict_bwe_iir_long, which seeds
        the recursion of every window from the recording).  The window grid, the two batched passes and the seeds are those of
        predict_inpainting_long, with every window a job and the ownership trimmed by K - 1 samples (more than one window needs
        end = int(overlap * L) >= 2 (K - 1)).  Each chunk of at most ``max_batch`` windows is one predict_resample through bwe_long.FIRObserved,
        which uses a filtered sample as an observation only where the window holds its whole filter support and takes the overlaps its
        neighbours restored as known.  tester.data_consistency off / "end" / "always" mean what they mean for predict_bwe.  A recording that
        exists only at a low sample rate ("decimate", "resample") goes through predict_bwe_lowrate_long, whose grid is aligned to the input period.
        Under an active process group the windows of each pass are shared out over the ranks as predict_inpainting_long states: the same
        arguments and weights (dist.broadcast_parameters) on every rank, ``seeds`` required, ``max_batch`` per rank, the full result on every rank."""
        return self._long("bwe", [(y,)], max_batch, seeds, filt=filt, filt_type=filt_type)[0]

    def predict_blind_bwe_long(self, y, probes=4, max_batch=8, seeds=None, frozen_taps=None):
        """Blind bandwidth extension of whole recordings y[R, N] -- N any length, each low-passed as a whole by an UNKNOWN zero-phase low-pass
        of its own -> [R, N] on y.device (blind_long.py).  Two stages, both through predict_resample.  Stage 1 fits ONE filter per recording:
        its ``probes`` windows of largest energy among the windows of predict_bwe_long's grid that lie wholly inside it (one aid_window_energy
        launch, read back once; window 0 when N < L) are sampled in chunks of whole recordings of at most ``max_batch`` probes through
        blind_long.PooledBlindLowpass, which in every guided evaluation fits one low-pass to the band statistics of all probes of a recording
        together (statistics, pooled fit, filter: three launches, no host round trip; on one stream); nothing carries over between evaluations
        and the probes' restorations are discarded.  Stage 2 is predict_bwe_long -- the grid, the ownership trimmed by K - 1 (more than one
        window needs end = int(overlap * L) >= 2 (K - 1)), the two batched passes, the seeds -- with the taps fitted for a window's recording
        (blind_long.FIRObservedRows).  Afterwards ``blind_fit`` [R, 2] holds the cut-off in Hz and the slope in dB per octave of every
        recording, ``blind_taps`` [R, K] its taps and ``blind_probes`` per recording the starts of the windows that were fitted on.  Settings:
        blind.settings_of(args), as predict_blind_bwe.  ``frozen_taps`` [K] or [R, K]: stage 1 is skipped entirely (no launch, no sampler
        call) and the result is predict_bwe_long's with those taps, bit for bit.  Guidance only -- xi > 0, data consistency off, rid False.
        ``seeds`` [R]: window w of recording r runs with seeds[r] * 65536 + w, its probe p with seeds[r] * 65536 + 65535 - p, so a recording's
        filter and result depend neither on the other recordings nor on max_batch.  There is no ``pool`` argument: recordings of different
        lengths are calls of their own.
        Under an active process group every rank calls with the same y and seeds (required) and gets the full result: rank k estimates the
        recordings dist.shard_range(R, k, world), one dist.gather_outputs brings all filters to every rank, and stage 2 shares the windows of
        each pass out as predict_inpainting_long states."""
        from . import blind, blind_long
        L, end = self._long_grid("predict_blind_bwe_long", consistency=blind_long.NO_PROJECTION)
        if not self.xi > 0:
            raise _lib.AidError("predict_blind_bwe_long needs reconstruction guidance: tester.posterior_sampling.xi must be > 0 (the filter is fitted "
                                "inside the guided evaluation)")
        cfg = blind.settings_of(self.args)
        blind_long.check_blind_long_args(y, cfg, L, end, probes, max_batch, seeds, frozen_taps)
        self._check_model()
        out, taps, fit, starts = blind_long.blind_bwe_long_passes(self, y, cfg, L, end, probes, max_batch, seeds, frozen_taps)
        self.blind_taps, self.blind_fit, self.blind_probes = taps, blind.fit_in_hz(fit, cfg, self.args.exp.sample_rate), starts
        return out

    blind_probes = None         # after predict_blind_bwe_long: per recording, the starts of the windows its filter was fitted on

    def predict_bwe_iir_long(self, y, filt, filt_type, max_batch=8, seeds=None):
        """Bandwidth-extend whole recordings y[R, N] -- N any length, low-passed as a whole with an IIR filter from a zero state -> [R, N] on
        y.device (bwe_iir_long.py).  filt_type "cheby1": filt = (b, a), as predict_bwe takes them (lfilter, clamp=False); "biquad":
        (b0, b1, b2, a0, a1, a2).  The coefficients are those of degrade.iir_coefficients (order <= 16) under IIRFilter's conditioning refusal.
        The window grid, the two batched passes, the seeds, the refusal of rid and the behaviour under a process group are those of
        predict_bwe_long with K - 1 = order (more than one window needs end = int(overlap * L) >= 2 order).  A window that does not start the
        recording takes its first ``order`` filtered samples as the initial state of the recursion instead of as observations, so from there
        on the window operator (bwe_iir_long.IIRObserved) does the recording's own arithmetic on the recording's own numbers; the float32
        rounding of those seeds moves a filtered sample by at most IIRObserved.seed_error_bound = order * amplification * 2^-24 of max|y|.
        tester.data_consistency off / "end" / "always" mean what they mean for predict_bwe "cheby1".
        "biquad" DEPARTS from predict_bwe "biquad": torchaudio clamps the filtered signal to [-1, 1]; here a recording with a sample |y| >= 1 is
        refused (the clamp acted, the recording no longer satisfies the recursion) and the window operator is the linear filter, whereas
        predict_bwe "biquad" also drops the gradient where the model's own filtered estimate leaves [-1, 1]."""
        return self._long("bwe_iir", [(y,)], max_batch, seeds, filt=filt, filt_type=filt_type)[0]

    def predict_bwe_declip_long(self, y, filt, filt_type, clip_value=None, mask=None, max_batch=8, seeds=None):
        """Bandwidth-extend whole recordings y[R, N] that are also clipped and have dropouts -- N any length -> [R, N] on y.device
        (bwe_declip_long.py).  The degradation model, applied to the recording as a whole, is y = mask * clamp(taps * x, -c_r, +c_r), in this
        order and no other: low-passed with the FIR taps ``filt`` ("same" padding, as predict_bwe_long; filt_type "firwin" / "firwin_hpf" only,
        the others are refused for predict_bwe_long's reasons), THEN clipped at +-clip_value (a float, or R floats: one level per recording, as
        predict_declipping_long; None: not clipped, carried as a level of +inf), THEN dropped where mask ([N], [1, N] or [R, N]; 1 = kept,
        0 = dropped; None: all ones) is 0.  The window grid, the ownership, the two batched passes and the seeds are those of predict_bwe_long
        (every window a job; more than one window needs end = int(overlap * L) >= 2 (K - 1)).  Each chunk of at most ``max_batch`` windows is one
        predict_resample through bwe_declip_long.FIRClipObserved, which sees a filtered sample through the clipper where the window holds its
        whole filter support, takes a dropped sample as unobserved (it still feeds its neighbours' filter sums) and the overlaps its neighbours
        restored as known.  With clip_value = None and mask = None the result is predict_bwe_long's, bit for bit.
        Guidance only: rid and tester.data_consistency in use are refused (no projection exists for the clipped filter).  A recording with a
        window that holds neither a filtered nor a known sample -- a dropout that swallows a whole window -- is refused before anything is
        launched, naming the recording and the window.
        Under an active process group the windows of each pass are shared out over the ranks as predict_inpainting_long states: the same
        arguments and weights (dist.broadcast_parameters) on every rank, ``seeds`` required, ``max_batch`` per rank, the full result on every rank."""
        return self._long("bwe_declip", [(y, clip_value, mask)], max_batch, seeds, filt=filt, filt_type=filt_type)[0]

    def predict_bwe_lowrate_long(self, y, factor, filt_type="resample", length=None, max_batch=8, seeds=None):
        """Bandwidth-extend whole recordings that exist only at a low sample rate: y[R, M] on the GPU -> [R, N] at the high rate, N any length
        (lowrate_long.py).  filt_type "resample": torchaudio's default resampler at degrade.bwe_resample_ratio(factor), as predict_bwe's
        (2 -> 2:1, 1.47 -> 147:100); "decimate": every factor-th sample (an integer in [1, 16]; the reference's 0:-1:factor).  ``length`` is N; it
        must be consistent with M, and defaults to the largest such N (resample: floor(M * orig / new); decimate: M * factor + 1).  The window
        grid, the two batched passes and the seeds are those of predict_bwe_long with K = 2 * width + orig, after the overlap
        end = int(overlap * L) is widened to end' = end + ((L - end) % orig): every window then starts at a multiple of the input period and
        resamples to the recording's own low-rate samples (more than one window needs end' >= 2 (K - 1); 2 end' < L).  Each chunk of at most
        ``max_batch`` windows is one predict_resample through lowrate_long.RateObserved, which observes [B, L + ceil(new * L / orig)] entries
        per window: the overlaps its neighbours restored as known, and the low-rate samples whose whole kernel support the window holds.
        Guidance only: an identity ratio, rid and tester.data_consistency in use are refused (the reference's y + x - A(x) is undefined for an
        operator that changes the length).
        Under an active process group the windows of each pass are shared out over the ranks as predict_inpainting_long states: the same
        arguments and weights (dist.broadcast_parameters) on every rank, ``seeds`` required, ``max_batch`` per rank, the full result on every rank."""
        return self._long("bwe_lowrate", [(y, length)], max_batch, seeds, factor=factor, filt_type=filt_type)[0]

    def predict_pr_long(self, y, length=None, max_batch=8, seeds=None):
        """Retrieve the phase of whole recordings known only by their STFT magnitude: y[R, F, T_rec] on the GPU (|STFT| as predict_pr takes it:
        win_size zeros appended, periodic Hamming window, center=False; F = win_size / 2 + 1, T_rec = 1 + N // hop_size) -> [R, N], N any length
        (phase_long.py).  win_size / hop_size as for predict_pr (phase_retrieval_sizes).  ``length`` is N; it must be consistent with T_rec, and
        defaults to the largest such N (T_rec * hop_size - 1).  The window grid, the two batched passes and the seeds are those of
        predict_inpainting_long with the ownership trimmed by win_size - 1, after the overlap end = int(overlap * L) is widened to
        end' = end + ((L - end) % hop_size): every window then starts on the hop grid and its frames are the recording's own (more than one window
        needs end' >= 2 (win_size - 1); 2 end' < L).  Each chunk of at most ``max_batch`` windows is one predict_resample through
        phase_long.STFTMagObserved, which observes [B, L + F * (1 + L // hop_size)] entries per window: the overlaps its neighbours restored as
        known, and the magnitude columns of the frames that lie inside the window (or over the end of the recording).
        THE NORM DIFFERS FROM predict_pr: the operator declares no matrix_obs, so tester.posterior_sampling.norm = 2 / 1 is the element-wise norm
        over the whole observation row, not the induced matrix norm of one segment's spectrogram that the reference's dim=(1, 2) gives predict_pr --
        an induced matrix norm has no meaning across windows, and known samples do not fit in the matrix.
        Guidance only: xi <= 0, rid and tester.data_consistency in use are refused.
        Under an active process group the windows of each pass are shared out over the ranks as predict_inpainting_long states: the same
        arguments and weights (dist.broadcast_parameters) on every rank, ``seeds`` required, ``max_batch`` per rank, the full result on every rank."""
        return self._long("pr", [(y, length)], max_batch, seeds)[0]

    def predict_spectrogram_inpainting_long(self, y, mask, max_batch=8, seeds=None):
        """Restore whole recordings whose spectrogram was masked: y[R, N] on the GPU -- N any length, y = the reference's apply_spectral_mask of
        the whole recording -- and mask[F, T_rec] or [R, F, T_rec] over the STFT of tester.spectrogram_inpainting.stft (F = n_fft / 2 + 1,
        T_rec = 1 + Np // hop_length, Np = N + (n_fft - N % n_fft): masks.spectral_mask(audio_len=N, ...)) -> [R, N] (spec_long.py).  The window
        grid, the two batched passes and the seeds are those of predict_inpainting_long with the ownership trimmed by 2 (n_fft - 1), after the
        overlap end = int(overlap * L) is widened to end' = end + ((L - end) % hop_length): every window then starts on the hop grid and its
        frames are the recording's own (more than one window needs end' >= 4 (n_fft - 1); 2 end' < L).  A window is a job when its owned range
        holds a sample under a frame with a masked bin; the others cost nothing and keep the recording's samples.  Each chunk of at most
        ``max_batch`` windows is one predict_resample through spec_long.SpectralMaskObserved, which uses a sample of y as an observation only
        where the window can compute every frame that covers it, and takes the overlaps its neighbours restored as known.
        tester.data_consistency off / "end" / "always" mean what they mean for predict_spectrogram_inpainting.  A window other than "hann", a
        hop_length that does not divide n_fft and rid are refused.
        Under an active process group the windows of each pass are shared out over the ranks as predict_inpainting_long states: the same
        arguments and weights (dist.broadcast_parameters) on every rank, ``seeds`` required, ``max_batch`` per rank, the full result on every rank."""
        from . import spec_long
        L, end = self._long_grid("predict_spectrogram_inpainting_long")
        st = self.args.tester.spectrogram_inpainting.stft
        spec_long.check_spec_args(y, mask, st.n_fft, st.hop_length, st.win_length, st.window, L, end, max_batch, seeds)
        self._check_model()
        return spec_long.spec_passes(self, y, mask, st.n_fft, st.hop_length, L, end, st.win_length, st.window, max_batch, seeds)

    POOLED_TASKS = ("inpainting", "declipping", "bwe", "bwe_iir", "bwe_declip", "bwe_lowrate", "pr")

    def predict_long_pooled(self, task, groups, max_batch=8, seeds=None, **task_args):
        """Whole recordings of DIFFERENT lengths in shared passes: ``task`` is "inpainting", "declipping", "bwe", "bwe_iir", "bwe_declip", "bwe_lowrate" or "pr", and every
        entry of ``groups`` is what the matching predict_*_long takes for one set of equal-length recordings -- (y, mask), (y, clip_value), y, y,
        (y, clip_value, mask), (y, length) and (y, length); a bare tensor is (y,) and a missing entry None.  ``task_args`` are the arguments all groups share:
        ``filt``, ``filt_type`` for "bwe", "bwe_iir" and "bwe_declip"; ``factor``, ``filt_type`` = "resample" for "bwe_lowrate".  -> one [R_g, N_g] per group, in order.
        The even windows of ALL groups run as one pooled pass in chunks of at most ``max_batch``, then the odd ones (restore.run_pooled_passes):
        a chunk may hold windows of several recordings and lengths, so a folder of short files runs at the sampler's full-batch rate.
        ``seeds``: one per recording, over all groups in order; the window w of a recording runs with seed * 65536 + w as in the plain
        methods, so with seeds every group's result is what its predict_*_long call returns.  Each group is checked exactly as by the plain
        method, all groups before anything is launched.
        "spectrogram_inpainting" is refused: aid_stft_mask_observed reads one recording-shaped mask in place, so masks of different T_rec
        cannot share a launch.
        Under an active process group the pooled windows of each pass are shared out over the ranks (one guard over all groups, one exchange
        per pass); ``seeds`` is then required."""
        if task == "spectrogram_inpainting":
            raise _lib.AidError("predict_long_pooled does not cover spectrogram inpainting: aid_stft_mask_observed reads one recording-shaped "
                                "mask [F, T_rec] in place, so the windows of recordings with different T_rec cannot share a launch "
                                "(call predict_spectrogram_inpainting_long per length)")
        if task not in self.POOLED_TASKS:
            raise NotImplementedError(f"predict_long_pooled: unknown task {task!r} (one of {', '.join(self.POOLED_TASKS)})")
        allowed = restore.LONG_TASKS[task].call_args
        if set(task_args) - set(allowed) or any(v is restore.REQUIRED and k not in task_args for k, v in allowed.items()):
            raise TypeError(f"predict_long_pooled({task!r}) takes the task arguments ({', '.join(allowed)}), got ({', '.join(task_args)})")
        return self._long(task, groups, max_batch, seeds, **{**allowed, **task_args})

    # ---- the remaining public methods of the reference class (its testers never call them; kept so that code written against
    # ---- testing.edm_sampler_inpainting.Sampler finds every name).  They run outside the sampling loop. ------------------------------
    def apply_mask(self, x, mask=None):
        """mask * x   (:264-269)"""
        m = self.mask if mask is None else mask
        return m.to(x.device, x.dtype) * x

    def apply_spectral_mask(self, x):
        """STFT -> mask -> inverse STFT of the installed spectrogram mask (:271-292), on the HIP STFT kernels (stft.SpectralMask)."""
        if not isinstance(self.spectral, SpectralMask):
            raise AttributeError("apply_spectral_mask: no spectrogram mask installed (predict_spectrogram_inpainting / setup_spectrogram_inpainting)")
        return self.spectral.apply(x.contiguous().float())

    def prepare_smooth_mask(self, mask, size=10):
        """(:302-325) as a method, like the reference's"""
        return prepare_smooth_mask(mask if mask.dim() > 1 else mask.reshape(1, -1), size)

    def proj_convex_set(self, x):
        """The data-consistency projection installed by predict_inpainting (:343) / predict_spectrogram_inpainting (:360); AttributeError when
        none was (the reference's attribute does not exist then)."""
        if self.y is None or not (self.data_consistency or self.data_consistency_end):
            raise AttributeError("proj_convex_set is undefined: needs observations and tester.data_consistency.use")
        x = x.detach().contiguous().float()
        return self._project(x) if self.spectral is None else self.spectral.project(x, self.y)

    def get_score(self, x, y, t_i, degradation=None):
        """ONE evaluation of the score (x_hat - x) / t_i^2 exactly as the loop forms it (:115-153): unconditional for y None (DC/Nyquist projector
        only), reconstruction guidance for xi > 0, replacement + projection for xi == 0.  ``y`` / ``degradation`` other than the installed ones are
        installed for this call (an operator object as it is, any other callable through LambdaDegradation).  With rid=True the guided branch returns the reference's
        5-tuple (score, denoised estimate, s * rec_grads, estimate after the guidance step, estimate after the projection; :106-108)."""
        t = torch.as_tensor(t_i, dtype=torch.float32).detach().reshape(()).cpu()
        x = x.detach().contiguous().float()
        B, L = x.shape
        saved = (self.y, self.mask, self.smask, self.spectral, self.degradation)
        try:
            if y is None:
                if degradation is not None:
                    raise AssertionError("unconditional sampling takes no degradation (:117)")
                self.y = None
            else:
                if y is not saved[0]:
                    self.y = y.contiguous().float()
                if callable(degradation) and degradation != saved[4] and degradation is not saved[3]:      # (bound methods compare by ==)
                    self.mask = self.smask = None
                    self.spectral, self.degradation = as_operator(degradation), degradation
            x_hat = self._denoise(x, t)
            keep, self.rid = self.rid, bool(self.rid and self.y is not None and self.xi > 0)
            try:
                _, d = self._score_step(x, x_hat, t, 0.0, mode=0)          # projection by the loop's rule (raises like the reference when undefined), d = -t * score
            finally:
                self.rid = keep
            score = torch.empty_like(x)
            _lib.call("aid_axpby", _lib.AxpbyParams(d.data_ptr(), d.data_ptr(), score.data_ptr(), None, None, B, L, -1.0 / float(t), 0.0))
            if self.rid and self.y is not None and self.xi > 0:
                return (score,) + tuple(self._rid_last) + (self._rid_pocs,)
            return score
        finally:
            self.y, self.mask, self.smask, self.spectral, self.degradation = saved

    def get_score_rec_guidance(self, x, y, t_i, degradation=None):
        """(:57-113) the guided evaluation on its own; needs xi > 0 like the branch that calls it in the reference (:129-131)."""
        if y is None or not self.xi > 0:
            raise _lib.AidError("get_score_rec_guidance needs observations and xi > 0")
        return self.get_score(x, y, t_i, degradation)

    def predict_spectrogram_inpainting(self, y_masked, mask):
        """y_masked[B,L], mask[F,T] (or [B,F,T]) over the STFT of tester.spectrogram_inpainting.stft -> [B,L]
        (:348-364): degradation = STFT-domain masking, projection y + x - A(x)."""
        self.setup_spectrogram_inpainting(y_masked, mask)
        return self.predict(self.y.shape, self.y.device)
