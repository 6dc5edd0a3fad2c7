"""CPU tests (no GPU) of autoregressive generation and compressed sensing (include/aid_autoregressive.h, Sampler.predict_autoregressive /
predict_compsens, masks.compsens_mask, harness.generate_long): the config lookup, the refusals (all raised
before anything touches a GPU), the mask builder, the length formula -- and ``oracle_autoregressive``, the reference's composition
(testing/edm_sampler.py:396-418: predict_unconditional, then predict_inpainting on the carried tail, hard concatenation) restated with
oracle.sampler.OracleSampler.  tests/test_gpu_autoregressive.py compares the HIP path against that helper; here it is pinned."""

import pytest
import torch

from conftest import rel_l2


# ---- the reference composition on the CPU oracle ------------------------------------------------------------------------------------
class ToyCPU(torch.nn.Module):
    """Same toy denoiser as tests/golden/make_golden.py::_ToyNet (a test fixture), in float32 or float64."""

    def __init__(self, L, dtype=torch.float32):
        super().__init__()
        from oracle.nsgt_cqt import OracleCQT
        self.CQTransform = OracleCQT(3, 8, "oct", ("kaiser", 1), 22050, L, dtype=dtype)
        self.k = torch.tensor([0.02, -0.05, 0.1, 0.25, 0.4, 0.25, 0.1, -0.05, 0.02], dtype=dtype).view(1, 1, 9)

    def forward(self, x, cnoise):
        y = torch.nn.functional.conv1d(x.unsqueeze(1), self.k, padding=4).squeeze(1)
        return y * torch.tanh(cnoise) + 0.1 * torch.sin(3.0 * x)


def oracle_autoregressive(osmp, shape, N, end, seeds=None, dtype=torch.float32, carried=None):
    """The reference's predict_autoregressive (edm_sampler.py:396-418) on an OracleSampler -> (piece [B, L + (N-1)(L-end)], windows, rng_states).
    RNG: seeds None -> the global CPU generator, consumed in the reference's order (prior, churn draws, next prior, ...); seeds [...] -> one
    generator per item for the WHOLE piece.  Every draw is a float32 draw cast to ``dtype``, so a float64 run sees the noise of the float32 run.
    ``rng_states[w]``: global generator state before window w (teacher-forced tests restore it).  ``carried``: windows of ANOTHER run whose
    tails condition this run's windows instead of its own (teacher forcing); None: free-running."""
    B, L = shape
    gens = None if seeds is None else [torch.Generator().manual_seed(int(s)) for s in seeds]

    def randn(shp, _gens):
        if gens is None:
            return torch.randn(shp, dtype=torch.float32).to(dtype)
        return torch.cat([torch.randn([1, shp[1]], generator=g, dtype=torch.float32) for g in gens], dim=0).to(dtype)
    osmp._randn = randn
    keep = torch.get_default_dtype()
    torch.set_default_dtype(dtype)                           # (the oracle builds its schedule and windows in the default dtype)
    try:
        mask = torch.ones((1, L), dtype=dtype)
        mask[:, end:] = 0
        states = [torch.get_rng_state()]
        x = osmp.predict_unconditional((B, L))
        windows, out = [x], x
        for w in range(1, N):
            prev = x if carried is None else carried[w - 1].to(dtype)
            y = torch.zeros((B, L), dtype=dtype)
            y[:, 0:end] = prev[:, L - end:]                  # (:414)
            states.append(torch.get_rng_state())
            x = osmp.predict_inpainting(y, mask)             # (:415)
            windows.append(x)
            out = torch.cat((out, x[..., end:]), -1)         # (:416)
    finally:
        torch.set_default_dtype(keep)
        del osmp._randn
    return out, windows, states


def toy_oracle(L, T, xi=0.25, dtype=torch.float32, **kw):
    from oracle.edm import OracleEDM
    from oracle.sampler import OracleSampler
    return OracleSampler(ToyCPU(L, dtype), OracleEDM(), T=T, xi=xi, hann_size=20, audio_len=L, **kw)


def test_oracle_composition_joins_are_exact_copies():
    from audio_inpainting_diffusion_amd.sampler import autoregressive_length
    L, N, end = 2048, 3, 512
    torch.manual_seed(5)
    out, wins, states = oracle_autoregressive(toy_oracle(L, 4), (1, L), N, end)
    step = L - end
    assert out.shape == (1, autoregressive_length(L, end, N)) == (1, L + 2 * step) and len(wins) == N and len(states) == N
    assert torch.isfinite(out).all()
    assert torch.equal(out[:, :L], wins[0])
    for w in (1, 2):
        off = L + (w - 1) * step
        assert torch.equal(out[:, off:off + step], wins[w][:, end:])
        assert torch.equal(out[:, off - end:off], wins[w - 1][:, L - end:])          # what window w was conditioned on
    # the same composition replayed window by window from the recorded generator states gives the same windows (teacher forcing with its own windows)
    torch.manual_seed(5)
    out2, wins2, _ = oracle_autoregressive(toy_oracle(L, 4), (1, L), N, end, carried=wins)
    assert torch.equal(out, out2)
    # the float64 composition sees the same noise: it differs from the float32 one by rounding only
    torch.manual_seed(5)
    out32, _, _ = oracle_autoregressive(toy_oracle(L, 6), (1, L), N, end)
    torch.manual_seed(5)
    out64, _, _ = oracle_autoregressive(toy_oracle(L, 6, dtype=torch.float64), (1, L), N, end, dtype=torch.float64)
    assert out64.dtype == torch.float64 and 0 < rel_l2(out32, out64) < 1e-4
    assert torch.get_default_dtype() == torch.float32
    # seeds: one generator per item for the whole piece -> item b of a batch is the B = 1 run with its seed
    both, _, _ = oracle_autoregressive(toy_oracle(L, 6), (2, L), 2, end, seeds=[11, 12])
    one, _, _ = oracle_autoregressive(toy_oracle(L, 6), (1, L), 2, end, seeds=[12])
    one64, _, _ = oracle_autoregressive(toy_oracle(L, 6, dtype=torch.float64), (1, L), 2, end, seeds=[12], dtype=torch.float64)
    # (same draws; the CPU conv / FFT routines take other code paths for B = 2, so the float32 rounding differs: held to the composition's own
    #  sensitivity to rounding, float32 against float64, with the factor the GPU tests use)
    assert rel_l2(both[1:2], one) <= 4 * rel_l2(one, one64) and rel_l2(both[0:1], one) > 0.1


# ---- config, refusals, mask, lengths ---------------------------------------------------------------------------------------------------
def test_overlap_lookup_order():
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.config import TESTER_LONG, small_args
    from audio_inpainting_diffusion_amd.sampler import autoregressive_overlap
    assert TESTER_LONG["autoregressive"] == dict(overlap=0.25, num_samples=4) and TESTER_LONG["comp_sens"] == dict(percentage=5)
    args = small_args()
    assert autoregressive_overlap(args) == 0.25                              # tester node (where the shipped yaml puts it)
    args.inference = dict(autoregressive=dict(overlap=0.5))
    assert autoregressive_overlap(args) == 0.5                               # inference node wins (where the reference reads it)
    args.inference = dict(other=1)
    assert autoregressive_overlap(args) == 0.25
    del args.tester["autoregressive"]
    with pytest.raises(_lib.AidError, match="autoregressive"):
        autoregressive_overlap(args)


class _Fused:                                                                # (stands for the MI355X network: never evaluated here)
    denoise = denoise_guided = None


def _stub_sampler(rid=False, **tester):
    from audio_inpainting_diffusion_amd.config import small_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.sampler import Sampler
    args = small_args(xi=0.25)
    for k, v in tester.items():
        node = args.tester
        *path, leaf = k.split(".")
        for q in path:
            node = getattr(node, q)
        setattr(node, leaf, v)
    return Sampler(model=_Fused(), diff_params=EDM(args), args=args, rid=rid), int(args.exp.audio_len)


def test_predict_autoregressive_refusals_come_before_the_gpu():
    from audio_inpainting_diffusion_amd import _lib
    smp, L = _stub_sampler()
    with pytest.raises(_lib.AidError, match="audio_len"):
        smp.predict_autoregressive((1, L - 4), 2, "cuda")
    with pytest.raises(_lib.AidError, match="N must be >= 1"):
        smp.predict_autoregressive((1, L), 0, "cuda")
    for ov in (0.0, 1e-6, 1.0, 1.5):
        smp, L = _stub_sampler(**{"autoregressive.overlap": ov})
        with pytest.raises(_lib.AidError, match="overlap"):
            smp.predict_autoregressive((1, L), 2, "cuda")
    smp, L = _stub_sampler(rid=True)
    with pytest.raises(_lib.AidError, match="rid"):
        smp.predict_autoregressive((1, L), 2, "cuda")
    smp, L = _stub_sampler()
    with pytest.raises(_lib.AidError, match="GPU only"):
        smp.predict_autoregressive((1, L), 2, "cpu")
    assert smp.y is None and smp.mask is None and smp.n_evals == 0 and smp._keep_gens is False


def test_predict_compsens_refusals_come_before_the_gpu():
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.masks import compsens_mask
    for over, what in (({"posterior_sampling.xi": 0.0, "data_consistency.use": False}, "xi"),
                       ({"data_consistency.use": True, "data_consistency.type": "always"}, "data consistency"),
                       ({"data_consistency.use": True, "data_consistency.type": "end"}, "data consistency")):
        smp, L = _stub_sampler(**over)
        m = compsens_mask(L, 5)
        with pytest.raises(_lib.AidError, match=what):
            smp.predict_compsens(torch.zeros(1, L) * m, m)
        assert smp.y is None and smp.mask is None                            # nothing was installed


def test_compsens_mask():
    from audio_inpainting_diffusion_amd.masks import compsens_mask
    for L, pct in ((4096, 5), (184184, 5), (1000, 12.5), (777, 33)):
        m = compsens_mask(L, pct, generator=torch.Generator().manual_seed(1))
        assert m.shape == (1, L) and m.dtype == torch.float32
        assert int(m.sum()) == int(round(pct / 100 * L)) and set(m.unique().tolist()) <= {0.0, 1.0}
        assert torch.equal(m, compsens_mask(L, pct, generator=torch.Generator().manual_seed(1)))
        assert not torch.equal(m, compsens_mask(L, pct, generator=torch.Generator().manual_seed(2)))
    assert int(compsens_mask(512, 0).sum()) == 0 and int(compsens_mask(512, 100).sum()) == 512
    with pytest.raises(ValueError):
        compsens_mask(512, 101)


@pytest.mark.parametrize("L,overlap,N,total", [(184184, 0.25, 4, 184184 + 3 * 138138), (184184, 0.25, 1, 184184), (4096, 0.25, 3, 4096 + 2 * 3072),
                                               (4099, 0.25, 2, 4099 + 3075), (1000, 0.999, 5, 1000 + 4 * 1)])
def test_output_length_formula(L, overlap, N, total):
    from audio_inpainting_diffusion_amd.sampler import autoregressive_length
    end = int(overlap * L)
    if L == 184184:
        assert end == 46046
    assert autoregressive_length(L, end, N) == total


def test_generate_long_checks_its_arguments():
    from audio_inpainting_diffusion_amd.harness import generate_long
    smp, _ = _stub_sampler()
    with pytest.raises(ValueError):
        generate_long(smp, 0, 2)
    with pytest.raises(ValueError):
        generate_long(smp, 3, 2, seeds=[1, 2])
