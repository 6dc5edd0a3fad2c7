"""CPU tests (no GPU) of phase retrieval (include/aid_phase.h, audio_inpainting_diffusion_amd/phase.py, Sampler.predict_pr):
the config lookup and the refusals that happen before any kernel runs."""

import pytest
import torch



def test_hamming_window_and_observation_shape_match_torch():
    import numpy as np
    from audio_inpainting_diffusion_amd.phase import hamming_tables, observation_shape
    w, tw = hamming_tables(1024)
    assert np.abs(w - torch.hamming_window(1024, dtype=torch.float64).numpy()).max() < 1e-15
    assert tw.shape == (512, 2)
    x2 = torch.zeros(1, 4096 + 1024)                                 # the reference appends win_size zeros
    X = torch.stft(x2, 1024, hop_length=256, window=torch.hamming_window(1024), center=False, return_complex=True)
    assert tuple(X.shape[1:]) == observation_shape(1024, 256, 4096) == (513, 17)
    x2 = torch.zeros(1, 4000 + 512)
    X = torch.stft(x2, 512, hop_length=384, window=torch.hamming_window(512), center=False, return_complex=True)
    assert tuple(X.shape[1:]) == observation_shape(512, 384, 4000)


def _sampler(xi=0.25, inference=None, tester=(1024, 256)):
    from audio_inpainting_diffusion_amd.config import small_args
    from audio_inpainting_diffusion_amd.edm import EDM
    from audio_inpainting_diffusion_amd.sampler import Sampler
    args = small_args(xi=xi)
    if tester is None:
        del args.tester["phase_retrieval"]
    else:
        args.tester.phase_retrieval = dict(win_size=tester[0], hop_size=tester[1])
    if inference is not None:
        args.inference = dict(phase_retrieval=dict(win_size=inference[0], hop_size=inference[1]))

    class _Fused:                                                   # (stands for the MI355X network: never evaluated here)
        denoise = denoise_guided = None
    return Sampler(model=_Fused(), diff_params=EDM(args), args=args)


def test_predict_pr_refusals():
    from audio_inpainting_diffusion_amd import _lib
    y = torch.zeros(1, 513, 17)                                    # |STFT| of 4096 samples, N = 1024, hop = 256
    with pytest.raises(_lib.AidError, match="xi"):
        _sampler(xi=0.0).predict_pr(y)
    for bad in (torch.zeros(1, 513, 16), torch.zeros(1, 512, 17), torch.zeros(513, 17), torch.zeros(1, 513 * 17)):
        with pytest.raises(_lib.AidError, match="predict_pr: y must be"):
            _sampler().predict_pr(bad)
    with pytest.raises(_lib.AidError, match="power of two"):
        _sampler(tester=(1000, 250)).predict_pr(torch.zeros(1, 501, 17))
    with pytest.raises(_lib.AidError, match="hop_size"):
        _sampler(tester=(1024, 0)).predict_pr(y)
    with pytest.raises(_lib.AidError, match="no phase_retrieval config"):
        _sampler(tester=None).predict_pr(y)


def test_phase_retrieval_config_lookup_order():
    from audio_inpainting_diffusion_amd.config import make_args
    from audio_inpainting_diffusion_amd.sampler import phase_retrieval_sizes
    assert phase_retrieval_sizes(make_args()) == (1024, 256)                     # the shipped tester yaml's values
    assert phase_retrieval_sizes(_sampler(inference=(512, 128)).args) == (512, 128)      # args.inference wins (where the reference reads them)
    assert phase_retrieval_sizes(_sampler(inference=(512, 128), tester=None).args) == (512, 128)
    assert phase_retrieval_sizes(_sampler(tester=(2048, 512)).args) == (2048, 512)
    # the lookup decides the expected observation shape: a y sized for the tester's sizes is refused when args.inference overrides them
    from audio_inpainting_diffusion_amd import _lib
    with pytest.raises(_lib.AidError, match=r"\[B, 257, 33\]"):
        _sampler(inference=(512, 128)).predict_pr(torch.zeros(1, 513, 17))


def test_stft_magnitude_is_gpu_only_and_checks_sizes_first():
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.phase import STFTMagnitude
    with pytest.raises(_lib.AidError, match="power of two"):
        STFTMagnitude(1000, 250, 4096, device="cpu")
    with pytest.raises(_lib.AidError, match="GPU only"):
        STFTMagnitude(1024, 256, 4096, device="cpu")
