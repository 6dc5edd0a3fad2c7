"""Host tests of what the whole-recording modes share (restore.py): the max_batch refusal of Sampler.predict_*_long, mode by mode (the
refusals of the seven pooled modes side by side: test_long_tasks_host.py), and
``rows(lo, hi)`` of the base class of the window operators.  No GPU."""
import pytest
import torch


# ---- max_batch: an int (not bool) >= 1 everywhere, refused before anything is launched ----------------------------------------------------
def _inpainting(L):
    from test_restore_long_host import _stub_sampler
    return _stub_sampler()[0].predict_inpainting_long, (torch.zeros(2, 3 * L), torch.ones(1, 3 * L))


def _declipping(L):
    from test_declip_long_host import _stub_sampler
    return _stub_sampler()[0].predict_declipping_long, (torch.zeros(2, 3 * L), 0.5)


def _bwe(L):
    from test_bwe_long_host import _stub_sampler
    return _stub_sampler()[0].predict_bwe_long, (torch.zeros(2, 3 * L), torch.ones(33) / 33, "firwin")


def _bwe_lowrate(L):
    from test_bwe_lowrate_long_host import _stub_sampler
    return _stub_sampler()[0].predict_bwe_lowrate_long, (torch.zeros(2, 3 * L // 2), 2, "resample")


def _pr(L):
    from test_pr_long_host import _stub_sampler
    return _stub_sampler()[0].predict_pr_long, (torch.zeros(2, 256 // 2 + 1, 1 + (3 * L) // 64),)                   # (win_size 256, hop_size 64)


def _spectrogram_inpainting(L):
    from test_spec_long_host import _stub_sampler
    from audio_inpainting_diffusion_amd.spec_long import rec_frames
    return _stub_sampler()[0].predict_spectrogram_inpainting_long, (torch.zeros(2, 3 * L), torch.ones(256 // 2 + 1, rec_frames(3 * L, 256, 64)))


@pytest.mark.parametrize("mode", [_inpainting, _declipping, _bwe, _bwe_lowrate, _pr, _spectrogram_inpainting])
def test_every_long_method_refuses_a_max_batch_that_is_no_int_of_at_least_one_before_any_launch(mode, monkeypatch):
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.config import small_args
    launched = []
    monkeypatch.setattr(_lib, "call", lambda name, p: launched.append(name))
    call, args = mode(int(small_args(xi=0.25).exp.audio_len))
    with pytest.raises(_lib.AidError, match="GPU only"):                        # (the arguments are valid but for the device, which is judged last)
        call(*args, max_batch=3)
    for bad in (0, -2, 2.5, True, "8"):
        with pytest.raises(_lib.AidError, match="max_batch"):
            call(*args, max_batch=bad)
    assert launched == []


# ---- rows(lo, hi) of the operators' base class --------------------------------------------------------------------------------------------
class _FakeGPUState(torch.Tensor):
    """a host tensor that says it is on the GPU: the state refusal is the only thing in ``rows`` that asks for a device"""
    is_cuda = True


def _operator(rows, n=5):
    from audio_inpainting_diffusion_amd.restore import WindowOperator

    class Trivial(WindowOperator):
        def __init__(self, state):
            super().__init__(state, "[1|B, n]")

        def _slice(self, lo, hi):
            return Trivial(self._state_rows(lo, hi))

    return Trivial(torch.arange(rows * n, dtype=torch.float32).reshape(rows, n).as_subclass(_FakeGPUState))


def test_rows_of_the_window_operator_base_checks_its_range_keeps_one_object_per_range_and_a_shared_row_shared():
    from audio_inpainting_diffusion_amd import _lib, degrade
    from audio_inpainting_diffusion_amd.restore import WindowOperator
    assert issubclass(WindowOperator, degrade._Operator)
    op = _operator(4)
    assert op.shared_mask is False and op.items_held == 4
    sub = op.rows(1, 3)
    assert type(sub) is type(op) and sub.state.shape == (2, 5) and sub.state.data_ptr() == op.state[1:3].data_ptr()         # a view, no copy
    assert op.rows(1, 3) is sub and op.rows(1, 3.0) is sub and op.rows(0, 4) is not sub and op.rows(0, 4).state.shape == (4, 5)
    for lo, hi in ((1, 1), (3, 2), (-1, 2), (0, 5), (4, 5)):
        with pytest.raises(_lib.AidError, match=r"Trivial\.rows"):
            op.rows(lo, hi)
    shared = _operator(1)
    assert shared.items_held is None
    for lo, hi in ((0, 1), (2, 7), (0, 1000)):
        s = shared.rows(lo, hi)
        assert s.state.shape == (1, 5) and s.state.data_ptr() == shared.state.data_ptr() and shared.rows(lo, hi) is s
    for lo, hi in ((1, 1), (-1, 2)):
        with pytest.raises(_lib.AidError, match=r"Trivial\.rows"):
            shared.rows(lo, hi)
    # the state refusal, with the class name in front
    for bad in (torch.zeros(2, 5), torch.zeros(2, 5, dtype=torch.float64).as_subclass(_FakeGPUState), torch.zeros(5).as_subclass(_FakeGPUState),
                torch.zeros(2, 10).as_subclass(_FakeGPUState)[:, ::2], None):
        with pytest.raises(_lib.AidError, match="Trivial: state must be a float32 GPU tensor"):
            type(op)(bad)
