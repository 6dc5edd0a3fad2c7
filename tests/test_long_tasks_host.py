"""Host tests of the task records of the whole-recording modes (restore.LONG_TASKS) and of their one driver (Sampler._long over
restore.run_task): the registry names what Sampler has, a plain predict_*_long call and predict_long_pooled over the same one group
refuse in the same words before any launch, a group is checked once and built from what was checked, and the TypeError for wrong
task arguments comes from the record.  ``_lib.call`` is stubbed to record launches, as in test_long_shared_host.py.  No GPU."""
import inspect

import pytest
import scipy.signal
import torch

TASKS = ("inpainting", "declipping", "bwe", "bwe_iir", "bwe_declip", "bwe_lowrate", "pr")
WIN, HOP = 256, 64                                                           # (win_size, hop_size of the stub sampler's phase retrieval)


def _sampler(**kw):
    from test_pr_long_host import _stub_sampler
    return _stub_sampler(win=WIN, hop=HOP, **kw)


def _case(task, L, R=2):
    """(the group's entries after y for R recordings of 3L samples on the host, the arguments all groups share) -- valid but for the device"""
    y = torch.zeros(R, 3 * L)
    taps = torch.ones(33) / 33
    return {"inpainting": ((y, torch.ones(1, 3 * L)), {}),
            "declipping": ((y, 0.5), {}),
            "bwe": ((y,), dict(filt=taps, filt_type="firwin")),
            "bwe_iir": ((y,), dict(filt=scipy.signal.cheby1(4, 0.05, 1000, fs=22050), filt_type="cheby1")),
            "bwe_declip": ((y, 0.5, torch.ones(3 * L)), dict(filt=taps, filt_type="firwin")),
            "bwe_lowrate": ((torch.zeros(R, 3 * L // 2), None), dict(factor=2, filt_type="resample")),
            "pr": ((torch.zeros(R, WIN // 2 + 1, 1 + (3 * L) // HOP), None), {})}[task]


def _plain(smp, task, group, shared, **kw):
    """the plain method, called as its signature has it: y, the shared arguments, the entries"""
    from audio_inpainting_diffusion_amd import restore
    return getattr(smp, restore.LONG_TASKS[task].method)(group[0], *shared.values(), *group[1:], **kw)


def _refusal(call):
    from audio_inpainting_diffusion_amd import _lib
    with pytest.raises(_lib.AidError) as e:
        call()
    return type(e.value), str(e.value)


def test_the_registry_names_the_pooled_tasks_their_methods_and_their_entries():
    from audio_inpainting_diffusion_amd import restore
    from audio_inpainting_diffusion_amd.sampler import Sampler
    assert set(restore.LONG_TASKS) == set(Sampler.POOLED_TASKS) == set(TASKS)
    for name, task in restore.LONG_TASKS.items():
        assert task.name == name and task.what in ("restored", "declipped")
        params = list(inspect.signature(getattr(Sampler, task.method)).parameters)
        assert params[:2] == ["self", "y"] and params[-2:] == ["max_batch", "seeds"]
        # after y: the arguments all groups share, then the group's entries -- exactly the method's parameters
        assert tuple(params[2:-2]) == tuple(task.call_args) + task.entries, name
    assert [restore.LONG_TASKS[t].entries for t in TASKS] == [("mask",), ("clip_value",), (), (), ("clip_value", "mask"), ("length",), ("length",)]
    assert [t for t in TASKS if restore.LONG_TASKS[t].guided] == ["pr"]
    assert [t for t in TASKS if restore.LONG_TASKS[t].consistency] == ["bwe_declip", "bwe_lowrate", "pr"]


@pytest.mark.parametrize("task", TASKS)
def test_the_plain_method_and_the_pooled_entry_refuse_in_the_same_words_before_any_launch(task, monkeypatch):
    from audio_inpainting_diffusion_amd import _lib, restore
    launched = []
    monkeypatch.setattr(_lib, "call", lambda name, p: launched.append(name))
    record = restore.LONG_TASKS[task]
    smp, L = _sampler()
    group, shared = _case(task, L)

    def both(smp, want, **kw):
        plain = _refusal(lambda: _plain(smp, task, group, shared, **kw))
        pooled = _refusal(lambda: smp.predict_long_pooled(task, [group], **shared, **kw))
        assert plain == pooled and plain[0] is _lib.AidError and want in plain[1], (plain, pooled)
        return plain[1]

    assert record.method in both(_sampler(rid=True)[0], "rid must be False")
    if record.consistency:
        for dc in ("always", "end"):
            assert record.consistency in both(_sampler(dc=dc)[0], "without data consistency")
    if record.guided:
        assert record.guided in both(_sampler(xi=0)[0], "xi must be > 0")
    for bad in (0, True, 2.5):
        both(smp, "max_batch", max_batch=bad)
    for bad in ([1], [1, 2, 3]):
        both(smp, f"{len(bad)} seeds for 2 recordings", seeds=bad)
    both(smp, "GPU only")                                                    # valid but for the device, which is judged last
    both(smp, "GPU only", max_batch=3, seeds=[4, 5])
    assert launched == []


def _counting(fn, counts, key):
    def counted(*a, **k):
        counts[key] = counts.get(key, 0) + 1
        return fn(*a, **k)
    return counted


@pytest.mark.parametrize("task", TASKS)
def test_a_group_is_checked_once_and_the_coefficient_table_is_made_once_per_call(task, monkeypatch):
    from audio_inpainting_diffusion_amd import _lib, bwe_iir_long, restore
    launched, counts = [], {}
    monkeypatch.setattr(_lib, "call", lambda name, p: launched.append(name))
    record = restore.LONG_TASKS[task]
    monkeypatch.setitem(restore.LONG_TASKS, task, record._replace(check=_counting(record.check, counts, "check")))
    monkeypatch.setattr(bwe_iir_long.IIRTable, "__init__", _counting(bwe_iir_long.IIRTable.__init__, counts, "table"))
    smp, L = _sampler()
    group, shared = _case(task, L)
    with pytest.raises(_lib.AidError, match="GPU only"):
        _plain(smp, task, group, shared)
    assert counts.get("check") == 1 and counts.get("table", 0) == (1 if task == "bwe_iir" else 0)
    counts.clear()
    with pytest.raises(_lib.AidError, match="GPU only"):
        smp.predict_long_pooled(task, [group, _case(task, L, R=1)[0]], seeds=[1, 2, 3], **shared)
    # (the first group is refused for its device: the second is not reached, and nothing was checked twice)
    assert counts.get("check") == 1 and counts.get("table", 0) == (1 if task == "bwe_iir" else 0)
    # both groups are reached when the device is not asked for: the last refusal of check_batch is stubbed away
    counts.clear()
    monkeypatch.setattr(restore, "check_batch", lambda *a, **k: None)
    monkeypatch.setattr(smp, "_check_model", lambda: (_ for _ in ()).throw(_lib.AidError("checked, not built")))
    with pytest.raises(_lib.AidError, match="checked, not built"):
        smp.predict_long_pooled(task, [group, _case(task, L, R=1)[0]], seeds=[1, 2, 3], **shared)
    assert counts.get("check") == 2 and counts.get("table", 0) == (1 if task == "bwe_iir" else 0)
    assert launched == []


def test_wrong_task_arguments_are_a_type_error_in_the_words_of_the_record():
    from audio_inpainting_diffusion_amd import _lib
    smp, L = _sampler()
    y = torch.zeros(1, 2 * L)
    for task in ("bwe", "bwe_iir", "bwe_declip"):
        for bad in (dict(), dict(filt=1), dict(filt_type="firwin"), dict(filt=1, filt_type="firwin", factor=2), dict(factor=2)):
            with pytest.raises(TypeError) as e:
                smp.predict_long_pooled(task, [y], **bad)
            assert str(e.value) == f"predict_long_pooled({task!r}) takes the task arguments (filt, filt_type), got ({', '.join(bad)})"
    for bad in (dict(), dict(filt_type="resample"), dict(factor=2, filt=1), dict(factor=2, filt_type="resample", length=5)):
        with pytest.raises(TypeError) as e:
            smp.predict_long_pooled("bwe_lowrate", [y], **bad)
        assert str(e.value) == f"predict_long_pooled('bwe_lowrate') takes the task arguments (factor, filt_type), got ({', '.join(bad)})"
    with pytest.raises(_lib.AidError, match="GPU only"):
        smp.predict_long_pooled("bwe_lowrate", [y], factor=2)                # filt_type defaults to "resample"
    for task in ("inpainting", "declipping", "pr"):
        with pytest.raises(TypeError) as e:
            smp.predict_long_pooled(task, [y], filt=1)
        assert str(e.value) == f"predict_long_pooled({task!r}) takes the task arguments (), got (filt)"
    with pytest.raises(NotImplementedError, match="unknown task 'denoising'"):
        smp.predict_long_pooled("denoising", [y])
    with pytest.raises(_lib.AidError, match="one recording-shaped mask"):
        smp.predict_long_pooled("spectrogram_inpainting", [y])
