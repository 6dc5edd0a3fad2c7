"""GPU tests of the job rows a gather must survive (csrc/aid_rows.h: rs_load_window), for the three gathers whose window starts lie on a
period: aid_lowrate_gather, aid_pr_gather, aid_spec_gather.  The table is device memory the launcher cannot inspect: a row with a recording
outside [0, R), a start below 0, at or past N or off the period gathers zeros, all absent; head / tail beyond L are clamped to L; lo / hi are
not the gather's business.  The outputs lie inside guarded buffers: nothing before or after the rows is written, and every entry of a row is.
(The pattern of test_gpu_bwe_long.py::test_an_invalid_job_row_of_the_bwe_gather_touches_nothing_outside_its_own_output.)"""
import pytest
import torch

from test_gpu_bwe_long import SENT

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64


def _rows(R, N, L, period):
    """(invalid rows, valid rows as (row in the table, the row it stands for after clamping)); every valid start is a multiple of 4"""
    past = N + (-N % period)
    invalid = [(R, 0, 0, 0, 0, L), (-1, 0, 0, 0, 0, L), (0, -2 * period, 0, 0, 0, L), (0, past, 0, 0, 0, L), (1 << 40, 1 << 40, 5, 5, 0, L),
               (0, period + 1, 0, 0, 0, L), (1, N - 1 - (N - 1) % period + 1, 0, 0, 0, L)]
    assert all(not (0 <= r < R and 0 <= s < N and s % period == 0) for r, s, *_ in invalid) and invalid[-1][1] < N and invalid[-2][1] % period
    mid = 2 * N // 3
    valid = [((1, 0, 10 * L, 0, 0, L), (1, 0, L, 0, 0, L)),                      # head clamped to L: the whole window known from out
             ((0, 8, 3, 10 * L, 0, L), (0, 8, 3, L, 0, L)),                      # tail clamped to L
             ((1, mid, 0, 0, -5, 10 * L), (1, mid, 0, 0, 0, L)),                 # the recording ends inside the window; lo / hi are ignored
             ((0, 8, -7, -7, 0, L), (0, 8, 0, 0, 0, L))]                         # negative head / tail clamped to 0
    assert mid % 4 == 0 and mid + L > N
    return invalid, valid


def _guarded(J, *row_lengths):
    return [torch.full((PAD + J * n + PAD,), SENT, device=DEV) for n in row_lengths]


def _check_guards(bufs):
    assert all(bool((b[:PAD] == SENT).all()) and bool((b[-PAD:] == SENT).all()) and not bool((b[PAD:-PAD] == SENT).any()) for b in bufs)


def _signals(R, N, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(R, N, generator=gen), torch.randn(R, N, generator=gen)


def test_an_invalid_job_row_of_the_lowrate_gather_touches_nothing_outside_its_own_output():
    from test_gpu_bwe_lowrate_long import _gather_ref
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.lowrate_long import low_len, rate_of, window_len
    from audio_inpainting_diffusion_amd.restore import job_table
    R, N, L = 2, 300, 128
    rate = rate_of(2, "resample")
    M, Mw = low_len(N, rate), window_len(L, rate)
    invalid, valid = _rows(R, N, L, rate.orig)
    rec, out = torch.randn(R, M, generator=torch.Generator().manual_seed(1)), _signals(R, N, 2)[1]
    rec_d, out_d = rec.to(DEV), out.to(DEV)
    jobs = invalid + [v[0] for v in valid]
    J, row = len(jobs), L + Mw
    bufs = _guarded(J, row, row)
    _lib.call("aid_lowrate_gather", _lib.LowrateGatherParams(rec_d.data_ptr(), out_d.data_ptr(), bufs[0][PAD:].data_ptr(), bufs[1][PAD:].data_ptr(),
                                                             job_table(jobs, DEV).data_ptr(), L, Mw, N, M, M, N, J, R, rate.orig, rate.new, rate.width, rate.K))
    _check_guards(bufs)
    y, k = (b[PAD:-PAD].reshape(J, row).cpu() for b in bufs)
    for j in range(len(invalid)):
        assert bool((y[j] == 0).all()) and bool((k[j] == -2).all()), j
    for j, (_, job) in enumerate(valid, len(invalid)):
        y_ref, k_ref = _gather_ref(rec, out, N, L, rate, job)
        assert torch.equal(k[j], k_ref) and torch.equal(y[j], y_ref), j
    j = len(invalid)
    assert bool((k[j, :L] == 1).all()) and torch.equal(y[j, :L], out[1, :L])                          # (head = L: all known)
    assert bool((k[j + 2, N - valid[2][1][1]:L] == -2).all()) and bool((k[j + 2, :L] != 1).all())      # (absent past N; no head, no tail)


def test_an_invalid_job_row_of_the_pr_gather_touches_nothing_outside_its_own_output():
    from test_gpu_pr_long import _gather_ref
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.phase_long import frames_of
    from audio_inpainting_diffusion_amd.restore import job_table
    R, N, L, n_fft, hop = 2, 150, 64, 16, 4
    F, T_rec, Tw = n_fft // 2 + 1, frames_of(N, hop), frames_of(L, hop)
    invalid, valid = _rows(R, N, L, hop)
    rec = torch.randn(R, F, T_rec, generator=torch.Generator().manual_seed(3)).abs()
    out = _signals(R, N, 4)[1]
    rec_d, out_d = rec.to(DEV), out.to(DEV)
    jobs = invalid + [v[0] for v in valid]
    J, row = len(jobs), L + F * Tw
    bufs = _guarded(J, row, L + Tw)
    _lib.call("aid_pr_gather", _lib.PrGatherParams(rec_d.data_ptr(), out_d.data_ptr(), bufs[0][PAD:].data_ptr(), bufs[1][PAD:].data_ptr(),
                                                   job_table(jobs, DEV).data_ptr(), L, N, T_rec, F * T_rec, T_rec, N, J, R, n_fft, hop, Tw))
    _check_guards(bufs)
    y, k = bufs[0][PAD:-PAD].reshape(J, row).cpu(), bufs[1][PAD:-PAD].reshape(J, L + Tw).cpu()
    for j in range(len(invalid)):
        assert bool((y[j] == 0).all()) and bool((k[j] == -2).all()), j
    for j, (_, job) in enumerate(valid, len(invalid)):
        y_ref, k_ref = _gather_ref(rec, out, N, L, n_fft, hop, job)
        assert torch.equal(k[j], k_ref) and torch.equal(y[j], y_ref), j
    j = len(invalid)
    assert bool((k[j, :L] == 1).all()) and torch.equal(y[j, :L], out[1, :L])                          # (head = L: all known)
    assert bool((k[j + 2, N - valid[2][1][1]:L] == -2).all()) and bool((k[j + 2, L:] == -2).any())     # (absent samples and frames past the end)


def test_an_invalid_job_row_of_the_spec_gather_touches_nothing_outside_its_own_output():
    from test_gpu_spec_long import _gather_ref
    from audio_inpainting_diffusion_amd import _lib
    from audio_inpainting_diffusion_amd.restore import job_table
    from audio_inpainting_diffusion_amd.spec_long import padded_length, window_frames
    R, N, L, n_fft, hop = 2, 150, 96, 16, 4
    Tw, Np = window_frames(L, n_fft, hop), padded_length(N, n_fft)
    invalid, valid = _rows(R, N, L, hop)
    rec, out = _signals(R, N, 5)
    rec_d, out_d = rec.to(DEV), out.to(DEV)
    jobs = invalid + [v[0] for v in valid]
    J = len(jobs)
    bufs = _guarded(J, L, L + Tw)
    itb = torch.full((8 + J * 3 + 8,), -77, dtype=torch.int64, device=DEV)
    _lib.call("aid_spec_gather", _lib.SpecGatherParams(rec_d.data_ptr(), out_d.data_ptr(), bufs[0][PAD:].data_ptr(), bufs[1][PAD:].data_ptr(), itb[8:].data_ptr(),
                                                       job_table(jobs, DEV).data_ptr(), L, N, Np, N, N, J, R, n_fft, hop, Tw))
    _check_guards(bufs)
    assert bool((itb[:8] == -77).all()) and bool((itb[-8:] == -77).all()) and not bool((itb[8:-8] == -77).any())
    y, k, it = bufs[0][PAD:-PAD].reshape(J, L).cpu(), bufs[1][PAD:-PAD].reshape(J, L + Tw).cpu(), itb[8:-8].reshape(J, 3).cpu()
    for j in range(len(invalid)):
        assert bool((y[j] == 0).all()) and bool((k[j] == -2).all()) and it[j].tolist() == [-1, -1, 0], j
    for j, (_, job) in enumerate(valid, len(invalid)):
        y_ref, k_ref, it_ref = _gather_ref(rec, out, N, L, n_fft, hop, job)
        assert torch.equal(k[j], k_ref) and torch.equal(y[j], y_ref) and torch.equal(it[j], it_ref), j
    j = len(invalid)
    assert bool((k[j, :L] == 1).all()) and torch.equal(y[j], out[1, :L])                              # (head = L: all known)
    assert bool((k[j + 2, N - valid[2][1][1]:L] == -2).all()) and bool((k[j + 3, :L] == 0).any())      # (absent past N; observed samples in a plain window)
