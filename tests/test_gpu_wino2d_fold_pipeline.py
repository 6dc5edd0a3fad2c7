"""The folded 2-D Winograd GEMM (csrc/aid_wino2d.hip, w2d_gemm_fold_kernel) after its kernels were generalised over the MFMA fragment (32 x 32 x 2 or 16 x 16 x 4) and
the 96 x 64 tile of the 96-channel panels moved from three waves of 32 x 32 x 2 to four waves of 16 x 16 x 4 fragments.  Through the C ABI (aid_conv2d_wino2d_gemm /
aid_conv2d).

Every instance keeps each element's K order and the order of the fold (Y_j += AF^T[j][xf] * acc in ascending xf), and both fp32 MFMA shapes accumulate their
products as one fmaf chain in ascending k (MI355X: four products of 16x16x4 round like two steps of 32x32x2), so M' and y must be the SAME BITS as the library of
the commit before, on the 128-wide instances and on the re-cut 96 x 64 one: tests/golden/w2d_fold_parent_sha256.json holds the sha256 of both, recorded on an MI355X
from a build of that commit.  The plane stream is then run at every number of K chunks per plane the shape check admits (aid_conv2d_wino2d_supported wants Cin >= 64: two chunks of
32 are the fewest, a single chunk per plane cannot be reached through the C ABI), against fp64 references at the bars of tests/test_gpu_wino2d.py; and the new
96-channel instance on the aligned, ragged and two-M-tile shapes, forward and in reverse.
"""
import hashlib
import json
import os

import pytest
import torch

from conftest import rel_l2
from test_gpu_wino2d import DEV, _FoldedLayer, _check_folded_forward

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "w2d_fold_parent_sha256.json")

# B, Cin, Cout, F, T, dil, instance                                  K chunks per plane
W2D_FOLD_BIT_CASES = [
    (4, 128, 128, 80, 512, 1, "<128x64,foldM,kc32"),               # 4   aligned
    (3, 128, 128, 78, 672, 1, "<128x64,foldM,kc32"),               # 4   ragged column tile and row tile
    (3, 64, 128, 78, 672, 1, "<128x64,foldM,kc32"),                # 2   the prologue holds all of plane 0
    (3, 80, 128, 78, 672, 1, "<128x64,foldM,kc16"),                # 5
    (3, 96, 96, 100, 544, 2, "<96x64,foldM,kc24"),                 # 4   the 96 x 64 tile: recorded from the three-wave 32x32x2 instance, asserted on the four-wave 16x16x4 one
]


@pytest.fixture(scope="module")
def L():
    from audio_inpainting_diffusion_amd import _lib
    _lib.lib()
    return _lib


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def fold_hashes(L, case):
    """sha256 of M' (the 40 planes the folded GEMM writes, from aid_conv2d_wino2d_gemm) and of y (aid_conv2d: gate + residual epilogue) of a seeded layer"""
    s = _FoldedLayer(L, case)
    B, Ci, C, Fd, T, dil = s.dims
    y = torch.full((B, C, Fd, T), float("nan"), device=DEV)
    p = s.params(y, stats=False)
    L.call("aid_conv2d_wino2d_gemm", p)
    torch.cuda.synchronize()
    name = L.lib().aid_last_kernel().decode()
    assert s.inst in name, name
    out = {"Mf": _sha(s.ws[:40 * C * s.N])}
    s.ws.fill_(7.0)
    L.call("aid_conv2d", p)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all())
    out["y"] = _sha(y)
    return out


def case_key(case):
    return "x".join(str(v) for v in case[:6])


@pytest.mark.parametrize("case", W2D_FOLD_BIT_CASES)
def test_folded_gemm_bits_unchanged(L, case):
    """M' and y are the bits of the parent commit's library (recorded from a build of it): the generalisation over the fragment changed nothing for FR = 32, and the
    16x16x4 instance of the 96 x 64 tile sums every element's products in the same order with the same roundings"""
    want = json.load(open(GOLDEN))["sha256"][case_key(case)]
    got = fold_hashes(L, case)
    assert got == want, (case, got, want)


W2D_FOLD_CHUNK_CASES = [
    # B, Cin, Cout, F, T, dil, instance                              K chunks per plane (2 and 4 at kc32, 5 at kc16 are W2D_FOLD_BIT_CASES)
    (3, 96, 128, 78, 672, 1, "<128x64,foldM,kc32"),                # 3   odd: a plane starts in another buffer of the ring of three every time
    (3, 112, 128, 78, 672, 1, "<128x64,foldM,kc16"),               # 7
    (3, 64, 96, 78, 672, 1, "<128x64(96),foldM,kc32"),             # 2   clamped weight columns
    (3, 80, 96, 78, 672, 1, "<128x64(96),foldM,kc16"),             # 5   clamped weight columns
]          # (the 96 x 64 instance takes Cin % 48 == 0 only -- Cin % 16 of the shape check and chunks of 24 -- which between 64 and 128 is Cin = 96: four chunks)


def _check_folded_planes(L, case, tag=None):
    """M' on its own (aid_conv2d_wino2d_gemm) against the 80 fp64 products folded with AF^T in fp64: the unfolded fp32 GEMM of the same U, V folded plane by plane
    in fp32 measures E; the folded kernel does the same sums in registers and must stay within 2 E on the whole tensor, on the last column tile and on the last M
    tile (the bar and the measurement of test_conv2d_wino2d_folded_gemm_planes: ratio 1.00); the other 40 planes of ws untouched; the kernel asserted by name."""
    s = _FoldedLayer(L, case)
    B, Ci, C, Fd, T, dil = s.dims
    N = s.N
    y = torch.full((B, C, Fd, T), float("nan"), device=DEV)
    p = s.params(y, stats=False)
    L.call("aid_conv2d_wino2d_gemm", p)
    torch.cuda.synchronize()
    name = L.lib().aid_last_kernel().decode()
    assert s.inst in name and (tag is None or tag in name), name
    rest = s.ws[40 * C * N:]
    assert float(rest.min()) == 7.0 and float(rest.max()) == 7.0
    Mf = s.ws[:40 * C * N].reshape(4, 10, C, N).cpu()
    M = torch.full((80 * C * N + 16,), 7.0, device=DEV)
    L.call("aid_wino2d_gemm", L.Wino2dGemmParams(s.wpw.data_ptr(), s.V.data_ptr(), M.data_ptr(), 80, Ci, C, s.wp.shape[1], s.wp.shape[2], N, 0))
    torch.cuda.synchronize()
    assert float(M[80 * C * N:].min()) == 7.0
    Mu = M[:80 * C * N].reshape(8, 10, C, N)
    AFT = L.wino45_matrices()[0]                                          # [4, 8]
    fold32 = torch.stack([sum(float(AFT[j, xf]) * Mu[xf] for xf in range(8) if AFT[j, xf] != 0) for j in range(4)]).cpu()
    U, V = s.wpw.cpu()[:, :Ci, :C].double().reshape(8, 10, Ci, C), s.V.cpu().double().reshape(8, 10, Ci, N)
    AFTd = torch.from_numpy(AFT)
    ref = torch.stack([torch.einsum("jf,fcn->jcn", AFTd, torch.bmm(U[:, xt].transpose(1, 2), V[:, xt])) for xt in range(10)], dim=1)      # [4, 10, C, N]
    n_tail, m_tail = (N - 1) // 64 * 64, (C - 1) // 128 * 128 if "128x64" in s.inst else (C - 1) // 96 * 96
    for what, sl in (("whole", (Ellipsis,)), ("last column tile", (Ellipsis, slice(n_tail, N))), ("last M tile", (Ellipsis, slice(m_tail, C), slice(None)))):
        e_k, e_t = rel_l2(Mf[sl], ref[sl]), rel_l2(fold32[sl], ref[sl])
        print(f"folded GEMM planes {case} {what}: folded kernel {e_k:.2e}, fp32 fold of the 80-plane M {e_t:.2e} (ratio {e_k / e_t:.2f})")
        assert e_k <= 2 * e_t, (what, e_k, e_t)


@pytest.mark.parametrize("case", W2D_FOLD_CHUNK_CASES)
def test_folded_gemm_at_every_chunk_count(L, case):
    """The eight-plane chunk stream at 2, 3, 5 and 7 K chunks per plane on the four-wave instances, with and without clamped weight columns (ragged column tile, ragged row
    tiles; >= 768 workgroups so that the launch folds).  (1) M' on its own (_check_folded_planes).  (2) the whole forward launch against the fp64 convolution on the
    CPU: 2.5e-5 on the whole tensor, W2D_FOLD_SLICE_BAR per (b, f) row and (b, co) tail (_check_folded_forward)."""
    B, Ci, C, Fd, T, dil, inst = case
    N = int(L.lib().aid_conv2d_wino2d_positions(B, Fd, T, dil)) // 2
    assert N % 64 != 0 and (Fd // dil) % 4 != 0
    _check_folded_planes(L, case)
    _check_folded_forward(L, case)


# The 96-channel panels: the 96 x 64 tile on FOUR waves x (48 x 32), 3 x 2 fragments of v_mfma_f32_16x16x4_f32 each (six independent accumulator chains per wave,
# every SIMD of the CU holds the same number of waves, three workgroups per CU), K chunks of 24 = 15 one-KiB pieces on four waves (the last one loaded twice).
# Besides the recorded bits of one shape above, these cases are checked against fp64 references at the existing bars.  The instance takes Cin % 48 == 0 (Cin % 16 of
# the shape check and chunks of 24):
# between the shape check's Cin >= 64 and the fold's Cin <= 128 that is Cin = 96, four chunks per plane; Cin = 48 is not a shape the C ABI admits.
W2D_FOLD96_CASES = [
    (4, 96, 96, 96, 512, 2, "<96x64,foldM,kc24"),                  # aligned
    (3, 96, 96, 100, 544, 2, "<96x64,foldM,kc24"),                 # ragged both ways
    (2, 96, 192, 38, 992, 1, "<96x64,foldM,kc24"),                 # two M tiles
]


@pytest.mark.parametrize("case", W2D_FOLD96_CASES)
def test_balanced_96_instance(L, case):
    """M' planes against the fp64 product folded with AF^T (2 E bar, whole / last column tile / last M tile) and the forward launch against the fp64 convolution
    (2.5e-5 whole tensor, W2D_FOLD_SLICE_BAR per slice), on the four-wave 16x16x4 instance, asserted by name"""
    _check_folded_planes(L, case, tag="4w16x16x4")
    _check_folded_forward(L, case)


def test_balanced_96_instance_reverse_and_fin(L):
    """fin_mode = 1 forward and the reverse sweep with fin_mode = 2 on the aligned 96 -> 96 case (the checks of test_conv2d_wino2d_folded_reverse_and_fin, which
    runs them on the ragged one): both launches on the four-wave instance"""
    import test_gpu_wino2d as tw
    inst = "<96x64,foldM,kc24,nb3,4w16x16x4"
    tw.test_conv2d_wino2d_folded_reverse_and_fin(L, W2D_FOLD96_CASES[0][:6] + (inst,), inst)
