/*
 * aid_degrade.h -- C ABI of the restoration degradations of libaid_hip.so (gfx950): FIR / IIR filtering, decimation
 * and hard clipping, each with its exact adjoint.  They are the linear (or piecewise linear) operators A of the
 * reference's bandwidth-extension and declipping samplers (testing/edm_sampler.py:245-300, :359-385), evaluated in
 * every guided denoiser evaluation as A(x_hat) and A^T(g).
 *
 * Same boundary contract as aid_kernels.h: raw device pointers, sizes and row strides in ELEMENTS, a hipStream_t
 * passed as void*, 0 or a negative AID_E_* code, no allocation, no synchronisation.  All signals are fp32 [B, len]
 * row-major.  Every entry point ends in the epilogue  out = c0 * A(x) + add1 + add2  (add1 / add2 optional, read with
 * the output's row stride), so the data-consistency projection y + x - A(x) costs no extra pass.
 */
#ifndef AID_DEGRADE_H
#define AID_DEGRADE_H

#include <stdint.h>
#include "aid_kernels.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AID_DEGRADE_ABI_VERSION 1
int aid_degrade_abi_version(void);

/* ---------------------------------------------------------------------------------------------------
 * aid_fir -- strided FIR correlation and its adjoint.
 *   adjoint = 0:  out[b, i] = sum_{k<K} h[k] * x[b, i*stride + k - pad_left],  i < L_out, x zero outside [0, L)
 *                 x is [B, L] (row stride x_ld), out is [B, L_out] (row stride out_ld)
 *   adjoint = 1:  A^T by gather (no atomics): x is [B, L_out], out is [B, L]
 *   covers torch conv1d(x[:,None], h[1,1,K], padding="same") (pad_left = (K-1)//2, the reference's apply_FIR_filter,
 *   edm_sampler.py:245-251), decimation x[..., 0:-1:f] (h = [1], stride = f, L_out = ceil((L-1)/f), :259-260) and
 *   strided low-passes.  stride 1: any K; stride 2..16: K <= 4096.
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    const float* x; float* out; const float* h;
    const float* add1; const float* add2; float c0;
    int B, K, stride, pad_left, adjoint;
    int64_t L, L_out;
    int64_t x_ld, out_ld;
} aid_fir_params;
int aid_fir(const aid_fir_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * aid_iir -- direct-form IIR filter (scipy.signal.lfilter(b, a, x) / torchaudio.functional.lfilter(x, a, b, clamp))
 *   and its adjoint, zero initial state, output length L, recursion in fp64.
 *   coef [2*(N+1)] fp64: b[0..N] then a[0..N], normalised so that a[0] = 1 (N = order <= 16);
 *   H [C, N] fp64: H[m][j] = y[m] of the input-free recursion started from y[-1-i] = (i == j)  (C >= N).
 *   Three launches, block-parallel over chunks of C samples:
 *     1. zero-state recursion of every chunk -> z [B, L] fp64, chunk end states -> state [B, n_chunks, N] fp64;
 *     2. carry scan over the chunks of a row: s_{c+1}[j] = zend_c[j] + sum_i H[C-1-j][i] s_c[i]  (state := s_c);
 *     3. out = z + H[n % C] . s_{n / C}, then [clamp], then the epilogue.
 *   adjoint = 1 runs the same recursion over reversed indices (A^T = J A J, J = reversal); no copy.
 *   clamp = 1: forward output clamped to [-1, 1] (torchaudio's clamp, applied after the recursion); pre [B, L] (optional
 *   in the forward) receives the unclamped output; the adjoint needs it and multiplies g by (-1 <= pre <= 1).
 *   z, state and pre are contiguous.
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    const float* x; float* out; float* pre;
    const double* coef; const double* H;
    double* z; double* state;
    const float* add1; const float* add2; float c0;
    int B, N, C, clamp, adjoint;
    int64_t L, x_ld, out_ld;
} aid_iir_params;
int aid_iir(const aid_iir_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * aid_clip -- hard clipping (the reference's apply_clip, edm_sampler.py:366-368).
 *   adjoint = 0:  out = clip(x, -clip, clip)
 *   adjoint = 1:  out = x * (-clip <= xref <= clip)   (x = incoming gradient, xref = the input of the matching forward;
 *                 inclusive bounds, as torch.clamp's backward)
 *   x / out are [B, L] with row strides x_ld / out_ld; xref is contiguous [B, L].
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    const float* x; const float* xref; float* out;
    const float* add1; const float* add2; float c0; float clip;
    int B, adjoint;
    int64_t L, x_ld, out_ld;
} aid_clip_params;
int aid_clip(const aid_clip_params* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AID_DEGRADE_H */
