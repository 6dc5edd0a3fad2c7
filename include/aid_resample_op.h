/*
 * aid_resample_op.h -- C ABI of the resampling degradation of bandwidth extension in libaid_hip.so (gfx950): the exact adjoint
 * of aid_resample_poly (aid_kernels.h), which the reconstruction guidance needs once per denoiser evaluation.
 *
 * With K = 2*width + orig_freq and orig_freq / new_freq already divided by their gcd, the forward map is
 *
 *      y[b, i*new + j] = sum_{t < K} k[j][t] * x[b, i*orig + t - width]          (x zero outside [0, L), i*new + j < Lout)
 *
 * and its transpose, for q < L,
 *
 *      gx[b, q] = sum over frames i >= 0 with 0 <= t = q + width - i*orig < K,
 *                     over phases j < new with i*new + j < Lout,   of   k[j][t] * g[b, i*new + j]
 *
 * Same boundary contract as aid_kernels.h: raw device pointers, sizes and row strides in ELEMENTS, a hipStream_t passed as
 * void*, 0 or a negative AID_E_* code, no allocation, no synchronisation.
 */
#ifndef AID_RESAMPLE_OP_H
#define AID_RESAMPLE_OP_H

#include <stdint.h>
#include "aid_kernels.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AID_RESAMPLE_OP_ABI_VERSION 1
int aid_resample_op_abi_version(void);

/* ---------------------------------------------------------------------------------------------------
 * aid_resample_poly_adj -- g [B, Lout] fp32 (row stride g_ld >= Lout) -> gx [B, L] fp32 (row stride gx_ld >= L)
 *   kT:    [K, new_freq] fp32, kT[t][j] = k[j][t]: the table aid_resample_poly takes, transposed
 *   j_lo, j_hi: [K] int32 each.  The term of tap t and phase j is visited for j_lo[t] <= j < j_hi[t] only (both clamped to
 *          [0, new_freq] by the kernel); every kT[t][j] outside that range must be 0.0f, so that the skipped terms are
 *          0.0f * g and the result is that of the full sum.  The Hann window of the table is clamped to zero outside its
 *          support, which leaves most of a row of kT exactly 0.0f at ratios with many phases.
 *   Geometry as aid_resample_poly requires it: K == 2*width + orig_freq, 0 < Lout <= ceil(new_freq * L / orig_freq);
 *   1 <= B <= 65535.  gx must not overlap an input.  A gather with one owner per gx[b, q]: no atomics, a fixed summation
 *   order (frames ascending, phases ascending), 64-bit sample indices.
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    const float* g; float* gx; const float* kT;
    const int32_t* j_lo; const int32_t* j_hi;
    int64_t g_ld, gx_ld, L, Lout;
    int B, orig_freq, new_freq, width, K;
} aid_resample_poly_adj_params;
int aid_resample_poly_adj(const aid_resample_poly_adj_params* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AID_RESAMPLE_OP_H */
