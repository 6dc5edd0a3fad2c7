/*
 * aid_autoregressive.h -- C ABI of the window carry of autoregressive generation in libaid_hip.so (gfx950).
 *
 * The reference's autoregressive sampler (testing/edm_sampler.py:386-418) produces a piece longer than one model
 * segment window by window: the first `end` samples of a new window are the last `end` samples of the previous one,
 * and the new part of every window is appended to the result (:414-416, three slicing / concatenation statements).
 * aid_ar_carry does both in ONE launch between two windows.
 *
 * Same boundary contract as aid_kernels.h: raw device pointers, sizes, offsets and row strides in ELEMENTS, a
 * hipStream_t passed as void*, 0 or a negative AID_E_* code, no allocation, no synchronisation.
 */
#ifndef AID_AUTOREGRESSIVE_H
#define AID_AUTOREGRESSIVE_H

#include <stdint.h>
#include "aid_kernels.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AID_AR_ABI_VERSION 1
int aid_ar_abi_version(void);

/* ---------------------------------------------------------------------------------------------------
 * aid_ar_carry -- x [B, L] contiguous fp32 is the window that was just sampled.
 *   y[b, i]                 = i < end ? x[b, L - end + i] : 0     i < L    (the next window's observations; y contiguous [B, L])
 *   out[b, off + i - skip]  = x[b, i]                             skip <= i < L,  skip = first ? 0 : end
 *   (out has row stride out_ld; `off` is the column of out where the new part of this window starts)
 *   y may be null (last window: append only).  1 <= end < L, off >= 0 and off + L - skip <= out_ld are required, so
 *   nothing outside row b of out is written.  x must not overlap y or out.
 *   Copies and zeroes only (bit-exact); float4 stores wherever the DESTINATION is 16-byte aligned, scalar head and
 *   tail otherwise -- end, L - end and off are in general not multiples of 4.
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    const float* x; float* y; float* out;
    int B, first;
    int64_t L, end, off, out_ld;
} aid_ar_carry_params;
int aid_ar_carry(const aid_ar_carry_params* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AID_AUTOREGRESSIVE_H */
