/*
 * aid_restore.h -- C ABI of the window gather / scatter of whole-recording restoration in libaid_hip.so (gfx950).
 *
 * A recording longer than one model segment is restored in two batched passes over windows of L samples laid out on the
 * autoregressive grid (restore.py: restore_plan): a pass gathers the observations and masks of all its windows into one
 * batch [J, L] (aid_window_gather), the sampler inpaints the batch, and the samples every window OWNS go back into the
 * result (aid_window_scatter).  Both kernels read a device table of J jobs, 6 int64 each:
 *
 *     r, s, head, tail, lo, hi      recording (row), first sample of the window, leading / trailing samples taken as observed
 *                                   from the result restored so far, owned range [lo, hi) relative to s
 *
 * Samples q = s + i >= N do not exist: they are gathered as observation 0 with mask 0 and never scattered.  A job whose r is
 * outside [0, R) or whose s is negative is skipped; head, tail, lo and hi are clamped to [0, L] -- the table lives in device
 * memory, so the kernels, not the launcher, keep every access inside the rows it was given.
 *
 * Same boundary contract as aid_kernels.h: raw device pointers, sizes, offsets and row strides in ELEMENTS, a
 * hipStream_t passed as void*, 0 or a negative AID_E_* code, no allocation, no synchronisation.
 */
#ifndef AID_RESTORE_H
#define AID_RESTORE_H

#include <stdint.h>
#include "aid_kernels.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AID_RESTORE_ABI_VERSION 1
#define AID_RESTORE_JOB_FIELDS 6
int aid_restore_abi_version(void);

/* ---------------------------------------------------------------------------------------------------
 * aid_window_gather -- for job j and i < L, q = s_j + i:
 *   edge      = i < head_j  or  i >= L - tail_j
 *   m[j, i]   = edge ? 1 : (q < N ? mask[r_j, q] : 0)
 *   y[j, i]   = m[j, i] * (q < N ? (edge ? out[r_j, q] : rec[r_j, q]) : 0)
 *   rec, out: [R, N] with row strides rec_ld, out_ld >= N; mask: [R, N] with row stride mask_ld >= N, or one shared row
 *   (mask_ld = 0); y, m: contiguous [J, L].  y and m must not overlap rec, out or mask.
 *   One pass; float4 stores over the 16-byte-aligned body of a row of y / m, float4 loads where the source is aligned at
 *   the same element, scalars otherwise and at the edges of the head / tail / N regions.
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    const float* rec; const float* out; const float* mask;
    float* y; float* m;
    const int64_t* jobs;
    int J, R;
    int64_t L, N, rec_ld, out_ld, mask_ld;
} aid_window_gather_params;
int aid_window_gather(const aid_window_gather_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * aid_gap_states -- dropouts of a filtered recording (bwe_declip_long.py), on the parameter block of aid_window_gather, IN
 *   PLACE over the rows aid_bwe_gather (aid_bwe_long.h) produced: y its observations, m its states.  For job j, i < L and
 *   q = s_j + i < N:
 *   m[j, i] == 0  and  mask[r_j, q] == 0      m[j, i] = -1,  y[j, i] = 0      (a dropped filtered sample is unobserved)
 *   Everything else is untouched: the other states, samples at or past N, and the rows of a job whose r is outside [0, R) or
 *   whose s is outside [0, N) (skipped).  mask: [R, N] with row stride mask_ld >= N, or one shared row (mask_ld = 0); y, m:
 *   contiguous [J, L], not overlapping mask.  rec, out, rec_ld and out_ld are unused; rec and out may be null.  Comparisons
 *   and constants only (bit-exact); no atomics.
 * ------------------------------------------------------------------------------------------------- */
int aid_gap_states(const aid_window_gather_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * aid_window_scatter -- out[r_j, s_j + i] = x[j, i]   for lo_j <= i < hi_j and s_j + i < N
 *   x: contiguous [J, L]; out: [R, N] with row stride out_ld >= N.  The owned ranges of the jobs of one call must not
 *   overlap (restore_plan: they partition the recording), so no atomics.  Copies only (bit-exact).
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    const float* x; float* out;
    const int64_t* jobs;
    int J, R;
    int64_t L, N, out_ld;
} aid_window_scatter_params;
int aid_window_scatter(const aid_window_scatter_params* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AID_RESTORE_H */
