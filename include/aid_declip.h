/*
 * aid_declip.h -- C ABI of declipping whole recordings in libaid_hip.so (gfx950): the observation operator of a window whose
 * samples are clipped, known or absent, and the gather that builds its per-window inputs.
 *
 * A clipped recording longer than one model segment is restored on the window grid of aid_restore.h (restore.py: restore_plan
 * over the mask |y| < c): the even windows that hold a clipped sample as one batch, then the odd ones, whose first and last
 * samples are the already restored overlaps.  Every sample of a window carries a STATE, a float in {0, 1, -1}:
 *
 *      0   observed through the clipper:  y = clamp(x, -c, c)      (the recording)
 *      1   known:                         y = x                    (an overlap sample another window restored)
 *     -1   absent:                        no observation           (the sample lies beyond the end of the recording)
 *
 * Any state > 0 is read as 1 and any state < 0 as -1.  c is a level PER ROW, read from device memory: the recordings of one
 * batch may clip at different levels.
 *
 * Same boundary contract as aid_kernels.h: raw device pointers, sizes, offsets and row strides in ELEMENTS, a
 * hipStream_t passed as void*, 0 or a negative AID_E_* code, no allocation, no synchronisation.
 */
#ifndef AID_DECLIP_H
#define AID_DECLIP_H

#include <stdint.h>
#include "aid_kernels.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AID_DECLIP_ABI_VERSION 1
int aid_declip_abi_version(void);

/* ---------------------------------------------------------------------------------------------------
 * aid_clip_known -- signals [B, L] fp32; k = state[b, i], c = clip[b] (> 0)
 *   mode 0 (apply):       out = k > 0 ? x : (k < 0 ? 0 : clamp(x, -c, c))
 *   mode 1 (adjoint):     out = k > 0 ? x : (k < 0 ? 0 : (-c <= xref <= c ? x : 0))        x: incoming gradient, xref: the input
 *                         of the matching apply; inclusive bounds, as aid_clip
 *   mode 2 (projection):  out = k > 0 ? y : (k < 0 ? x : (y >= c ? max(x, c) : (y <= -c ? min(x, -c) : y)))
 *                         the point nearest to x of the (convex) set of signals consistent with the observation y
 *   x, out: row strides x_ld, out_ld >= L; xref (mode 1) and y (mode 2): row strides xref_ld, y_ld >= L, unused pointers may
 *   be null; state: [B, L] with row stride state_ld >= L, or one shared row (state_ld = 0); clip: [B].  out must not overlap
 *   an input.  One pass; float4 over the 16-byte-aligned body of a row of out (loads where the source is aligned at the same
 *   element), scalars at the ragged ends; selections, comparisons, min and max only: every mode is exact.
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    const float* x; const float* xref; const float* y; const float* state; const float* clip;
    float* out;
    int B, mode;
    int64_t L, x_ld, xref_ld, y_ld, state_ld, out_ld;
} aid_clip_known_params;
int aid_clip_known(const aid_clip_known_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * aid_declip_gather -- for job j of the table of aid_restore.h (r, s, head, tail, lo, hi; 6 int64) and i < L, q = s_j + i:
 *   edge      = i < head_j  or  i >= L - tail_j
 *   k[j, i]   = q >= N ? -1 : (edge ? 1 : 0)
 *   y[j, i]   = q >= N ?  0 : (edge ? out[r_j, q] : rec[r_j, q])
 *   c[j]      = clip[r_j]
 *   rec, out: [R, N] with row strides rec_ld, out_ld >= N; clip: [R]; y, k: contiguous [J, L]; c: [J].  y, k and c must not
 *   overlap rec, out or clip.  The table is device memory: a job whose r is outside [0, R) or whose s is outside [0, N) is
 *   skipped (y = 0, k = -1, c = 0 over its row); head and tail are clamped to [0, L].  One launch serves a whole pass;
 *   copies only (bit-exact).  The samples go back with aid_window_scatter.
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    const float* rec; const float* out; const float* clip;
    float* y; float* k; float* c;
    const int64_t* jobs;
    int J, R;
    int64_t L, N, rec_ld, out_ld;
} aid_declip_gather_params;
int aid_declip_gather(const aid_declip_gather_params* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AID_DECLIP_H */
