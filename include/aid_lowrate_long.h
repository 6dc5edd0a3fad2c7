/*
 * aid_lowrate_long.h -- C ABI of bandwidth extension of whole low-sample-rate recordings in libaid_hip.so (gfx950): the observation
 * operator of a window seen through the rational-ratio resampler of aid_resample_poly (aid_kernels.h), and the gather that builds
 * its per-window inputs.
 *
 * A recording that exists only at a low sample rate (M samples) is restored at the high rate (N samples) on the window grid of
 * aid_restore.h, with every window start a multiple of the input period orig_freq (lowrate_long.py): a window cut from the
 * high-rate signal and resampled then yields the recording's own low-rate samples wherever the window holds the sample's whole
 * kernel support.  With K = 2*width + orig_freq and Mw = ceil(new_freq * L / orig_freq), a window's observation row has L + Mw
 * entries: the first L on the high-rate side (entry i is sample s + i), the last Mw on the low-rate side (entry n is low-rate
 * sample (s / orig_freq) * new_freq + n of the recording).  Every entry carries a STATE, one float:
 *
 *   high-rate entry i       1   known:       y = x[i]          (an overlap sample another window restored)
 *                          -1   no direct observation          (the sample exists; it is seen through the resampler only)
 *                          -2   absent                         (beyond the end of the recording: it enters the resampler as 0)
 *   low-rate entry n        0   observed:    y = sum_{t<K} k[j][t] xin[i*orig_freq + t - width],  n = i*new_freq + j
 *                          -1   unobserved                     (the kernel support leaves the window although the recording goes on)
 *                          -2   absent                         (beyond the last low-rate sample of the recording)
 *
 * Any state > 0 is read as 1, any state <= -2 as -2; a low-rate entry is observed only when its state == 0.
 *
 * Same boundary contract as aid_kernels.h: raw device pointers, sizes, offsets and row strides in ELEMENTS, a
 * hipStream_t passed as void*, 0 or a negative AID_E_* code, no allocation, no synchronisation.
 */
#ifndef AID_LOWRATE_LONG_H
#define AID_LOWRATE_LONG_H

#include <stdint.h>
#include "aid_kernels.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AID_LOWRATE_LONG_ABI_VERSION 1
int aid_lowrate_long_abi_version(void);

/* ---------------------------------------------------------------------------------------------------
 * aid_rate_observed -- state [B, L + Mw] (row stride state_ld >= L + Mw, or one shared row: state_ld = 0), kh = state[b, i],
 *   kl = state[b, L + n]; samples outside [0, L) are 0.
 *   mode 0 (apply):    x [B, L] (x_ld >= L) -> out [B, L + Mw] (out_ld >= L + Mw)
 *                      xin = kh <= -2 ? 0 : x
 *                      out[i]     = kh > 0 ? x[i] : 0
 *                      out[L + n] = kl == 0 ? sum_{t<K} k[j][t] xin[i*orig_freq + t - width] : 0          (n = i*new_freq + j)
 *   mode 1 (adjoint):  x [B, L + Mw] (x_ld >= L + Mw), the incoming gradient -> out [B, L] (out_ld >= L)
 *                      gin[n] = kl == 0 ? x[L + n] : 0;   a = the sum of aid_resample_poly_adj over gin (Lout = Mw)
 *                      out[q] = kh <= -2 ? 0 : (kh > 0 ? a[q] + x[q] : a[q])
 *   k: [new_freq, K] fp32, the table aid_resample_poly takes; kT, j_lo, j_hi: as aid_resample_poly_adj takes them
 *   (aid_resample_op.h).  Mode 0 reads k only, mode 1 kT, j_lo and j_hi only.  The sums are those of aid_resample_poly and
 *   aid_resample_poly_adj, with the same terms in the same order: with no known or absent sample and every low-rate state 0, the
 *   low side of mode 0 and mode 1 on [0 | g] give those kernels' bits.  Selections are exact: a known output of mode 0 is x itself.
 *   Geometry: K == 2*width + orig_freq, Mw == ceil(new_freq * L / orig_freq), 1 <= B <= 65535.  out must not overlap an input.
 *   One thread per output element, no atomics, a fixed summation order.
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    const float* x; const float* state; const float* k; const float* kT;
    const int32_t* j_lo; const int32_t* j_hi;
    float* out;
    int64_t L, Mw, x_ld, state_ld, out_ld;
    int B, mode, orig_freq, new_freq, width, K;
} aid_rate_observed_params;
int aid_rate_observed(const aid_rate_observed_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * aid_lowrate_gather -- for job j of the table of aid_restore.h (r, s, head, tail, lo, hi; 6 int64); the first match decides.
 *   High-rate entry i < L, q = s_j + i:
 *     q >= N                                                   state[j, i] = -2,  y[j, i] = 0
 *     i < head_j  or  i >= L - tail_j                          state[j, i] =  1,  y[j, i] = out[r_j, q]
 *     otherwise                                                state[j, i] = -1,  y[j, i] = 0
 *   Low-rate entry n < Mw, mrec = (s_j / orig_freq) * new_freq + n, a0 = (n / new_freq) * orig_freq - width:
 *     mrec >= M                                                state[j, L + n] = -2,  y[j, L + n] = 0
 *     (s_j > 0 and a0 < 0)  or  (s_j + L < N and a0 + K > L)   state[j, L + n] = -1,  y[j, L + n] = 0
 *     otherwise                                                state[j, L + n] =  0,  y[j, L + n] = rec[r_j, mrec]
 *   rec: the low-rate recordings [R, M], row stride rec_ld >= M; out: the high-rate result so far [R, N], row stride
 *   out_ld >= N; y, state: contiguous [J, L + Mw].  y and state must not overlap rec or out.  The table is device memory: a job
 *   whose r is outside [0, R), whose s is outside [0, N) or no multiple of orig_freq is skipped (y = 0, state = -2 over its
 *   row); head and tail are clamped to [0, L].  One launch serves a whole pass; copies only (bit-exact).  The samples go back
 *   with aid_window_scatter.
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    const float* rec; const float* out;
    float* y; float* state;
    const int64_t* jobs;
    int64_t L, Mw, N, M, rec_ld, out_ld;
    int J, R, orig_freq, new_freq, width, K;
} aid_lowrate_gather_params;
int aid_lowrate_gather(const aid_lowrate_gather_params* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AID_LOWRATE_LONG_H */
