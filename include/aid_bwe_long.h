/*
 * aid_bwe_long.h -- C ABI of bandwidth extension of whole recordings in libaid_hip.so (gfx950): the observation operator of a
 * window seen through a stride-1 FIR filter, whose samples are filtered, known, unobserved or absent, and the gather that
 * builds its per-window inputs.
 *
 * A low-passed recording longer than one model segment is restored on the window grid of aid_restore.h (bwe_long.py): every
 * even window as one batch, then the odd ones, whose first and last samples are the already restored overlaps.  The recording
 * was filtered as a whole ("same" padding: zeros before its first and after its last sample), so inside a window only the
 * samples that hold the whole filter support behind them are observations of the window.  Every sample of a window carries a
 * STATE, one float:
 *
 *      0   filtered:    y = sum_k h[k] xin[i + k - P]     (the low-passed recording; P = (K-1)/2)
 *      1   known:       y = x                             (an overlap sample another window restored)
 *     -1   unobserved:  no observation                    (the sample exists and feeds its neighbours' observations; its own
 *                                                          filtered value depends on samples outside the window)
 *     -2   absent:      no observation                    (the sample lies beyond the end of the recording: it enters the
 *                                                          filter as 0, the recording's own padding)
 *
 * Any state > 0 is read as 1, any state <= -2 as -2 and any other state < 0 as -1.
 *
 * Same boundary contract as aid_kernels.h: raw device pointers, sizes, offsets and row strides in ELEMENTS, a
 * hipStream_t passed as void*, 0 or a negative AID_E_* code, no allocation, no synchronisation.
 */
#ifndef AID_BWE_LONG_H
#define AID_BWE_LONG_H

#include <stdint.h>
#include "aid_kernels.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AID_BWE_LONG_ABI_VERSION 1
int aid_bwe_long_abi_version(void);

/* ---------------------------------------------------------------------------------------------------
 * aid_fir_observed -- signals [B, L] fp32, taps h[K], k = state[b, i], P = (K-1)/2; samples outside [0, L) are 0.
 *   mode 0 (apply):       xin = k <= -2 ? 0 : x;  c[i] = sum_{j<K} h[j] xin[i + j - P]
 *                         out = k > 0 ? x : (k == 0 ? c : 0)
 *   mode 1 (adjoint):     gin = k == 0 ? x : 0;   a[i] = sum_{j<K} h[j] gin[i - j + P]         x: incoming gradient
 *                         out = k <= -2 ? 0 : (k > 0 ? a + x : a)
 *   mode 2 (projection):  c as in mode 0;  out = k > 0 ? y : (k == 0 ? (y - c) + x : x)
 *   x, out: row strides x_ld, out_ld >= L; y (mode 2): row stride y_ld >= L, may be null otherwise; state: [B, L] with row
 *   stride state_ld >= L, or one shared row (state_ld = 0).  out must not overlap an input.  The sums are those of aid_fir at
 *   stride 1 (aid_degrade.h), in the same order: with every state 0, modes 0 and 1 give aid_fir's bits ("same" padding and its
 *   adjoint), and mode 2 those of aid_fir's epilogue -c + y + x.  Selections are exact: a known output of mode 0 is x itself.
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    const float* x; const float* y; const float* state; const float* h;
    float* out;
    int B, K, mode;
    int64_t L, x_ld, y_ld, state_ld, out_ld;
} aid_fir_observed_params;
int aid_fir_observed(const aid_fir_observed_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * aid_bwe_gather -- for job j of the table of aid_restore.h (r, s, head, tail, lo, hi; 6 int64) and i < L, q = s_j + i,
 *   P = (K-1)/2, Q = K-1-P; the first match decides:
 *   q >= N                                                   state[j, i] = -2,  y[j, i] = 0
 *   i < head_j  or  i >= L - tail_j                          state[j, i] =  1,  y[j, i] = out[r_j, q]
 *   (s_j > 0 and i < P)  or  (s_j + L < N and i >= L - Q)    state[j, i] = -1,  y[j, i] = 0
 *   otherwise                                                state[j, i] =  0,  y[j, i] = rec[r_j, q]
 *   rec, out: [R, N] with row strides rec_ld, out_ld >= N; y, state: contiguous [J, L].  y and state must not overlap rec or
 *   out.  The table is device memory: a job whose r is outside [0, R) or whose s is outside [0, N) is skipped (y = 0,
 *   state = -2 over its row); head and tail are clamped to [0, L].  One launch serves a whole pass; copies only (bit-exact).
 *   The samples go back with aid_window_scatter.
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    const float* rec; const float* out;
    float* y; float* state;
    const int64_t* jobs;
    int J, R, K;
    int64_t L, N, rec_ld, out_ld;
} aid_bwe_gather_params;
int aid_bwe_gather(const aid_bwe_gather_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * aid_iir_observed -- the same window seen through an IIR filter (bwe_iir_long.py), on the parameter block of aid_fir_observed:
 *   K = order + 1 in [2, 17]; h is a float table [2 K], b[0..K) then a[0..K), normalised (a[0] = 1; exact in fp32); L <= 2^20.
 *   A fifth state, -3 (SEED): the leading run of -3 states of a row, S samples long, holds samples of the filtered recording
 *   that start the recursion instead of being observed.  A -3 after that run counts as -1.  Any other state <= -2 is absent.
 *   With k = state[b, i], xin = absent ? 0 : x, u[i] = sum_{j<K, i-j>=0} b[j] xin[i-j], and the recursion in fp64
 *       yh[i] = 0 (i < S);   yh[i] = u[i] - sum_{1<=j<K, i-j>=S} a[j] yh[i-j]  (i >= S):
 *   mode 0 (apply):       out = k > 0 ? x : (k == 0 ? yh : 0)
 *   mode 1 (adjoint):     g0 = k == 0 ? x : 0;  w[i] = 0 (i < S),  w[i] = g0[i] - sum_{1<=j<K, i+j<L} a[j] w[i+j]  (i >= S, backwards);
 *                         c[i] = sum_{j<K, i+j<L} b[j] w[i+j];   out = absent ? 0 : (k > 0 ? c + x : c)
 *   mode 2 (projection):  out = k > 0 ? y : (k == 0 ? (y - yh) + x : x)
 *   mode 3 (preparation): x is a raw row of aid_iir_gather;  r[i] = x[i] (i < S),  r[i] = -sum_{1<=j<K, i-j>=0} a[j] r[i-j]  (i >= S);
 *                         out = k > 0 ? x : (k == 0 ? x - r (fp64, rounded once) : 0)
 *   Strides, the shared state row (state_ld = 0) and the no-overlap rule are those of aid_fir_observed.  One workgroup per
 *   row; registers and static LDS only: no scratch, nothing kept between calls.  Deterministic.
 * aid_iir_gather -- on the parameter block of aid_bwe_gather, K = order + 1 in [2, 17]; for job j and i < L, q = s_j + i; the
 *   first match decides:
 *   q >= N                                                   state[j, i] = -2,  y[j, i] = 0
 *   s_j > 0 and i < K - 1                                    state[j, i] = -3,  y[j, i] = rec[r_j, q]
 *   i < head_j  or  i >= L - tail_j                          state[j, i] =  1,  y[j, i] = out[r_j, q]
 *   otherwise                                                state[j, i] =  0,  y[j, i] = rec[r_j, q]
 *   Everything else as aid_bwe_gather (invalid jobs, clamping, copies only).  The rows are raw: one mode-3 launch of
 *   aid_iir_observed turns them into the observations.
 * ------------------------------------------------------------------------------------------------- */
int aid_iir_observed(const aid_fir_observed_params* p, void* stream);
int aid_iir_gather(const aid_bwe_gather_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * aid_fir_clip_observed -- the same window seen through the FIR filter FOLLOWED BY a hard clipper, one level per item
 *   (bwe_declip_long.py), on the parameter block of aid_fir_observed: h is a float table [K + B], the K taps, then the level
 *   c_b of every item (> 0; +inf: the item is not clipped).  States, P, "samples outside [0, L) are 0" and the sums as
 *   aid_fir_observed; k = state[b, i].
 *   mode 0 (apply):       xin = k <= -2 ? 0 : x;  c[i] = sum_{j<K} h[j] xin[i + j - P]
 *                         out[b, i]     = k > 0 ? x : (k == 0 ? fminf(fmaxf(c, -c_b), c_b) : 0)      plane 0: the observation
 *                         out[B + b, i] = k == 0 ? c : 0                                             plane 1: the pre-clip sum
 *                         out holds TWO planes of B rows, [2 B] rows with row stride out_ld: the plane stride is B * out_ld.
 *   mode 1 (adjoint):     x: incoming gradient; y: plane 1 of the matching mode-0 launch, row stride y_ld >= L
 *                         gin = (k == 0 and -c_b <= y <= c_b) ? x : 0      (inclusive bounds, as aid_clip and aid_clip_known)
 *                         a[i] = sum_{j<K} h[j] gin[i - j + P];   out = k <= -2 ? 0 : (k > 0 ? a + x : a)        one plane
 *   Any other mode is refused (the clipped filter has no projection), and so is a null y in mode 1; y may be null in mode 0.
 *   Strides, the shared state row (state_ld = 0) and the no-overlap rule are those of aid_fir_observed.  The sums are
 *   aid_fir_observed's, in the same order: plane 0 carries the bits of aid_clip_known (mode 0, states 0 / 1 / < 0) applied to
 *   mode 0 of aid_fir_observed, plane 1 those of aid_fir_observed where k == 0, and mode 1 those of aid_fir_observed's mode 1
 *   applied to aid_clip_known's mode 1 -- in one launch each instead of two.  With every level +inf, modes 0 (plane 0) and 1
 *   give aid_fir_observed's bits.  Selections are exact.  No LDS beyond the tile's, no atomics, nothing kept between calls.
 * ------------------------------------------------------------------------------------------------- */
int aid_fir_clip_observed(const aid_fir_observed_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * aid_fir_observed_items -- aid_fir_observed with one filter per item (blind.py: the taps fitted for every item), on the parameter
 *   block of aid_fir_observed: h is a float table [B, K] with row stride K, item b is filtered with h[b, 0..K).  Everything else --
 *   states, modes 0 / 1 / 2, strides, the shared state row (state_ld = 0), the no-overlap rule, the sums and their order -- is
 *   aid_fir_observed's: with equal rows of h it gives aid_fir_observed's bits, and with every state 0 as well those of aid_fir.
 * ------------------------------------------------------------------------------------------------- */
int aid_fir_observed_items(const aid_fir_observed_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * aid_window_energy -- the energy of the windows of a job table (blind_long.py: the windows a recording's filter is fitted on), on
 *   the parameter block of aid_bwe_gather: for job j of the table of aid_restore.h (r, s, ...; 6 int64),
 *       energy[j] = sum over i < L with s_j + i < N of rec[r_j, s_j + i]^2        in fp64.
 *   rec: [R, N] fp32 with row stride rec_ld >= N; jobs: [J, 6] in device memory; y = energy: J DOUBLES behind the float pointer
 *   (contiguous, 8-byte aligned).  out and state are not read, K and out_ld are ignored.  As in aid_bwe_gather a job whose r is outside
 *   [0, R) or whose s is outside [0, N) is skipped: its energy is 0.  One workgroup per job: every lane adds the squares of the samples
 *   i = lane, lane + 256, ... ascending, and the 256 partial sums are added as a fixed binary tree.  No atomics: a second launch gives
 *   the same bits.
 * ------------------------------------------------------------------------------------------------- */
int aid_window_energy(const aid_bwe_gather_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * aid_eval_sums -- the weighted time-domain sums and the frame mean behind the restoration metrics (metrics.py), on the parameter
 *   block of aid_fir_observed.  What every field means here:
 *   x      the estimate  e [B, L], row stride x_ld >= L                                                                   (read)
 *   y      the reference r [B, L], row stride y_ld >= L                                                                   (read)
 *   state  the region weights [B, L], row stride state_ld >= L, or one shared row (state_ld = 0); 0 or non-zero, not fractional;
 *          null: every sample counts                                                                                      (read)
 *   h      the frame distances [B, K] with row stride K, an output of aid_stft_logspec_dist (K = its n_frames): a value < 0 marks
 *          a frame that is not counted                                                                                    (read)
 *   out    sums [B, 8]: 8 DOUBLES per item behind the float pointer (contiguous, 8-byte aligned); out_ld is ignored        (written)
 *   mode   must be 0
 *   sums[b] = n (the samples with a non-zero weight), sum r^2, sum e^2, sum r e, sum (r - e)^2 and max |r - e| over those samples,
 *   the number of counted frames, the sum of their distances -- all in fp64.  One workgroup of 512 lanes per item: lane l takes the
 *   samples (then the frames) l, l + 512, ... ascending, and the 512 partial results are combined as a fixed binary tree.  No
 *   atomics: a second launch gives the same bits; item b does not depend on the other items.
 * ------------------------------------------------------------------------------------------------- */
int aid_eval_sums(const aid_fir_observed_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * aid_ar_score -- the outlier score of declicking (declick.py; csrc/aid_declick.hip): every block of a recording is fitted with an
 *   autoregressive model and every sample scored by its prediction residual over a robust scale.  On the parameter block of
 *   aid_bwe_gather.  What every field means here:
 *   rec     the recordings [R, N] fp32, row stride rec_ld >= N                                                              (read)
 *   out     the scalars: 2 floats in HOST memory, ridge >= 0 and sigma_floor > 0, both finite.  The launcher reads them before it
 *           returns and hands them to the kernel with its arguments; the memory may be reused as soon as the call returns.    (read)
 *   y       the scores [R, N] fp32, row stride out_ld >= N                                                                  (written)
 *   state   sigma [R, J] fp32, contiguous: the scale of every block, 0 where the block was not scored                       (written)
 *   jobs    not read (may be null)
 *   L       the block length: 256, 512, 1024, 2048 or 4096;  K  the model order, 1 <= K <= 32 and 8 K <= L
 *   J       the blocks of a recording: J == ceil(N / L);  R <= 65535
 *   Block j of a row holds the n samples x[0 .. n) at the positions [j L, min(N, (j + 1) L)).  With n < 8 K it is not scored: its
 *   scores and its sigma are 0.  Otherwise, in fp64:  r[m] = sum_{i = m}^{n - 1} x[i] x[i - m] for m = 0 .. K, r[0] *= 1 + ridge; with
 *   r[0] <= 0 the block is not scored either.  Levinson-Durbin on r gives a[1 .. K] with a[0] = 1 (it stops, leaving the remaining
 *   coefficients 0, once the error power is <= 0).  e[q] = sum_{k = 0}^{K} a[k] rec[q - k] over the RECORDING's samples (those of the
 *   previous block where q - k falls there, 0 before the first sample).  The scored samples are the block's, but never the first K
 *   of the recording, whose score is 0.  median = the element of rank n' / 2 (0-based, integer division) of |e| over the n' scored
 *   samples, sorted ascending; sigma = max(median / 0.6745, sigma_floor); score = |e| / sigma, rounded to fp32 once.
 *   One workgroup of 256 lanes per (recording, block): the block and K samples of history in LDS; lane l adds the products
 *   i = l, l + 256, ... ascending (from the first i >= m) and the 256 partial sums are added as a fixed binary tree; one lane runs the
 *   recursion; the median comes from a bitonic sort of |e|, padded with +inf, in LDS.  Static LDS only, no scratch, no atomics,
 *   nothing kept between calls: a second launch gives the same bits, and a row does not depend on the other rows.  Non-finite
 *   samples are outside the contract.
 *
 * aid_click_mask -- from the scores to the mask of predict_inpainting_long (1 = observed, 0 = restore).  On the parameter block of
 *   aid_fir_observed.  What every field means here:
 *   x       the recordings [B, L] fp32, row stride x_ld >= L                                                                (read)
 *   y       the scores [B, L] fp32 (aid_ar_score's), row stride y_ld >= L                                                   (read)
 *   state   not read (may be null)
 *   h       the settings: 4 floats in HOST memory -- threshold > 0, then the whole numbers pad in [0, 256], min_run (0 = no run rule,
 *           otherwise 2 <= min_run <= max_run) and max_run in [1, 1024] -- read by the launcher as aid_ar_score reads its scalars (read)
 *   out     the mask [B, L] fp32, row stride out_ld >= L                                                                    (written)
 *   K       ignored;  mode  must be 0;  B <= 65535
 *   A sample is FLAGGED when its score is > threshold (fp32 against fp32), or, with min_run > 0, when it lies in a maximal run of
 *   bit-identical samples of length l, min_run <= l <= max_run, that holds neither the first nor the last sample of the recording.
 *   mask[q] = 0 when a sample of [q - pad, q + pad] within [0, L) is flagged, 1 otherwise.
 *   One workgroup of 256 lanes per tile of 1024 samples; the tile with pad + max_run samples on either side (clamped to the
 *   recording) in LDS.  Run starts, run ends and the count of flags behind the +-pad window are scans in LDS.  A run that reaches
 *   the edge of what was loaded without ending is longer than max_run or holds an end of the recording: it is never flagged.
 *   Compares and integers only: exact.  No atomics; deterministic; a row does not depend on the other rows.
 * ------------------------------------------------------------------------------------------------- */
int aid_ar_score(const aid_bwe_gather_params* p, void* stream);
int aid_click_mask(const aid_fir_observed_params* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AID_BWE_LONG_H */
