/*
 * aid_spec_long.h -- C ABI of spectrogram inpainting of whole recordings in libaid_hip.so (gfx950): the observation operator of a
 * window seen through the STFT-domain masking operator of aid_stft_frames / aid_stft_ola (aid_kernels.h), and the gather that builds
 * its per-window inputs.
 *
 * All positions are in RECORDING coordinates.  A recording of N samples is padded to Np = N + (n_fft - N % n_fft) and has
 * T_rec = 1 + Np / hop frames; half = n_fft / 2.  Frame t reads the positions q = t*hop - half + j, j in [0, n_fft), through
 *      q < 0  ->  -q,        q >= Np  ->  2 (Np - 1) - q,        value = q < N ? x[q] : 0
 * (torch.stft: centred, reflect padding, after the zero padding to Np), and the recording's operator is
 *      A(x)[n] = 1/env[n] * sum_t w[n + half - t*hop] * (F^-1 diag(mask[:, t]) F (w . frame_t))[n + half - t*hop]
 * over the frames t in [0, T_rec) that cover n; env is the overlap-added squared window over the same frames.
 *
 * The recording is restored on the window grid of aid_restore.h with every window start s a multiple of hop (spec_long.py): window
 * frame j is then recording frame s / hop + j, and Tw = 1 + (L + n_fft) / hop covers every frame a window can compute.  The window
 * holds x[s, s + L); samples at s + i >= N are absent and enter as 0.  Frame t is COMPUTABLE in the window when every position it
 * reads, after the two reflections, is either >= N or inside [s, s + L).  A window's STATE row has L + Tw entries, one float per
 * sample and one per frame:
 *
 *   sample i               -2   absent                         (s + i >= N)
 *                           1   known:       y = x[i]          (an overlap sample another window restored)
 *                           0   observed:    y = A(x)[s + i]   (every frame of the recording that covers s + i is computable)
 *                          -1   unobserved                     (the sample exists and feeds frames; its own y depends on samples
 *                                                               outside the window)
 *   frame j                -2   absent                         (s / hop + j >= T_rec)
 *                          -1   not computable
 *                           0   computable
 *
 * Any state > 0 is read as 1, any state <= -2 as -2; a sample is observed and a frame is run only when its state == 0.
 * An ITEM row is 3 int64: (r, s, N) -- the recording (its row of the mask), the window start and the recording's length.  All items of
 * a call share Np (N in [Np - n_fft, Np)), and with it T_rec and the envelope table.
 *
 * Same boundary contract as aid_kernels.h: raw device pointers, sizes, offsets and strides in ELEMENTS, a hipStream_t passed as
 * void*, 0 or a negative AID_E_* code, no allocation, no synchronisation.
 */
#ifndef AID_SPEC_LONG_H
#define AID_SPEC_LONG_H

#include <stdint.h>
#include "aid_kernels.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AID_SPEC_LONG_ABI_VERSION 1
#define AID_SPEC_ITEM_FIELDS 3
int aid_spec_long_abi_version(void);

/* ---------------------------------------------------------------------------------------------------
 * aid_stft_mask_observed -- state [B, L + Tw] (row stride state_ld >= L + Tw), items [B, 3] contiguous; kh = state[b, i],
 *   kf = state[b, L + j]; xin = kh <= -2 ? 0 : x.  With c[i] = 1/env[s + i] * sum over the frames j with kf[j] == 0 that cover s + i
 *   of the masked frame of xin (the frame reads the window through the reflection rule; a position outside [s, s + L) reads 0):
 *   mode 0 (apply):    out[i] = kh > 0 ? x[i] : (kh == 0 ? c[i] : 0)
 *   mode 1 (adjoint):  x is the gradient g; with a = the transpose of c over the same frames, applied to (kh == 0 ? g : 0):
 *                      out[i] = kh <= -2 ? 0 : (kh > 0 ? a[i] + g[i] : a[i])
 *   mode 2 (project):  out[i] = kh > 0 ? y[i] : (kh == 0 ? (-c[i] + y[i]) + x[i] : x[i])
 *   x, y, out [B, L] with row strides x_ld, y_ld, out_ld >= L (y is read in mode 2 only).  mask: the recordings' masks [Rm, F, T_rec]
 *   read in place, item stride mask_sB (0: one mask shared by all recordings; r is then not read), bin stride mask_ld >= T_rec, unit
 *   stride along T; window frame j multiplies by column s / hop + j of recording r.  inv_env [Np]: 1 / env of the recording.  window
 *   [n_fft], twiddle [n_fft/2] complex, as aid_stft_frames takes them.  frames [B, Tw, n_fft] contiguous is scratch: written for the
 *   frames with kf == 0 only, and only those are read.
 *   Two launches per call: one workgroup per (item, window frame) -- a frame with kf != 0 leaves before any LDS traffic and runs no
 *   FFT -- then one lane per sample, which gathers the covering frames in ascending order (no atomics, deterministic) and applies
 *   1/env and the select.  The sums are those of aid_stft_frames / aid_stft_ola, with the same terms in the same order: with N = L,
 *   s = 0 and every sample state 0 the three modes give that operator's apply, adjoint and c0 = -1 projection bit for bit.
 *   The item table is device memory: an item with s < 0, s no multiple of hop, s >= N, N outside [max(1, Np - n_fft), Np) or (with
 *   mask_sB != 0) r outside [0, Rm) runs no frame and has c = a = 0.
 *   n_fft a power of two in [16, 8192]; hop divides n_fft; Np a multiple of n_fft; n_frames == 1 + (L + n_fft) / hop;
 *   1 <= B <= 65535.  out must not overlap an input.
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    const float* x; const float* y; const float* state; const int64_t* items;
    const float* window; const float* twiddle; const float* inv_env; const float* mask;
    float* frames; float* out;
    int64_t L, Np, x_ld, y_ld, state_ld, out_ld, mask_sB, mask_ld;
    int B, Rm, n_fft, hop, n_frames, mode;
} aid_stft_mask_observed_params;
int aid_stft_mask_observed(const aid_stft_mask_observed_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * aid_spec_gather -- for job j of the table of aid_restore.h (r, s, head, tail, lo, hi; 6 int64); the first match decides.
 *   Sample i < L, q = s_j + i:
 *     q >= N                                                   state[j, i] = -2,  y[j, i] = 0
 *     i < head_j  or  i >= L - tail_j                          state[j, i] =  1,  y[j, i] = out[r_j, q]
 *     every frame t in [0, T_rec) that covers q is computable  state[j, i] =  0,  y[j, i] = rec[r_j, q]
 *     otherwise                                                state[j, i] = -1,  y[j, i] = 0
 *   Frame f < Tw = n_frames, t = s_j / hop + f:
 *     t >= T_rec                                               state[j, L + f] = -2
 *     frame t is not computable in [s_j, s_j + L)              state[j, L + f] = -1
 *     otherwise                                                state[j, L + f] =  0
 *   items[j] = (r_j, s_j, N).
 *   rec: the masked recordings [R, N], row stride rec_ld >= N; out: the result so far [R, N], row stride out_ld >= N; y: contiguous
 *   [J, L]; state: contiguous [J, L + Tw]; items: contiguous [J, 3].  They must not overlap rec or out.  Np == N + (n_fft - N % n_fft),
 *   n_frames == 1 + (L + n_fft) / hop.  The table is device memory: a job whose r is outside [0, R), whose s is outside [0, N) or no
 *   multiple of hop is skipped (y = 0, state = -2 over its rows, items[j] = (-1, -1, 0)); head and tail are clamped to [0, L].  One
 *   launch serves a whole pass; copies only (bit-exact).  The samples go back with aid_window_scatter.
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    const float* rec; const float* out;
    float* y; float* state; int64_t* items;
    const int64_t* jobs;
    int64_t L, N, Np, rec_ld, out_ld;
    int J, R, n_fft, hop, n_frames;
} aid_spec_gather_params;
int aid_spec_gather(const aid_spec_gather_params* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AID_SPEC_LONG_H */
