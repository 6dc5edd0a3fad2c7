/*
 * aid_phase_long.h -- C ABI of phase retrieval of whole recordings in libaid_hip.so (gfx950): the observation operator of a window
 * seen through the STFT magnitude of aid_stft_mag (aid_phase.h), and the gather that builds its per-window inputs.
 *
 * A recording of N samples is known only by its magnitude spectrogram rec [F, T_rec] (F = n_fft/2 + 1, T_rec = 1 + N / hop: frame t
 * reads samples [t*hop, t*hop + n_fft), zeros at and past N).  It is restored on the window grid of aid_restore.h with every window
 * start a multiple of hop (phase_long.py): frame j of a window that starts at s is then frame s / hop + j of the recording --
 * exactly, wherever the window holds the frame's n_fft samples or the recording ends inside it.  With Tw = 1 + L / hop a window's
 * observation row has L + F*Tw entries: the first L are samples (entry i is sample s + i), the rest is the [F, Tw] magnitude block
 * with frames contiguous (aid_stft_mag's layout).  Its STATE row has L + Tw entries, one float per sample and one per frame:
 *
 *   sample i                1   known:       y = x[i]          (an overlap sample another window restored)
 *                          -1   no direct observation          (the sample exists; it is seen through the STFT only)
 *                          -2   absent                         (beyond the end of the recording: it enters the STFT as 0)
 *   frame j                 0   observed:    y[k, j] = |FFT(window * xin[j*hop ...])|_k
 *                          -1   unobserved                     (the frame leaves the window although the recording goes on)
 *                          -2   absent                         (beyond the last frame of the recording)
 *
 * Any state > 0 is read as 1, any state <= -2 as -2; a frame is observed only when its state == 0.
 *
 * Same boundary contract as aid_kernels.h: raw device pointers, sizes, offsets and strides in ELEMENTS, a hipStream_t passed as
 * void*, 0 or a negative AID_E_* code, no allocation, no synchronisation.
 */
#ifndef AID_PHASE_LONG_H
#define AID_PHASE_LONG_H

#include <stdint.h>
#include "aid_kernels.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AID_PHASE_LONG_ABI_VERSION 1
int aid_phase_long_abi_version(void);

/* ---------------------------------------------------------------------------------------------------
 * aid_stft_mag_observed -- state [B, L + Tw] (row stride state_ld >= L + Tw, or one shared row: state_ld = 0), kh = state[b, i],
 *   kf = state[b, L + j]; F = n_fft/2 + 1, Tw = n_frames = 1 + L / hop; samples at and past L are 0.
 *   mode 0 (apply):  x [B, L] (x_ld >= L) -> out [B, L + F*Tw] (out_ld >= L + F*Tw); g is not read
 *                    xin = kh <= -2 ? 0 : x
 *                    out[i]              = kh > 0 ? x[i] : 0
 *                    out[L + k*Tw + j]   = kf == 0 ? |FFT(window * xin[j*hop ...])|_k : 0
 *   mode 1 (VJP):    x [B, L] (the point of linearisation), g [B, L + F*Tw] (g_ld >= L + F*Tw) -> out [B, L] (out_ld >= L)
 *                    a = aid_stft_mag's adjoint of the magnitude part of g over the observed frames only, taken at xin
 *                    out[q] = kh <= -2 ? 0 : (kh > 0 ? a[q] + g[q] : a[q])
 *                    frames [B, Tw, n_fft] contiguous is scratch: written for the observed frames only, and only those are read.
 *   window [n_fft], twiddle [n_fft/2] complex, as aid_stft_mag takes them.  One workgroup per (item, frame); an unobserved or absent
 *   frame runs no FFT.  The sums are those of aid_stft_mag, with the same terms in the same order: with every frame observed and no
 *   sample known or absent, the magnitude block of mode 0 and mode 1 on [0 | g] give that kernel's bits.  Selections are exact: a
 *   known output of mode 0 is x itself.  Bins with |X| = 0 contribute 0 (an observed frame over absent samples only gives magnitude 0
 *   and gradient 0).  Mode 0 is one launch, mode 1 two; no atomics, a fixed summation order.
 *   n_fft a power of two in [16, 8192]; 0 < hop <= n_fft; 1 <= B <= 65535.  out must not overlap an input.
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    const float* x; const float* g; const float* state;
    const float* window; const float* twiddle;
    float* frames; float* out;
    int64_t L, x_ld, g_ld, state_ld, out_ld;
    int B, n_fft, hop, n_frames, mode;
} aid_stft_mag_observed_params;
int aid_stft_mag_observed(const aid_stft_mag_observed_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * aid_pr_gather -- for job j of the table of aid_restore.h (r, s, head, tail, lo, hi; 6 int64); the first match decides.
 *   Sample i < L, q = s_j + i:
 *     q >= N                                                   state[j, i] = -2,  y[j, i] = 0
 *     i < head_j  or  i >= L - tail_j                          state[j, i] =  1,  y[j, i] = out[r_j, q]
 *     otherwise                                                state[j, i] = -1,  y[j, i] = 0
 *   Frame f < Tw = n_frames, t = s_j / hop + f, every bin k < F:
 *     t >= T_rec                                               state[j, L + f] = -2,  y[j, L + k*Tw + f] = 0
 *     s_j + L < N  and  f*hop + n_fft > L                      state[j, L + f] = -1,  y[j, L + k*Tw + f] = 0
 *     otherwise                                                state[j, L + f] =  0,  y[j, L + k*Tw + f] = rec[r_j, k, t]
 *   rec: the magnitude spectrograms [R, F, T_rec], item stride rec_ld, bin stride rec_bin_ld >= T_rec, unit stride along T
 *   (rec_ld >= (F - 1) * rec_bin_ld + T_rec); out: the result so far [R, N], row stride out_ld >= N; y: contiguous
 *   [J, L + F*Tw]; state: contiguous [J, L + Tw].  y and state must not overlap rec or out.  T_rec == 1 + N / hop,
 *   n_frames == 1 + L / hop.  The table is device memory: a job whose r is outside [0, R), whose s is outside [0, N) or no multiple
 *   of hop is skipped (y = 0, state = -2 over its rows); head and tail are clamped to [0, L].  One launch serves a whole pass; copies
 *   only (bit-exact).  The samples go back with aid_window_scatter.
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    const float* rec; const float* out;
    float* y; float* state;
    const int64_t* jobs;
    int64_t L, N, T_rec, rec_ld, rec_bin_ld, out_ld;
    int J, R, n_fft, hop, n_frames;
} aid_pr_gather_params;
int aid_pr_gather(const aid_pr_gather_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * aid_stft_logspec_dist -- the per-frame log-spectral distance between an estimate and a reference (metrics.py), on the parameter
 *   block of aid_stft_mag_observed, with the framing, window and twiddle of aid_stft_mag (zero-extended signals, center=False,
 *   T = n_frames = 1 + L / hop).  What every field means here:
 *   x       the estimate  [B, L], row stride x_ld >= L                                                                    (read)
 *   g       the reference [B, L], row stride g_ld >= L                                                                    (read)
 *   state   the region weights [B, L], row stride state_ld >= L, or one shared row (state_ld = 0); 0 or non-zero, not fractional;
 *           null: every sample counts                                                                                     (read)
 *   window  [n_fft];  twiddle [n_fft/2] complex                                                                           (read)
 *   frames  the band: 3 floats in HOST memory, k_lo, k_hi (whole numbers, 0 <= k_lo <= k_hi <= n_fft/2) and floor >= 0.  The
 *           launcher reads them before it returns -- so it can refuse a band outside the spectrum -- and hands them to the
 *           kernel with its arguments; the memory may be reused as soon as the call returns.                              (read)
 *   out     [B, T], row stride out_ld >= T                                                                                (written)
 *   mode    must be 0
 *   A frame t is COUNTED when it holds a sample q < L, t*hop <= q < t*hop + n_fft, whose weight is non-zero; without weights that is
 *   every frame with t*hop < L (the trailing frame at t = L / hop when hop divides L holds no sample).  With R, E the spectra of the
 *   reference and the estimate over the frame,
 *       out[b, t] = sqrt( 1/(k_hi - k_lo + 1) * sum_{k = k_lo .. k_hi} (log10(|R_k|^2 + floor) - log10(|E_k|^2 + floor))^2 )
 *   for a counted frame and -1 for any other, which runs no FFT.  |R_k|^2 and |E_k|^2 are fp32, the logarithms and the sum over the
 *   bins fp64: lane l of 256 adds the bins k_lo + l, k_lo + l + 256, ... ascending and the partial sums are added as a fixed binary
 *   tree.  One workgroup per (item, frame); no atomics, a second launch gives the same bits; item b does not depend on the others.
 *   n_fft a power of two in [16, 8192]; 0 < hop <= n_fft; B * T < 2^31.
 * ------------------------------------------------------------------------------------------------- */
int aid_stft_logspec_dist(const aid_stft_mag_observed_params* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AID_PHASE_LONG_H */
