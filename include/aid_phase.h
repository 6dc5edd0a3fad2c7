/*
 * aid_phase.h -- C ABI of the phase-retrieval pieces of libaid_hip.so (gfx950): the STFT-magnitude operator of the
 * reference's SamplerPhaseRetrieval (testing/edm_sampler.py:308-335) with its vector-Jacobian product, and the guidance
 * seed of the induced matrix norms that torch.linalg.norm(y - A(x_hat), dim=(1, 2), ord=1 | 2) takes over 3-D
 * observations (testing/edm_sampler_inpainting.py:67-75).
 *
 * Same boundary contract as aid_kernels.h: raw device pointers, sizes and row strides in ELEMENTS, a hipStream_t
 * passed as void*, 0 or a negative AID_E_* code, no allocation, no synchronisation.
 */
#ifndef AID_PHASE_H
#define AID_PHASE_H

#include <stdint.h>
#include "aid_kernels.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AID_PHASE_ABI_VERSION 1
int aid_phase_abi_version(void);

/* ---------------------------------------------------------------------------------------------------
 * aid_stft_mag -- |STFT| of the zero-extended signal, center=False, one-sided, unnormalised:
 *   X[b, k, t] = sum_{j<N} window[j] * x[b, t*hop + j] * exp(-2 pi i j k / N),  x = 0 at and past L
 *   (torch.stft(cat(x, zeros(N)), N, hop, window, center=False): T = 1 + L / hop frames, F = N/2 + 1 bins)
 *   adjoint = 0:  out[b, k, t] = |X[b, k, t]|                        x [B, L] (row stride x_ld) -> out [B, F, T] contiguous
 *   adjoint = 1:  the VJP at x (the x_hat of the matching forward; X is recomputed from it):
 *                 out[b, q] = sum_t window[q - t*hop] * Re( IFFT_N(Z_t) )[q - t*hop],  q < L   (IFFT unnormalised)
 *                 Z_t[k] = g[b, k, t] * X[b, k, t] / |X[b, k, t]| for k <= N/2 (0 where |X| = 0), Z_t[k] = 0 above
 *                 g [B, F, T] contiguous -> out [B, L] (row stride out_ld); frames [B, T, N] contiguous is scratch
 *                 (written by the frame pass, read by the overlap-add gather; no atomics, deterministic).
 *   window [N], twiddle [N/2] complex (cos, -sin)(2 pi m / N) as float2.
 *   N = n_fft a power of two in [16, 8192]; 0 < hop <= N; n_frames = 1 + L / hop.
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    const float* x; const float* g; float* out; float* frames;
    const float* window; const float* twiddle;
    int B, n_fft, hop, n_frames, adjoint;
    int64_t L, x_ld, out_ld;
} aid_stft_mag_params;
int aid_stft_mag(const aid_stft_mag_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * aid_matrix_norm_seed -- induced norm of R_b = y_b - den_b, viewed as an F x T matrix per item, and its seed
 *   g = d norm / d den = -d norm / d R (the sign convention of aid_guidance_seed).  One workgroup per item; the result
 *   of item b does not depend on the other items.  den, y, g are [B, F, T] contiguous.
 *   ord 1:  norm = max_t sum_f |R[f, t]| (fp64 sums); g = -sign(R) on the arg-max column, divided by the number of
 *           columns that tie exactly (torch.amax's backward).
 *   ord 2:  norm = sigma_1(R); g = -u_1 v_1^T.  Power iteration on R^T R in fp64 from v_0 = the column 2-norms of R
 *           (data-derived, no state across calls), stopped when ||R^T u - sigma v|| / sigma <= tol (u = R v / ||R v||,
 *           sigma = ||R v||) or after max_iter iterations; the triplet of the last iteration is used either way.
 *           r [B, F, T] fp32 scratch receives R.  diag [B, 2] (optional): iterations run, final residual.
 *   (F + T) * 8 + 256 bytes of LDS per workgroup: F + T <= 8160.
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    const float* den; const float* y; float* g; float* norm;
    float* r; float* diag;
    int B, F, T, ord, max_iter;
    double tol;
} aid_matrix_norm_params;
int aid_matrix_norm_seed(const aid_matrix_norm_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Blind bandwidth extension (blind.py): the statistics and the fit of a one-knee low-pass, on the two parameter blocks above.
 *
 * aid_stft_band_stats -- on aid_stft_mag_params, with the framing, window and twiddle of aid_stft_mag (T = n_frames, F = N/2 + 1):
 *   x [B, L] (row stride x_ld) = the current estimate x_hat; g [B, F, T] contiguous = |Y|, an output of aid_stft_mag;
 *   out [B, 2, F] contiguous:  out[b, 0, k] = Sxx = sum_t |X[b, k, t]|^2,   out[b, 1, k] = Sxy = sum_t |X[b, k, t]| * g[b, k, t]
 *   |X| carries aid_stft_mag's bits (the same frame body).  frames [B, T, 2, F] contiguous is scratch: one workgroup per frame writes
 *   its fp32 products there, a second pass adds them over t = 0 .. T-1 in fp64 and rounds once.  No atomics; deterministic; item b
 *   does not depend on the other items.  adjoint must be 0, g and frames non-null; out_ld is not read.
 *
 * aid_lowpass_fit -- on aid_matrix_norm_params, one workgroup per item, fp64, static LDS only, nothing kept between calls:
 *   den  = stats [B, 2, F], an output of aid_stft_band_stats                                                            (read)
 *   y    = a float table [NC + NA + 2]: cut-off candidates c_j > 0 in bins, slope candidates A_i < 0 in dB per octave,
 *          then floor_dB (< 0) and k_lo (>= 0, a whole number)                                                          (read)
 *   r    = the tap window w [K]                                                                                         (read)
 *   g    = taps [B, K]                                                                                                  (written)
 *   norm = fit [B, 4]: c, A, cost, number of valid bins                                                                 (written)
 *   diag = must be null;   T = NC,  ord = NA,  max_iter = K (odd, K <= N - 1, N = 2 (F - 1)),  tol = eps;   F in [9, 1025]
 *   H(k; c, A) = 10^(max(floor_dB, min(0, A log2(k / c))) / 20) for k > c, 1 for k <= c;   gmin = 10^(floor_dB / 20)
 *   g_k = clamp(Sxy_k / Sxx_k, gmin, 1);  bin k is valid when k >= k_lo and Sxx_k >= eps * max_k Sxx_k and Sxx_k > 0
 *   cost(j, i) = mean over the valid bins of (H(k; c_j, A_i) - g_k)^2  (0 without a valid bin); the lowest cost wins, ties go to the
 *   lowest j, then the lowest i.  With (c, A) the winner, P = (K - 1) / 2 and H_k = H(k; c, A):
 *   taps[b, n] = w[n] / N * (H_0 + 2 sum_{k=1}^{N/2-1} H_k cos(2 pi k (n - P) / N) + H_{N/2} cos(pi (n - P))),  rounded to fp32 once.
 *
 * aid_lowpass_fit_groups -- aid_lowpass_fit on statistics pooled over groups of items (blind_long.py: one filter per recording, fitted
 *   to all its probe windows together), on aid_matrix_norm_params with aid_lowpass_fit's fields and
 *   diag = the group ids: B ints in HOST memory behind the float pointer, group[b] in [0, B), B <= AID_LOWPASS_FIT_MAX_ITEMS.  The
 *          launcher reads them before it returns -- so it can refuse an id outside [0, B) -- and hands them to the kernel with its
 *          arguments; the memory may be reused as soon as the call returns.
 *   For item b,  S[s, k] = sum over the items b' with group[b'] == group[b], in ascending b', of stats[b', s, k]  in fp64, and fit[b]
 *   and taps[b] are those of aid_lowpass_fit on S: the same code on the same candidates, S not rounded to fp32.  Every item of a group
 *   gets the same bits; with every item in a group of its own the output is aid_lowpass_fit's bit for bit.  One workgroup per item;
 *   static LDS only; no atomics, nothing kept between calls.  Deterministic.
 * ------------------------------------------------------------------------------------------------- */
#define AID_LOWPASS_FIT_MAX_ITEMS 256
int aid_stft_band_stats(const aid_stft_mag_params* p, void* stream);
int aid_lowpass_fit(const aid_matrix_norm_params* p, void* stream);
int aid_lowpass_fit_groups(const aid_matrix_norm_params* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AID_PHASE_H */
