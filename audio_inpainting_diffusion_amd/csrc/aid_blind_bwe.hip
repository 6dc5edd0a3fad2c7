// Blind bandwidth extension (blind.py): the low-pass that degraded a recording is not given, it is fitted to the current estimate inside
// every guided evaluation -- three launches on the caller's stream, no host round trip.  Declared in include/aid_phase.h (statistics and
// fit, on the parameter blocks of aid_stft_mag and aid_matrix_norm_seed) and include/aid_bwe_long.h (the filter with one tap row per item).
//
//   band_stats_frames_kernel : one workgroup per (item, frame), the frame body of aid_stft_mag (pm_frame_fft, aid_stft_mag_tile.h): |X_k|, then
//                              the two products |X_k|^2 and |X_k| |Y_k| of the frame go to the scratch [B, T, 2, F] (bins contiguous).  x_hat is
//                              read n_fft / hop times through LDS, |Y| once.
//   band_stats_sum_kernel    : grid (tiles of 64 of the 2 F columns, items); 4 lane groups add a quarter of the frames each, ascending, in fp64,
//                              and the four partial sums are added in group order: a fixed order, no atomics.
//   lowpass_fit_kernel       : one workgroup of 1024 lanes per item, all in fp64: the fit and the tap design of aid_lowpass_fit.h on the
//                              statistics of the item.
//   fir_observed_items_kernel: fir_observed_kernel of aid_bwe_long.hip with the taps of item b at h + b * K (the tile loop fir_tile).
#include "aid_rows.h"
#include "aid_fir_tile.h"
#include "aid_stft_mag_tile.h"
#include "aid_lowpass_fit.h"
#include "aid_phase.h"
#include "aid_bwe_long.h"

#define BS_COLS 64                        // columns of the scratch per workgroup of the sum pass
#define BS_GROUPS 4                       // lane groups that share the frames of a column

// ---- band statistics -------------------------------------------------------------------------------------------------
struct bs_row {                                                    // sample q of the row, 0 at and past L
    const float* __restrict__ x; int64_t L;
    __device__ __forceinline__ float operator()(int64_t q) const { return q < L ? x[q] : 0.f; }
};

__global__ __launch_bounds__(STFT_THREADS) void band_stats_frames_kernel(const aid_stft_mag_params p) {
    const int b = blockIdx.x / p.n_frames, t = blockIdx.x - b * p.n_frames;
    extern __shared__ __attribute__((aligned(16))) float2 bs_lds[];
    const int N = p.n_fft, F = (N >> 1) + 1, T = p.n_frames;
    const float2* X = pm_frame_fft(bs_row{p.x + (int64_t)b * p.x_ld, p.L}, (int64_t)t * p.hop, N, p.window, p.twiddle, bs_lds, bs_lds + N);
    const float* __restrict__ y = p.g + (int64_t)b * F * T + t;
    float* __restrict__ part = p.frames + ((int64_t)b * T + t) * 2 * F;
    for (int k = threadIdx.x; k < F; k += STFT_THREADS) {
        const float2 c = X[k];
        const float m = sqrtf(c.x * c.x + c.y * c.y);
        part[k] = m * m;
        part[F + k] = m * y[(int64_t)k * T];
    }
}

__global__ __launch_bounds__(BS_COLS * BS_GROUPS) void band_stats_sum_kernel(const aid_stft_mag_params p) {
    __shared__ double part[BS_GROUPS][BS_COLS];
    const int b = blockIdx.y, T = p.n_frames, F2 = 2 * ((p.n_fft >> 1) + 1);
    const int col = threadIdx.x % BS_COLS, grp = threadIdx.x / BS_COLS, j = blockIdx.x * BS_COLS + col;
    const int per = (T + BS_GROUPS - 1) / BS_GROUPS, t0 = grp * per, t1 = min(T, t0 + per);
    double s = 0.0;
    if (j < F2) {
        const float* __restrict__ fr = p.frames + (int64_t)b * T * F2 + j;
#pragma unroll 8
        for (int t = t0; t < t1; ++t) s += (double)fr[(int64_t)t * F2];
    }
    part[grp][col] = s;
    __syncthreads();
    if (grp == 0 && j < F2) {
        double a = part[0][col];
#pragma unroll
        for (int g = 1; g < BS_GROUPS; ++g) a += part[g][col];
        p.out[(int64_t)b * F2 + j] = (float)a;
    }
}

extern "C" int aid_stft_band_stats(const aid_stft_mag_params* p, void* stream) {
    AID_REQUIRE(p && p->x && p->g && p->out && p->frames && p->window && p->twiddle, "aid_stft_band_stats: null pointer");
    AID_REQUIRE(!p->adjoint, "aid_stft_band_stats: adjoint must be 0");
    AID_REQUIRE(p->n_fft >= 16 && p->n_fft <= 4096 && (p->n_fft & (p->n_fft - 1)) == 0, "aid_stft_band_stats: n_fft must be a power of two in [16, 4096]");
    AID_REQUIRE(p->hop > 0 && p->hop <= p->n_fft, "aid_stft_band_stats: hop must be in [1, n_fft]");
    AID_REQUIRE(p->B > 0 && p->B <= 65535 && p->L > 0 && p->x_ld >= p->L, "aid_stft_band_stats: bad shape or row stride (1 <= B <= 65535)");
    AID_REQUIRE(p->n_frames == 1 + p->L / p->hop, "aid_stft_band_stats: n_frames must be 1 + L / hop");
    AID_REQUIRE((int64_t)p->B * p->n_frames <= 0x7fffffff, "aid_stft_band_stats: too many frames");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)p->n_fft * 2 * sizeof(float2);
    hipLaunchKernelGGL(band_stats_frames_kernel, dim3(p->B * p->n_frames), dim3(STFT_THREADS), lds, st, *p);
    AID_CHECK_LAUNCH();
    hipLaunchKernelGGL(band_stats_sum_kernel, dim3(aid_cdiv(p->n_fft + 2, BS_COLS), p->B), dim3(BS_COLS * BS_GROUPS), 0, st, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}

// ---- the fit ---------------------------------------------------------------------------------------------------------
// (the body is lf_fit_and_design of aid_lowpass_fit.h, shared with lowpass_fit_groups_kernel of aid_blind_long.hip)
__global__ __launch_bounds__(LF_THREADS) void lowpass_fit_kernel(const aid_matrix_norm_params p) {
    __shared__ lf_lds lds;
    const int b = blockIdx.x, F = p.F;
    const float* __restrict__ st = p.den + (int64_t)b * 2 * F;
    lf_fit_and_design(lds, [&](int s, int k) { return (double)st[s * F + k]; }, F, p.T, p.ord, p.max_iter, p.y, p.tol, p.r,
                      p.norm + (int64_t)b * 4, p.g + (int64_t)b * p.max_iter);
}

extern "C" int aid_lowpass_fit(const aid_matrix_norm_params* p, void* stream) {
    AID_REQUIRE(p && p->den && p->y && p->r && p->g && p->norm, "aid_lowpass_fit: null pointer");
    AID_REQUIRE(!p->diag, "aid_lowpass_fit: diag must be null");
    AID_REQUIRE(p->B > 0, "aid_lowpass_fit: empty batch");
    const int N = 2 * (p->F - 1);
    AID_REQUIRE(p->F <= LF_MAX_F && N >= 16 && (N & (N - 1)) == 0, "aid_lowpass_fit: F must be n_fft / 2 + 1 for a power of two n_fft in [16, 2048]");
    AID_REQUIRE(p->T >= 1 && p->ord >= 1 && (int64_t)p->T * p->ord < 0x7fffffff, "aid_lowpass_fit: the candidate tables must hold 1 <= NC, NA and NC * NA < 2^31");
    AID_REQUIRE(p->max_iter >= 1 && (p->max_iter & 1) && p->max_iter <= N - 1, "aid_lowpass_fit: K must be odd and in [1, n_fft - 1]");
    AID_REQUIRE(p->tol >= 0.0, "aid_lowpass_fit: eps must be >= 0");
    hipLaunchKernelGGL(lowpass_fit_kernel, dim3(p->B), dim3(LF_THREADS), 0, (hipStream_t)stream, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}

// ---- the filter with one tap row per item ---------------------------------------------------------------------------------
// MODE 0 apply, 1 adjoint, 2 projection (fir_observed_kernel of aid_bwe_long.hip; the taps of item b are h + b * K)
template <int MODE>
__global__ __launch_bounds__(FIR_THREADS) void fir_observed_items_kernel(const aid_fir_observed_params p) {
    const int64_t b = blockIdx.y, L = p.L;
    const int t = threadIdx.x;
    const int64_t tile0 = (int64_t)blockIdx.x * FIR_TO;
    const float* __restrict__ x = p.x + b * p.x_ld;
    const float* __restrict__ k = p.state + b * p.state_ld;
    const float* __restrict__ h = p.h + b * p.K;
    const int P = (p.K - 1) / 2;
    double accd[FIR_R];
    if (MODE == 1) fir_tile([&](int64_t q) { return (q >= 0 && q < L && k[q] == 0.f) ? x[q] : 0.f; }, tile0, h, p.K, p.K - 1 - P, 1, accd);
    else           fir_tile([&](int64_t q) { return (q >= 0 && q < L && !rs_absent(k[q])) ? x[q] : 0.f; }, tile0, h, p.K, P, 0, accd);
    float* __restrict__ out = p.out + b * p.out_ld;
#pragma unroll
    for (int r = 0; r < FIR_R; ++r) {
        const int64_t i = tile0 + t * FIR_R + r;
        if (i < L) {
            const float c = (float)accd[r], kv = k[i], xv = x[i];
            float v;
            if (MODE == 0) v = rs_known(kv) ? xv : (kv == 0.f ? c : 0.f);
            else if (MODE == 1) v = rs_absent(kv) ? 0.f : (rs_known(kv) ? c + xv : c);
            else {
                const float yv = p.y[b * p.y_ld + i];
                v = rs_known(kv) ? yv : (kv == 0.f ? (yv - c) + xv : xv);
            }
            out[i] = v;
        }
    }
}

extern "C" int aid_fir_observed_items(const aid_fir_observed_params* p, void* stream) {
    AID_REQUIRE(p && p->x && p->state && p->h && p->out, "aid_fir_observed_items: null pointer");
    AID_REQUIRE(p->mode >= 0 && p->mode <= 2, "aid_fir_observed_items: mode must be 0 (apply), 1 (adjoint) or 2 (projection)");
    AID_REQUIRE(p->mode != 2 || (p->y && p->y_ld >= p->L), "aid_fir_observed_items: the projection needs y with a row stride >= L");
    AID_REQUIRE(p->B > 0 && p->B <= 65535 && p->K > 0 && p->L > 0, "aid_fir_observed_items: empty or oversized shape (1 <= B <= 65535, K >= 1)");
    AID_REQUIRE(p->x_ld >= p->L && p->out_ld >= p->L && (p->state_ld == 0 || p->state_ld >= p->L), "aid_fir_observed_items: a row stride is shorter than L");
    const dim3 grid(aid_cdiv(p->L, FIR_TO), p->B), block(FIR_THREADS);
    if (p->mode == 0) hipLaunchKernelGGL(fir_observed_items_kernel<0>, grid, block, 0, (hipStream_t)stream, *p);
    else if (p->mode == 1) hipLaunchKernelGGL(fir_observed_items_kernel<1>, grid, block, 0, (hipStream_t)stream, *p);
    else hipLaunchKernelGGL(fir_observed_items_kernel<2>, grid, block, 0, (hipStream_t)stream, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}
