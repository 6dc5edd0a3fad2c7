// Objective restoration metrics (metrics.py): the per-frame log-spectral distance between an estimate and a reference, and the weighted
// time-domain sums behind SNR and SI-SDR.  Declared in include/aid_phase_long.h (aid_stft_logspec_dist, on the parameter block of
// aid_stft_mag_observed) and include/aid_bwe_long.h (aid_eval_sums, on that of aid_fir_observed).
//
//   logspec_dist_kernel : one workgroup of STFT_THREADS lanes per (item, frame), with the framing, window and twiddles of aid_stft_mag.  The
//                         workgroup first looks for a counted sample (q < L with a non-zero weight) in its frame; without one it writes -1 and
//                         runs no FFT.  Otherwise two FFTs on pm_frame_fft (aid_stft_mag_tile.h): the reference, whose powers |R_k|^2 of the
//                         band go to an fp32 table in LDS, then the estimate.  Lane l takes the bins k_lo + l, k_lo + l + 256, ... ascending:
//                         d = log10(|R_k|^2 + floor) - log10(|E_k|^2 + floor) and its square in fp64; the 256 partial sums are added as a
//                         fixed binary tree in LDS.  Two FFTs rather than one complex FFT split by Hermitian symmetry: the split would leak
//                         the rounding of the louder signal into the bins where the other one is quiet.
//                         LDS: 2 N float2 for the FFT, N/2 + 2 floats of powers, 256 doubles: 146 KB at N = 8192, one workgroup per CU.
//   eval_sums_kernel    : one workgroup of 512 lanes per item.  Lane l takes the samples l, l + 512, ... ascending and keeps n, sum r^2,
//                         sum e^2, sum r e, sum (r - e)^2 and max |r - e| over the counted ones in fp64 (the products of two fp32 numbers are
//                         exact there), then the frames l, l + 512, ... of the distances: how many are >= 0 and their sum.  The eight rows of
//                         512 partial results are reduced as a fixed binary tree in LDS (sum, or max for the sixth).
//   No atomics in either: a second launch gives the same bits, and item b does not depend on the other items.
#include "aid_common.h"
#include "aid_stft_mag_tile.h"
#include "aid_phase_long.h"
#include "aid_bwe_long.h"

#define EV_MAX_LDS (8192 * 2 * 8 + (4096 + 2) * 4 + STFT_THREADS * 8)   // 149512 bytes of the 160 KB of a CU
#define ES_THREADS 512
#define ES_SUMS 8

struct ev_row {                                                    // sample q of the row, 0 at and past L
    const float* __restrict__ x; int64_t L;
    __device__ __forceinline__ float operator()(int64_t q) const { return q < L ? x[q] : 0.f; }
};

struct ev_dist_args {                                              // the kernel's arguments: the caller's block and the checked band
    aid_stft_mag_observed_params p;
    int k_lo, k_hi;
    float floor;
};

__global__ __launch_bounds__(STFT_THREADS) void logspec_dist_kernel(const ev_dist_args a) {
    const aid_stft_mag_observed_params& p = a.p;
    const int b = blockIdx.x / p.n_frames, t = blockIdx.x - b * p.n_frames;
    extern __shared__ __attribute__((aligned(16))) float2 ev_lds[];
    const int N = p.n_fft, nb = a.k_hi - a.k_lo + 1;
    const int64_t s0 = (int64_t)t * p.hop;
    float* out = p.out + (int64_t)b * p.out_ld + t;
    // counted: a sample q = s0 + j < L, j < N, with a non-zero weight (s0 <= L because t <= L / hop)
    const int64_t n = min((int64_t)N, p.L - s0);
    float2* A = ev_lds;
    float2* Bf = ev_lds + N;
    float* P = reinterpret_cast<float*>(ev_lds + 2 * N);           // [nb] <= N/2 + 1 powers of the reference
    double* red = reinterpret_cast<double*>(P + (N >> 1) + 2);     // (8-byte aligned: N/2 + 2 is even)
    int* flag = reinterpret_cast<int*>(red);                       // (free until the sum over the bins)
    bool any = n > 0;
    if (p.state) {
        const float* __restrict__ w = p.state + (int64_t)b * p.state_ld + s0;
        any = false;
        for (int64_t j = threadIdx.x; j < n; j += STFT_THREADS) any |= w[j] != 0.f;
        if (threadIdx.x == 0) *flag = 0;
        __syncthreads();
        if (any) *flag = 1;                                        // (every writer writes the same value)
        __syncthreads();
        any = *flag != 0;
    }
    if (!any) {                                                    // (uniform over the workgroup)
        if (threadIdx.x == 0) *out = -1.f;
        return;
    }
    const float2* X = pm_frame_fft(ev_row{p.g + (int64_t)b * p.g_ld, p.L}, s0, N, p.window, p.twiddle, A, Bf);
    for (int i = threadIdx.x; i < nb; i += STFT_THREADS) {
        const float2 c = X[a.k_lo + i];
        P[i] = c.x * c.x + c.y * c.y;
    }
    __syncthreads();                                               // (the next frame overwrites A, which may hold X)
    X = pm_frame_fft(ev_row{p.x + (int64_t)b * p.x_ld, p.L}, s0, N, p.window, p.twiddle, A, Bf);
    const double fl = (double)a.floor;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nb; i += STFT_THREADS) {
        const float2 c = X[a.k_lo + i];
        const double d = log10((double)P[i] + fl) - log10((double)(c.x * c.x + c.y * c.y) + fl);
        acc = fma(d, d, acc);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int o = STFT_THREADS / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = (float)sqrt(red[0] / (double)nb);
}

extern "C" int aid_stft_logspec_dist(const aid_stft_mag_observed_params* p, void* stream) {
    AID_REQUIRE(p && p->x && p->g && p->out && p->window && p->twiddle && p->frames, "aid_stft_logspec_dist: null pointer");
    AID_REQUIRE(p->mode == 0, "aid_stft_logspec_dist: mode must be 0 (the distance has no adjoint)");
    AID_REQUIRE(p->n_fft >= 16 && p->n_fft <= 8192 && (p->n_fft & (p->n_fft - 1)) == 0, "aid_stft_logspec_dist: n_fft must be a power of two in [16, 8192]");
    AID_REQUIRE(p->hop > 0 && p->hop <= p->n_fft, "aid_stft_logspec_dist: hop must be in [1, n_fft]");
    AID_REQUIRE(p->B > 0 && p->L > 0 && p->x_ld >= p->L && p->g_ld >= p->L, "aid_stft_logspec_dist: bad shape or row stride");
    AID_REQUIRE(!p->state || p->state_ld == 0 || p->state_ld >= p->L, "aid_stft_logspec_dist: the weights' row stride must be 0 (one shared row) or at least L");
    AID_REQUIRE(p->n_frames == 1 + p->L / p->hop, "aid_stft_logspec_dist: n_frames must be 1 + L / hop");
    AID_REQUIRE(p->out_ld >= p->n_frames, "aid_stft_logspec_dist: the output's row stride is shorter than n_frames");
    AID_REQUIRE((int64_t)p->B * p->n_frames <= 0x7fffffff, "aid_stft_logspec_dist: too many frames");
    ev_dist_args a;
    a.p = *p;
    const float* band = p->frames;                                 // (host memory: see include/aid_phase_long.h)
    const float lo = band[0], hi = band[1];
    AID_REQUIRE(lo >= 0.f && lo <= hi && hi <= (float)(p->n_fft >> 1) && lo == (float)(int)lo && hi == (float)(int)hi,
                "aid_stft_logspec_dist: the band must be whole bins with 0 <= k_lo <= k_hi <= n_fft / 2");
    AID_REQUIRE(band[2] >= 0.f && band[2] <= 3.0e38f, "aid_stft_logspec_dist: floor must be a finite number >= 0");
    a.k_lo = (int)lo; a.k_hi = (int)hi; a.floor = band[2];
    const size_t lds = (size_t)p->n_fft * 2 * sizeof(float2) + ((size_t)(p->n_fft >> 1) + 2) * sizeof(float) + STFT_THREADS * sizeof(double);
    static bool attr = false;
    if (lds > 64 * 1024 && !attr) {                                // (all of the kernel's LDS is dynamic: EV_MAX_LDS is the whole need at n_fft = 8192)
        const hipError_t e = hipFuncSetAttribute((const void*)logspec_dist_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, EV_MAX_LDS);
        if (e != hipSuccess) { aid_set_error(hipGetErrorString(e)); return AID_E_LAUNCH; }
        attr = true;
    }
    hipLaunchKernelGGL(logspec_dist_kernel, dim3(p->B * p->n_frames), dim3(STFT_THREADS), lds, (hipStream_t)stream, a);
    AID_CHECK_LAUNCH();
    return AID_OK;
}

__global__ __launch_bounds__(ES_THREADS) void eval_sums_kernel(const aid_fir_observed_params p) {
    __shared__ double part[ES_SUMS][ES_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    const float* __restrict__ e = p.x + (int64_t)b * p.x_ld;
    const float* __restrict__ r = p.y + (int64_t)b * p.y_ld;
    const float* __restrict__ w = p.state ? p.state + (int64_t)b * p.state_ld : nullptr;
    double n = 0.0, rr = 0.0, ee = 0.0, re = 0.0, dd = 0.0, mx = 0.0;
    for (int64_t i = t; i < p.L; i += ES_THREADS) {
        if (w && !(w[i] != 0.f)) continue;
        const double rv = (double)r[i], ev = (double)e[i], d = rv - ev;
        n += 1.0;
        rr = fma(rv, rv, rr);
        ee = fma(ev, ev, ee);
        re = fma(rv, ev, re);
        dd = fma(d, d, dd);
        mx = fmax(mx, fabs(d));
    }
    const float* __restrict__ h = p.h + (int64_t)b * p.K;
    double nf = 0.0, sf = 0.0;
    for (int i = t; i < p.K; i += ES_THREADS) {
        const float v = h[i];
        if (v >= 0.f) { nf += 1.0; sf += (double)v; }
    }
    part[0][t] = n; part[1][t] = rr; part[2][t] = ee; part[3][t] = re; part[4][t] = dd; part[5][t] = mx; part[6][t] = nf; part[7][t] = sf;
    __syncthreads();
#pragma unroll
    for (int o = ES_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int s = 0; s < ES_SUMS; ++s) part[s][t] = s == 5 ? fmax(part[s][t], part[s][t + o]) : part[s][t] + part[s][t + o];
        }
        __syncthreads();
    }
    if (t < ES_SUMS) ((double*)p.out)[(int64_t)b * ES_SUMS + t] = part[t][0];
}

extern "C" int aid_eval_sums(const aid_fir_observed_params* p, void* stream) {
    AID_REQUIRE(p && p->x && p->y && p->h && p->out, "aid_eval_sums: null pointer");
    AID_REQUIRE(p->mode == 0, "aid_eval_sums: mode must be 0");
    AID_REQUIRE(p->B > 0 && p->L > 0 && p->K > 0, "aid_eval_sums: empty shape (B, L, K >= 1)");
    AID_REQUIRE(p->x_ld >= p->L && p->y_ld >= p->L, "aid_eval_sums: a row stride is shorter than L");
    AID_REQUIRE(!p->state || p->state_ld == 0 || p->state_ld >= p->L, "aid_eval_sums: the weights' row stride must be 0 (one shared row) or at least L");
    AID_REQUIRE(((uintptr_t)p->out & 7) == 0, "aid_eval_sums: the sums are doubles: out must be 8-byte aligned");
    hipLaunchKernelGGL(eval_sums_kernel, dim3(p->B), dim3(ES_THREADS), 0, (hipStream_t)stream, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}
