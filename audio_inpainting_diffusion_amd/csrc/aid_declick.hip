// Declicking (declick.py): the detector that turns a recording into the mask predict_inpainting_long restores.  Declared in
// include/aid_bwe_long.h: aid_ar_score on the parameter block of aid_bwe_gather, aid_click_mask on that of aid_fir_observed.
//
//   ar_score_kernel<BLOCK> : one workgroup of 256 lanes per (recording, block of BLOCK samples).  The block and `order` samples of history go
//                            to LDS as fp32.  Autocorrelation r[0 .. order] in fp64: lane l adds the products i = l, l + 256, ... ascending
//                            (the product of two fp32 numbers is exact in fp64), the 256 partial sums are added as a fixed binary tree, one
//                            lag at a time.  Lane 0 runs Levinson-Durbin on tables in LDS.  Every lane then forms the residuals of its
//                            BLOCK / 256 samples and keeps |e| in registers; a copy, +inf where a sample is not scored, is sorted in LDS
//                            (bitonic, BLOCK doubles) and the median read at rank n' / 2.  score = |e| / sigma leaves as fp32.
//                            Floating-point contraction is off in this file: but for the order of the autocorrelation sums the kernel does
//                            the operations of declick.score_host one for one, so the two differ by what that reordering moves alone.
//                            LDS at BLOCK = 4096: 16512 B of samples, 32768 B of |e|, 2048 B of partial sums, 792 B of tables: 52136 B as laid out,
//                            three workgroups per CU; at the default 2048: 27.5 KB, five.  Latency-bound: 66 sort stages, 17 tree sums.
//   click_mask_kernel      : one workgroup of 256 lanes per tile of 1024 samples.  The samples of the tile and pad + max_run on either side
//                            (clamped to the recording) go to LDS as their bits.  The start of the run a sample lies in is a max-scan over
//                            the positions where a sample differs from the one before, its end a min-scan from the right; a run that
//                            reaches the edge of what was loaded is longer than max_run or holds an end of the recording and is not
//                            flagged.  The flags of the tile and pad on either side are counted by an add-scan: mask = 0 where the count
//                            over [q - pad, q + pad] is not 0.  Integers and compares only.  LDS: 3 x 14336 B + 2 x 6144 B = 55296 B.
//   No atomics, no scratch, nothing kept between launches: a second launch gives the same bits, and a row does not depend on the others.
#include "aid_common.h"
#include "aid_bwe_long.h"

#pragma clang fp contract(off)

#define DC_THREADS 256
#define DC_MAX_ORDER 32
#define DC_TILE 1024
#define DC_MAX_PAD 256
#define DC_MAX_RUN 1024
#define DC_EXT (DC_TILE + 2 * (DC_MAX_PAD + DC_MAX_RUN))           // 3584 samples: the tile and its halo
#define DC_FLAGS (DC_TILE + 2 * DC_MAX_PAD)                        // 1536 flags: the tile and pad on either side

struct dc_score_args {                                             // the kernel's arguments: the caller's block and the checked scalars
    aid_bwe_gather_params p;
    double ridge, sigma_floor;
};

template <int BLOCK>
__global__ __launch_bounds__(DC_THREADS) void ar_score_kernel(const dc_score_args a) {
    constexpr int PER = BLOCK / DC_THREADS;
    __shared__ float xs[BLOCK + DC_MAX_ORDER];                     // xs[i] = rec[base - K + i]: K samples of history, then the block
    __shared__ double srt[BLOCK];
    __shared__ double red[DC_THREADS];
    __shared__ double r[DC_MAX_ORDER + 1], ac[DC_MAX_ORDER + 1], tmp[DC_MAX_ORDER + 1];
    static_assert(sizeof(float) * (BLOCK + DC_MAX_ORDER) + sizeof(double) * (BLOCK + DC_THREADS + 3 * (DC_MAX_ORDER + 1)) <= 64 * 1024, "static LDS");
    const aid_bwe_gather_params& p = a.p;
    const int t = threadIdx.x, K = p.K, j = blockIdx.x, b = blockIdx.y;
    const int64_t base = (int64_t)j * BLOCK;
    const int n = (int)min((int64_t)BLOCK, p.N - base);            // (>= 1: J == ceil(N / BLOCK))
    const float* __restrict__ x = p.rec + (int64_t)b * p.rec_ld;
    float* __restrict__ score = p.y + (int64_t)b * p.out_ld + base;
    float* sigma_out = p.state + (int64_t)b * p.J + j;
    if (n < 8 * K) {                                               // (uniform over the workgroup)
        for (int i = t; i < n; i += DC_THREADS) score[i] = 0.f;
        if (t == 0) *sigma_out = 0.f;
        return;
    }
    for (int i = t; i < n + K; i += DC_THREADS) {
        const int64_t q = base - K + i;
        xs[i] = q >= 0 ? x[q] : 0.f;
    }
    __syncthreads();
    const float* xb = xs + K;                                      // the block's own samples
    for (int m = 0; m <= K; ++m) {
        double acc = 0.0;
        for (int i = t < m ? t + DC_THREADS : t; i < n; i += DC_THREADS) acc = fma((double)xb[i], (double)xb[i - m], acc);
        red[t] = acc;
        __syncthreads();
#pragma unroll
        for (int o = DC_THREADS / 2; o > 0; o >>= 1) {
            if (t < o) red[t] += red[t + o];
            __syncthreads();
        }
        if (t == 0) r[m] = red[0];                                 // (red[0] is lane 0's own: the next lag needs no barrier)
    }
    if (t == 0) {
        r[0] = r[0] * (1.0 + a.ridge);
        ac[0] = 1.0;
        for (int k = 1; k <= K; ++k) ac[k] = 0.0;
        double E = r[0];
        for (int m = 1; m <= K && E > 0.0; ++m) {
            double acc = r[m];
            for (int k = 1; k < m; ++k) acc = acc + ac[k] * r[m - k];
            const double kr = -acc / E;
            for (int k = 1; k < m; ++k) tmp[k] = ac[k] + kr * ac[m - k];
            for (int k = 1; k < m; ++k) ac[k] = tmp[k];
            ac[m] = kr;
            E = E * (1.0 - kr * kr);
        }
    }
    __syncthreads();
    if (!(r[0] > 0.0)) {                                           // (uniform: a silent block)
        for (int i = t; i < n; i += DC_THREADS) score[i] = 0.f;
        if (t == 0) *sigma_out = 0.f;
        return;
    }
    double ev[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int i = t + u * DC_THREADS;
        double e = 0.0;
        if (i < n)
            for (int k = 0; k <= K; ++k) e = e + ac[k] * (double)xb[i - k];
        ev[u] = fabs(e);
        srt[i] = (i < n && base + i >= K) ? ev[u] : (double)INFINITY;
    }
    __syncthreads();
    for (int k = 2; k <= BLOCK; k <<= 1)
        for (int s = k >> 1; s > 0; s >>= 1) {
            for (int h = t; h < BLOCK / 2; h += DC_THREADS) {
                const int i = 2 * h - (h & (s - 1)), l = i + s;    // the pair (i, i ^ s) with bit s of i clear
                const bool up = (i & k) == 0;
                const double u = srt[i], v = srt[l];
                if ((u > v) == up) { srt[i] = v; srt[l] = u; }
            }
            __syncthreads();
        }
    const int scored = n - (base == 0 ? K : 0);                    // (> 0: n >= 8 K)
    const double sigma = fmax(srt[scored >> 1] / 0.6745, a.sigma_floor);
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int i = t + u * DC_THREADS;
        if (i < n) score[i] = base + i >= K ? (float)(ev[u] / sigma) : 0.f;
    }
    if (t == 0) *sigma_out = (float)sigma;
}

extern "C" int aid_ar_score(const aid_bwe_gather_params* p, void* stream) {
    AID_REQUIRE(p && p->rec && p->out && p->y && p->state, "aid_ar_score: null pointer");
    AID_REQUIRE(p->L == 256 || p->L == 512 || p->L == 1024 || p->L == 2048 || p->L == 4096, "aid_ar_score: block must be 256, 512, 1024, 2048 or 4096");
    AID_REQUIRE(p->K >= 1 && p->K <= DC_MAX_ORDER && 8 * (int64_t)p->K <= p->L, "aid_ar_score: order must be in [1, 32] with 8 * order <= block");
    AID_REQUIRE(p->R > 0 && p->R <= 65535 && p->N > 0, "aid_ar_score: bad shape (1 <= R <= 65535, N >= 1)");
    AID_REQUIRE(p->rec_ld >= p->N && p->out_ld >= p->N, "aid_ar_score: a row stride is shorter than N");
    AID_REQUIRE((int64_t)p->J == (p->N + p->L - 1) / p->L, "aid_ar_score: J must be ceil(N / block)");
    dc_score_args a;
    a.p = *p;
    const float* s = p->out;                                       // (host memory: see include/aid_bwe_long.h)
    AID_REQUIRE(s[0] >= 0.f && s[0] <= 3.0e38f, "aid_ar_score: ridge must be a finite number >= 0");
    AID_REQUIRE(s[1] > 0.f && s[1] <= 3.0e38f, "aid_ar_score: sigma_floor must be a finite number > 0");
    a.ridge = (double)s[0]; a.sigma_floor = (double)s[1];
    const dim3 grid(p->J, p->R), block(DC_THREADS);
    switch (p->L) {
        case 256:  hipLaunchKernelGGL(ar_score_kernel<256>, grid, block, 0, (hipStream_t)stream, a); break;
        case 512:  hipLaunchKernelGGL(ar_score_kernel<512>, grid, block, 0, (hipStream_t)stream, a); break;
        case 1024: hipLaunchKernelGGL(ar_score_kernel<1024>, grid, block, 0, (hipStream_t)stream, a); break;
        case 2048: hipLaunchKernelGGL(ar_score_kernel<2048>, grid, block, 0, (hipStream_t)stream, a); break;
        default:   hipLaunchKernelGGL(ar_score_kernel<4096>, grid, block, 0, (hipStream_t)stream, a); break;
    }
    AID_CHECK_LAUNCH();
    return AID_OK;
}

struct dc_mask_args {                                              // the kernel's arguments: the caller's block and the checked settings
    aid_fir_observed_params p;
    float threshold;
    int pad, min_run, max_run;
};

// Inclusive Hillis-Steele scan of a[0 .. n) in LDS (OP 0: max, 1: min, 2: sum) between two buffers; returns the one that holds the result.
// Every lane must have written a[] and passed a barrier before the call; the result may be read right after it.
template <int OP>
__device__ __forceinline__ int* dc_scan(int* a, int* b, int n) {
    for (int off = 1; off < n; off <<= 1) {
        for (int i = threadIdx.x; i < n; i += DC_THREADS) {
            const int u = a[i];
            const int v = i >= off ? a[i - off] : u;
            b[i] = i < off ? u : (OP == 0 ? max(u, v) : OP == 1 ? min(u, v) : u + v);
        }
        __syncthreads();
        int* s = a; a = b; b = s;
    }
    return a;
}

__global__ __launch_bounds__(DC_THREADS) void click_mask_kernel(const dc_mask_args a) {
    __shared__ uint32_t xs[DC_EXT];
    __shared__ int bufA[DC_EXT], bufB[DC_EXT];
    __shared__ int flag[DC_FLAGS], st[DC_FLAGS];
    const aid_fir_observed_params& p = a.p;
    const int t = threadIdx.x, b = blockIdx.y, pad = a.pad;
    const int64_t N = p.L, t0 = (int64_t)blockIdx.x * DC_TILE;
    const float* __restrict__ x = p.x + (int64_t)b * p.x_ld;
    const float* __restrict__ sc = p.y + (int64_t)b * p.y_ld;
    const int FR = DC_TILE + 2 * pad;                              // flag f stands for the sample q = t0 - pad + f
    const int64_t f0 = t0 - pad;
    for (int f = t; f < FR; f += DC_THREADS) {
        const int64_t q = f0 + f;
        flag[f] = (q >= 0 && q < N && sc[q] > a.threshold) ? 1 : 0;
    }
    if (a.min_run > 0) {                                           // (uniform)
        const int halo = pad + a.max_run;
        const int64_t lo = max((int64_t)0, t0 - halo), hi = min(N, t0 + DC_TILE + halo);
        const int E = (int)(hi - lo);                              // <= DC_EXT
        for (int i = t; i < E; i += DC_THREADS) xs[i] = __float_as_uint(x[lo + i]);
        __syncthreads();
        for (int i = t; i < E; i += DC_THREADS) bufA[i] = (i == 0 || xs[i] != xs[i - 1]) ? i : -1;
        __syncthreads();
        const int* S = dc_scan<0>(bufA, bufB, E);                  // S[i]: where the run of sample lo + i starts
        for (int f = t; f < FR; f += DC_THREADS) {
            const int64_t q = f0 + f;
            st[f] = (q >= 0 && q < N) ? S[q - lo] : 0;
        }
        __syncthreads();
        for (int i = t; i < E; i += DC_THREADS) bufA[E - 1 - i] = (i == E - 1 || xs[i] != xs[i + 1]) ? i : DC_EXT;
        __syncthreads();
        const int* Q = dc_scan<1>(bufA, bufB, E);                  // Q[E - 1 - i]: where it ends
        for (int f = t; f < FR; f += DC_THREADS) {
            const int64_t q = f0 + f;
            if (q >= 0 && q < N) {
                const int s = st[f], e = Q[E - 1 - (int)(q - lo)], len = e - s + 1;
                if (s > 0 && e < E - 1 && len >= a.min_run && len <= a.max_run) flag[f] = 1;
            }
        }
    }
    __syncthreads();
    for (int f = t; f < FR; f += DC_THREADS) bufA[f] = flag[f];
    __syncthreads();
    const int* Cn = dc_scan<2>(bufA, bufB, FR);                    // Cn[f]: the flags among 0 .. f
    float* __restrict__ out = p.out + (int64_t)b * p.out_ld + t0;
    for (int u = t; u < DC_TILE && t0 + u < N; u += DC_THREADS)
        out[u] = (Cn[u + 2 * pad] - (u > 0 ? Cn[u - 1] : 0)) > 0 ? 0.f : 1.f;
}

extern "C" int aid_click_mask(const aid_fir_observed_params* p, void* stream) {
    AID_REQUIRE(p && p->x && p->y && p->h && p->out, "aid_click_mask: null pointer");
    AID_REQUIRE(p->mode == 0, "aid_click_mask: mode must be 0");
    AID_REQUIRE(p->B > 0 && p->B <= 65535 && p->L > 0, "aid_click_mask: bad shape (1 <= B <= 65535, L >= 1)");
    AID_REQUIRE(p->x_ld >= p->L && p->y_ld >= p->L && p->out_ld >= p->L, "aid_click_mask: a row stride is shorter than L");
    AID_REQUIRE((p->L + DC_TILE - 1) / DC_TILE <= 0x7fffffff, "aid_click_mask: too many tiles");
    const float* s = p->h;                                         // (host memory: see include/aid_bwe_long.h)
    AID_REQUIRE(s[0] > 0.f && s[0] <= 3.0e38f, "aid_click_mask: threshold must be a finite number > 0");
    AID_REQUIRE(s[1] >= 0.f && s[1] <= (float)DC_MAX_PAD && s[1] == (float)(int)s[1], "aid_click_mask: pad must be a whole number in [0, 256]");
    AID_REQUIRE(s[3] >= 1.f && s[3] <= (float)DC_MAX_RUN && s[3] == (float)(int)s[3], "aid_click_mask: max_run must be a whole number in [1, 1024]");
    AID_REQUIRE(s[2] == 0.f || (s[2] >= 2.f && s[2] <= s[3] && s[2] == (float)(int)s[2]),
                "aid_click_mask: min_run must be 0 (no run rule) or a whole number in [2, max_run]");
    dc_mask_args a;
    a.p = *p;
    a.threshold = s[0]; a.pad = (int)s[1]; a.min_run = (int)s[2]; a.max_run = (int)s[3];
    hipLaunchKernelGGL(click_mask_kernel, dim3((unsigned)((p->L + DC_TILE - 1) / DC_TILE), p->B), dim3(DC_THREADS), 0, (hipStream_t)stream, a);
    AID_CHECK_LAUNCH();
    return AID_OK;
}
