// The stride-1 FIR tile loop shared by aid_fir (aid_degrade.hip), aid_fir_observed (aid_bwe_long.hip) and aid_fir_clip_observed
// (aid_bwe_declip_long.hip).
//
//   One workgroup of FIR_THREADS lanes computes FIR_TO = 2048 consecutive outputs of one row.  Taps and the input tile plus its halo are
//   staged in LDS in chunks of FIR_KC = 1024 taps; each lane owns FIR_R = 8 consecutive outputs and walks the taps in blocks of 8 with a
//   16-float register window (float4 LDS reads, 64 FMAs per 24 floats read).  The 8-tap partial sums are fp32, the running sums fp64, so
//   long filters (K = 4096) stay at fp32 rounding.  What a staged sample IS is the caller's business: ``load(q)`` returns input sample q of
//   the row for ANY q (it bounds the access itself and returns 0 outside the row), so a kernel may select on the way into LDS at no cost
//   in LDS or registers.  The arithmetic and its order are fixed here: two kernels that stage the same values get the same bits.
#pragma once
#include "aid_common.h"

#define FIR_THREADS 256
#define FIR_R 8                          // outputs per lane
#define FIR_TO (FIR_THREADS * FIR_R)     // outputs per workgroup
#define FIR_KC 1024                      // taps per LDS chunk

// accd[r] = sum_k hk[k] * load(tile0 + t * FIR_R + r + k - pad),  hk[k] = rev ? h[K-1-k] : h[k],  t = threadIdx.x.
// Every lane of the workgroup must call it (it synchronises); blockDim.x == FIR_THREADS.
template <class LOAD>
__device__ __forceinline__ void fir_tile(LOAD load, int64_t tile0, const float* __restrict__ h, int K, int pad, int rev, double (&accd)[FIR_R]) {
    __shared__ __attribute__((aligned(16))) float hs[FIR_KC];
    __shared__ __attribute__((aligned(16))) float xs[FIR_TO + FIR_KC];
    const int t = threadIdx.x;
#pragma unroll
    for (int r = 0; r < FIR_R; ++r) accd[r] = 0.0;
    for (int kc0 = 0; kc0 < K; kc0 += FIR_KC) {
        const int kn = min(FIR_KC, K - kc0);
        const int knp = (kn + FIR_R - 1) / FIR_R * FIR_R;
        for (int k = t; k < knp; k += FIR_THREADS) {
            const int kg = kc0 + k;
            hs[k] = k < kn ? h[rev ? K - 1 - kg : kg] : 0.f;
        }
        const int64_t q0 = tile0 + kc0 - pad;
        for (int m = t; m < FIR_TO + knp; m += FIR_THREADS) xs[m] = load(q0 + m);
        __syncthreads();
        for (int kk = 0; kk < knp; kk += FIR_R) {
            float xw[2 * FIR_R], hv[FIR_R];
            const float4* xp = reinterpret_cast<const float4*>(xs + t * FIR_R + kk);
            const float4* hp = reinterpret_cast<const float4*>(hs + kk);
#pragma unroll
            for (int v = 0; v < FIR_R / 2; ++v) {
                const float4 a = xp[v];
                xw[4 * v] = a.x; xw[4 * v + 1] = a.y; xw[4 * v + 2] = a.z; xw[4 * v + 3] = a.w;
            }
#pragma unroll
            for (int v = 0; v < FIR_R / 4; ++v) {
                const float4 a = hp[v];
                hv[4 * v] = a.x; hv[4 * v + 1] = a.y; hv[4 * v + 2] = a.z; hv[4 * v + 3] = a.w;
            }
            float acc[FIR_R];
#pragma unroll
            for (int r = 0; r < FIR_R; ++r) acc[r] = 0.f;
#pragma unroll
            for (int j = 0; j < FIR_R; ++j)
#pragma unroll
                for (int r = 0; r < FIR_R; ++r) acc[r] = fmaf(hv[j], xw[r + j], acc[r]);
#pragma unroll
            for (int r = 0; r < FIR_R; ++r) accd[r] += (double)acc[r];
        }
        __syncthreads();
    }
}
