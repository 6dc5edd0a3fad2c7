// Radix-2 Stockham FFT of one frame in LDS, shared by the STFT kernels (aid_stft.hip: spectrogram masking, aid_phase.hip:
// STFT magnitude).  The workgroup is STFT_THREADS lanes; a, b are two N-point float2 buffers in LDS.
#pragma once
#include <hip/hip_runtime.h>

#define STFT_THREADS 256

__device__ __forceinline__ float2 st_cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// radix-2 Stockham in LDS; tw = exp(-2 pi i m / N), m < N/2.  sign -1 forward, +1 inverse (unnormalised).
__device__ float2* st_fft(float2* a, float2* b, int N, const float2* __restrict__ tw, float sign) {
    for (int Ns = 1; Ns < N; Ns <<= 1) {
        const int tstride = N / (2 * Ns);
        for (int j = threadIdx.x; j < (N >> 1); j += STFT_THREADS) {
            const int k = j & (Ns - 1);
            float2 w = tw[k * tstride];
            w.y *= -sign;
            const float2 u = a[j];
            const float2 v = st_cmul(a[j + (N >> 1)], w);
            const int j0 = ((j - k) << 1) + k;
            b[j0] = make_float2(u.x + v.x, u.y + v.y);
            b[j0 + Ns] = make_float2(u.x - v.x, u.y - v.y);
        }
        __syncthreads();
        float2* t = a; a = b; b = t;
    }
    return a;
}
