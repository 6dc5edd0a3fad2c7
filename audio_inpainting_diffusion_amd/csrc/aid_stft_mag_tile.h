// The frame and overlap-add bodies of the STFT magnitude and its VJP, shared by aid_stft_mag (aid_phase.hip) and
// aid_stft_mag_observed (aid_phase_long.hip).
//
//   One workgroup of STFT_THREADS lanes owns one frame; A and Bf are two N-point float2 buffers in LDS (aid_fft_lds.h).  What a sample
//   IS is the caller's business: ``load(q)`` returns sample q of the row for ANY q >= 0 (it bounds the access itself and returns 0 at and
//   past the end of the row), so a kernel may select on the way into LDS; ``use(t)`` tells the overlap-add whether frame t of the scratch
//   was written.  The arithmetic and its order are fixed here: two kernels that load the same values and use the same frames get the
//   same bits.
#pragma once
#include "aid_common.h"
#include "aid_fft_lds.h"

// the frame that starts at sample s0, times the window, forward FFT; returns the LDS buffer that holds X.  Every lane of the workgroup
// must call it (it synchronises).
template <class LOAD>
__device__ __forceinline__ float2* pm_frame_fft(LOAD load, int64_t s0, int N, const float* __restrict__ window, const float* __restrict__ twiddle,
                                                float2* A, float2* Bf) {
    for (int j = threadIdx.x; j < N; j += STFT_THREADS) {
        const float v = load(s0 + j);
        A[j] = make_float2(v * window[j], 0.f);
    }
    __syncthreads();
    return st_fft(A, Bf, N, reinterpret_cast<const float2*>(twiddle), -1.f);
}

// out[k * ld] = |X_k|, k <= N/2
template <class LOAD>
__device__ __forceinline__ void pm_mag_frame(LOAD load, int64_t s0, int N, const float* __restrict__ window, const float* __restrict__ twiddle,
                                             float2* lds, float* __restrict__ out, int64_t ld) {
    const int F = (N >> 1) + 1;
    const float2* X = pm_frame_fft(load, s0, N, window, twiddle, lds, lds + N);
    for (int k = threadIdx.x; k < F; k += STFT_THREADS) {
        const float2 c = X[k];
        out[(int64_t)k * ld] = sqrtf(c.x * c.x + c.y * c.y);
    }
}

// fr[j] = window[j] * Re(IFFT_N(Z))[j], Z_k = g[k * ld] X_k / |X_k| for k <= N/2 (0 where |X_k| = 0), 0 above (the output is one-sided:
// no Hermitian mirror); X is recomputed from the samples
template <class LOAD>
__device__ __forceinline__ void pm_vjp_frame(LOAD load, int64_t s0, int N, const float* __restrict__ window, const float* __restrict__ twiddle,
                                             float2* lds, const float* __restrict__ g, int64_t ld, float* __restrict__ fr) {
    const int half = N >> 1;
    float2* A = lds;
    float2* Bf = lds + N;
    float2* X = pm_frame_fft(load, s0, N, window, twiddle, A, Bf);
    for (int k = threadIdx.x; k < N; k += STFT_THREADS) {      // in place: lane-private k
        float2 z = make_float2(0.f, 0.f);
        if (k <= half) {
            const float2 c = X[k];
            const float m = sqrtf(c.x * c.x + c.y * c.y);
            if (m > 0.f) {
                const float s = g[(int64_t)k * ld] / m;
                z = make_float2(c.x * s, c.y * s);
            }
        }
        X[k] = z;
    }
    __syncthreads();
    const float2* S = st_fft(X, X == A ? Bf : A, N, reinterpret_cast<const float2*>(twiddle), +1.f);
    for (int j = threadIdx.x; j < N; j += STFT_THREADS) fr[j] = S[j].x * window[j];
}

// sample q < L of the overlap-add over the frame scratch fr [T, N] of one item: the frames that cover q, ascending (q / hop < T because
// T = 1 + L / hop); a frame with !use(t) is skipped and its scratch is not read
template <class USE>
__device__ __forceinline__ float pm_ola(USE use, const float* __restrict__ fr, int64_t q, int N, int hop) {
    const int64_t t1 = q / hop;
    const int64_t t0 = q < N ? 0 : (q - (N - 1) + hop - 1) / hop;
    float acc = 0.f;
    for (int64_t t = t0; t <= t1; ++t)
        if (use(t)) acc += fr[t * N + (q - t * hop)];
    return acc;
}
