// The frame and overlap-add bodies of the STFT-domain masking operator, shared by aid_stft_frames / aid_stft_ola (aid_stft.hip) and
// aid_stft_mask_observed (aid_spec_long.hip).
//
//   One workgroup of STFT_THREADS lanes owns one frame; A and Bf are two N-point float2 buffers in LDS (aid_fft_lds.h).  What entry j of
//   the frame IS is the caller's business: ``load(j)`` returns it for j in [0, N) -- border handling, selects and the 1/envelope
//   pre-scale of the adjoint included -- and bounds the access itself; ``use(t)`` tells the overlap-add whether frame t of the scratch was
//   written.  The arithmetic and its order are fixed here: two kernels that load the same values and use the same frames get the same
//   bits.
#pragma once
#include "aid_common.h"
#include "aid_fft_lds.h"

// fr[j] = window[j] / N * Re(IFFT(m .* FFT(window .* load)))[j]; m is the mask column (bin stride mask_ld), mirrored above N/2.
// Every lane of the workgroup must call it (it synchronises).
template <class LOAD>
__device__ __forceinline__ void st_mask_frame(LOAD load, int N, const float* __restrict__ window, const float* __restrict__ twiddle,
                                              const float* __restrict__ m, int64_t mask_ld, float2* A, float2* Bf, float* __restrict__ fr) {
    const int half = N >> 1;
    for (int j = threadIdx.x; j < N; j += STFT_THREADS) {
        const float v = load(j);
        A[j] = make_float2(v * window[j], 0.f);
    }
    __syncthreads();
    const float2* tw = reinterpret_cast<const float2*>(twiddle);
    float2* R = st_fft(A, Bf, N, tw, -1.f);
    for (int f = threadIdx.x; f < N; f += STFT_THREADS) {
        const int fm = f <= half ? f : N - f;
        const float mv = m[(int64_t)fm * mask_ld];
        R[f].x *= mv;
        R[f].y *= mv;
    }
    __syncthreads();
    float2* S = st_fft(R, R == A ? Bf : A, N, tw, +1.f);
    const float inv = 1.0f / (float)N;
    for (int j = threadIdx.x; j < N; j += STFT_THREADS) fr[j] = S[j].x * window[j] * inv;
}

// sum of the frames covering centred position q = pos + N/2 (pos >= -N/2), ascending, over the frames [0, n_frames) of the signal; the
// scratch fr holds frames [t0, t0 + n_held) of them, and a frame outside it or with !use(t - t0) is skipped and its scratch is not read
template <class USE>
__device__ __forceinline__ float st_cover(USE use, const float* __restrict__ fr, int64_t pos, int N, int hop, int64_t n_frames,
                                          int64_t t0, int64_t n_held) {
    const int64_t q = pos + (N >> 1);
    int64_t n1 = q / hop;
    int64_t n0 = (q - (N - 1) + hop - 1) / hop;
    if (q - (N - 1) < 0) n0 = 0;
    if (n1 > n_frames - 1) n1 = n_frames - 1;
    if (n0 < t0) n0 = t0;
    if (n1 > t0 + n_held - 1) n1 = t0 + n_held - 1;
    float acc = 0.f;
    for (int64_t n = n0; n <= n1; ++n)
        if (use(n - t0)) acc += fr[(n - t0) * N + (q - n * hop)];
    return acc;
}

struct st_all {                                                    // every frame of the scratch was written
    __device__ __forceinline__ bool operator()(int64_t) const { return true; }
};
