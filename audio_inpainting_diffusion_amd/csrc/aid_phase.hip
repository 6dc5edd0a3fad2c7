// Phase retrieval (include/aid_phase.h): the STFT-magnitude operator with its VJP, and the guidance seed of the induced
// matrix norms over [B, F, T] observations.
//
//   stft_mag_kernel          : one workgroup per (item, frame): gather x (zero at and past L) times window -> LDS radix-2
//                              Stockham FFT (aid_fft_lds.h) -> |X_k|, k <= N/2, written to out[b, k, t] (frames contiguous).
//   stft_mag_vjp_frames_kernel: the same gather and FFT (X is recomputed from the stored x_hat rather than kept from the
//                              forward: one more FFT per frame instead of a [B, T, F] complex buffer), Z_k = g_k X_k / |X_k|
//                              for k <= N/2 and 0 above (the output is one-sided: no Hermitian mirror), unnormalised inverse
//                              FFT, real part times window -> frame buffer [B, T, N].
//   stft_mag_ola_kernel      : one lane per sample q < L gathers the frames covering it (no atomics -> deterministic).
//   The bodies of the three are device functions in aid_stft_mag_tile.h, which aid_phase_long.hip instantiates with selects.
//   Bins with |X_k| = 0 contribute 0.  The reference's autograd (sqrt of re^2 + im^2) gives 0 * inf = NaN there; in
//   practice that only happens in the all-zero last frame when hop divides L, which covers the appended zeros only, so its
//   NaN lands on the padding that torch.cat's backward drops and the reference's gradient w.r.t. x stays finite -- as here.
//
//   mnorm1_kernel / mnorm2_kernel: one 1024-lane workgroup per item, fp64 accumulation, see aid_phase.h.
#include "aid_common.h"
#include "aid_stft_mag_tile.h"
#include "aid_phase.h"

#define MN_THREADS 1024
#define MN_WAVES (MN_THREADS / AID_WAVE)
#define MN_MAX_LDS 65536

extern "C" int aid_phase_abi_version(void) { return AID_PHASE_ABI_VERSION; }

// ---- STFT magnitude ------------------------------------------------------------------------------------------------
// (the frame and overlap-add bodies live in aid_stft_mag_tile.h, shared with aid_stft_mag_observed; here without selects)
struct pm_row {                                                    // sample q of the row, 0 at and past L
    const float* __restrict__ x; int64_t L;
    __device__ __forceinline__ float operator()(int64_t q) const { return q < L ? x[q] : 0.f; }
};
struct pm_all {
    __device__ __forceinline__ bool operator()(int64_t) const { return true; }
};

__global__ __launch_bounds__(STFT_THREADS) void stft_mag_kernel(const aid_stft_mag_params p) {
    const int b = blockIdx.x / p.n_frames, t = blockIdx.x - b * p.n_frames;
    extern __shared__ __attribute__((aligned(16))) float2 pm_lds[];
    const int F = (p.n_fft >> 1) + 1;
    pm_mag_frame(pm_row{p.x + (int64_t)b * p.x_ld, p.L}, (int64_t)t * p.hop, p.n_fft, p.window, p.twiddle, pm_lds,
                 p.out + (int64_t)b * F * p.n_frames + t, p.n_frames);
}

__global__ __launch_bounds__(STFT_THREADS) void stft_mag_vjp_frames_kernel(const aid_stft_mag_params p) {
    const int b = blockIdx.x / p.n_frames, t = blockIdx.x - b * p.n_frames;
    extern __shared__ __attribute__((aligned(16))) float2 pm_lds[];
    const int N = p.n_fft, F = (N >> 1) + 1;
    pm_vjp_frame(pm_row{p.x + (int64_t)b * p.x_ld, p.L}, (int64_t)t * p.hop, N, p.window, p.twiddle, pm_lds,
                 p.g + (int64_t)b * F * p.n_frames + t, p.n_frames, p.frames + ((int64_t)b * p.n_frames + t) * N);
}

__global__ __launch_bounds__(256) void stft_mag_ola_kernel(const aid_stft_mag_params p) {
    const int b = blockIdx.y, N = p.n_fft;
    const float* fr = p.frames + (int64_t)b * p.n_frames * N;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < p.L; q += (int64_t)gridDim.x * 256)
        p.out[(int64_t)b * p.out_ld + q] = pm_ola(pm_all{}, fr, q, N, p.hop);
}

extern "C" int aid_stft_mag(const aid_stft_mag_params* p, void* stream) {
    AID_REQUIRE(p && p->x && p->out && p->window && p->twiddle, "aid_stft_mag: null pointer");
    AID_REQUIRE(!p->adjoint || (p->g && p->frames), "aid_stft_mag: the adjoint needs g and the frame scratch");
    AID_REQUIRE(p->n_fft >= 16 && p->n_fft <= 8192 && (p->n_fft & (p->n_fft - 1)) == 0, "aid_stft_mag: n_fft must be a power of two in [16, 8192]");
    AID_REQUIRE(p->hop > 0 && p->hop <= p->n_fft, "aid_stft_mag: hop must be in [1, n_fft]");
    AID_REQUIRE(p->B > 0 && p->L > 0 && p->x_ld >= p->L, "aid_stft_mag: bad shape or row stride");
    AID_REQUIRE(p->n_frames == 1 + p->L / p->hop, "aid_stft_mag: n_frames must be 1 + L / hop");
    AID_REQUIRE((int64_t)p->B * p->n_frames <= 0x7fffffff, "aid_stft_mag: too many frames");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)p->n_fft * 2 * sizeof(float2);
    if (!p->adjoint) {
        hipLaunchKernelGGL(stft_mag_kernel, dim3(p->B * p->n_frames), dim3(STFT_THREADS), lds, st, *p);
        AID_CHECK_LAUNCH();
        return AID_OK;
    }
    AID_REQUIRE(p->B <= 65535 && p->out_ld >= p->L, "aid_stft_mag: bad output shape or row stride");
    hipLaunchKernelGGL(stft_mag_vjp_frames_kernel, dim3(p->B * p->n_frames), dim3(STFT_THREADS), lds, st, *p);
    AID_CHECK_LAUNCH();
    int gx = aid_cdiv(p->L, 256); if (gx > 2048) gx = 2048;
    hipLaunchKernelGGL(stft_mag_ola_kernel, dim3(gx, p->B), dim3(256), 0, st, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}

// ---- induced matrix norms ------------------------------------------------------------------------------------------
__device__ __forceinline__ double mn_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// every lane gets the sum (or the max); red holds MN_WAVES doubles
__device__ double mn_block_reduce(double v, double* red, bool is_max) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o, 64);
        v = is_max ? fmax(v, w) : v + w;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = red[0];
    for (int i = 1; i < MN_WAVES; ++i) r = is_max ? fmax(r, red[i]) : r + red[i];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(MN_THREADS) void mnorm1_kernel(const aid_matrix_norm_params p) {
    extern __shared__ double mn_lds[];
    const int b = blockIdx.x, F = p.F, T = p.T;
    double* cs = mn_lds;                                     // [T] column sums of |R|
    double* red = mn_lds + T;
    const int64_t base = (int64_t)b * F * T;
    const float* y = p.y + base;
    const float* den = p.den + base;
    double m = -1.0;
    for (int t = threadIdx.x; t < T; t += MN_THREADS) {
        double s = 0.0;
        for (int f = 0; f < F; ++f) s += fabs((double)(y[(int64_t)f * T + t] - den[(int64_t)f * T + t]));
        cs[t] = s;
        m = fmax(m, s);
    }
    m = mn_block_reduce(m, red, true);                       // (also orders the cs writes before the reads below)
    double c = 0.0;
    for (int t = threadIdx.x; t < T; t += MN_THREADS) c += cs[t] == m ? 1.0 : 0.0;
    c = mn_block_reduce(c, red, false);
    if (threadIdx.x == 0) {
        p.norm[b] = (float)m;
        if (p.diag) { p.diag[2 * b] = 0.f; p.diag[2 * b + 1] = 0.f; }
    }
    const float w = (float)(1.0 / c);
    float* g = p.g + base;
    for (int64_t i = threadIdx.x; i < (int64_t)F * T; i += MN_THREADS) {
        const int t = (int)(i % T);
        float v = 0.f;
        if (cs[t] == m) {
            const float r = y[i] - den[i];
            v = r > 0.f ? -w : (r < 0.f ? w : 0.f);           // -d|r|/dr / ties
        }
        g[i] = v;
    }
}

__global__ __launch_bounds__(MN_THREADS) void mnorm2_kernel(const aid_matrix_norm_params p) {
    extern __shared__ double mn_lds[];
    const int b = blockIdx.x, F = p.F, T = p.T;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* v = mn_lds;                                      // [T]
    double* u = mn_lds + T;                                  // [F]
    double* red = u + F;
    const int64_t base = (int64_t)b * F * T;
    const float* y = p.y + base;
    const float* den = p.den + base;
    float* R = p.r + base;
    // R = y - den (fp32, as the reference forms it); v0[t] = ||R[:, t]|| * (1 + t/T)  (data-derived start; the ramp keeps it
    // off the degenerate R v0 = 0 of two opposite columns)
    double acc = 0.0;
    for (int t = threadIdx.x; t < T; t += MN_THREADS) {
        double s = 0.0;
        for (int f = 0; f < F; ++f) {
            const int64_t o = (int64_t)f * T + t;
            const float r = y[o] - den[o];
            R[o] = r;
            s += (double)r * (double)r;
        }
        const double v0 = sqrt(s) * (1.0 + (double)t / T);
        v[t] = v0;
        acc += v0 * v0;
    }
    const double nv = mn_block_reduce(acc, red, false);
    int it = 0;
    double sigma = 0.0, res = 0.0;
    if (nv > 0.0) {
        double inv = 1.0 / sqrt(nv);
        for (int t = threadIdx.x; t < T; t += MN_THREADS) v[t] *= inv;
        __syncthreads();
        for (;;) {
            // u = R v  (one wave per row)
            for (int f = wave; f < F; f += MN_WAVES) {
                const float* Rf = R + (int64_t)f * T;
                double d = 0.0;
                for (int t = lane; t < T; t += AID_WAVE) d = fma((double)Rf[t], v[t], d);
                d = mn_wave_sum(d);
                if (lane == 0) u[f] = d;
            }
            __syncthreads();
            acc = 0.0;
            for (int f = threadIdx.x; f < F; f += MN_THREADS) acc += u[f] * u[f];
            const double s = sqrt(mn_block_reduce(acc, red, false));      // ||R v||
            if (!(s > 0.0)) { sigma = 0.0; res = 0.0; ++it; break; }
            inv = 1.0 / s;
            for (int f = threadIdx.x; f < F; f += MN_THREADS) u[f] *= inv;
            __syncthreads();
            // w = R^T u (one lane per column); residual ||w - s v|| / s; v <- w / ||w||
            double rr = 0.0, ww = 0.0;
            for (int t = threadIdx.x; t < T; t += MN_THREADS) {
                double w = 0.0;
#pragma unroll 8
                for (int f = 0; f < F; ++f) w = fma((double)R[(int64_t)f * T + t], u[f], w);
                const double e = w - s * v[t];
                rr += e * e;
                ww += w * w;
                v[t] = w;
            }
            rr = mn_block_reduce(rr, red, false);
            ww = mn_block_reduce(ww, red, false);
            ++it;
            res = sqrt(rr) / s;
            sigma = sqrt(ww);                                 // ||R^T u|| >= u^T R v = s: the better estimate of sigma_1
            inv = 1.0 / sigma;
            for (int t = threadIdx.x; t < T; t += MN_THREADS) v[t] *= inv;
            __syncthreads();
            if (res <= p.tol || it >= p.max_iter) break;
        }
    }
    if (threadIdx.x == 0) {
        p.norm[b] = (float)sigma;
        if (p.diag) { p.diag[2 * b] = (float)it; p.diag[2 * b + 1] = (float)res; }
    }
    float* g = p.g + base;
    const bool zero = !(sigma > 0.0);
    for (int64_t i = threadIdx.x; i < (int64_t)F * T; i += MN_THREADS) {
        const int f = (int)(i / T), t = (int)(i - (int64_t)f * T);
        g[i] = zero ? 0.f : (float)(-u[f] * v[t]);
    }
}

extern "C" int aid_matrix_norm_seed(const aid_matrix_norm_params* p, void* stream) {
    AID_REQUIRE(p && p->den && p->y && p->g && p->norm, "aid_matrix_norm_seed: null pointer");
    AID_REQUIRE(p->B > 0 && p->F > 0 && p->T > 0, "aid_matrix_norm_seed: empty shape");
    AID_REQUIRE(p->ord == 1 || p->ord == 2, "aid_matrix_norm_seed: ord is 1 or 2");
    const size_t lds = ((size_t)(p->ord == 2 ? p->F + p->T : p->T) + 32) * sizeof(double);
    AID_REQUIRE(lds <= MN_MAX_LDS, "aid_matrix_norm_seed: F + T must be at most 8160");
    hipStream_t st = (hipStream_t)stream;
    if (p->ord == 1) {
        hipLaunchKernelGGL(mnorm1_kernel, dim3(p->B), dim3(MN_THREADS), lds, st, *p);
    } else {
        AID_REQUIRE(p->r, "aid_matrix_norm_seed: ord 2 needs the residual scratch r");
        AID_REQUIRE(p->max_iter >= 1 && p->tol >= 0.0, "aid_matrix_norm_seed: max_iter >= 1 and tol >= 0");
        hipLaunchKernelGGL(mnorm2_kernel, dim3(p->B), dim3(MN_THREADS), lds, st, *p);
    }
    AID_CHECK_LAUNCH();
    return AID_OK;
}
