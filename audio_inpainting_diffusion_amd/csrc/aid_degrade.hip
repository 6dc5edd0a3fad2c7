// Restoration degradations (include/aid_degrade.h): FIR / IIR filtering, decimation, hard clipping and their adjoints.
//
//   fir (stride 1, both directions): one workgroup per (row, tile of 2048 outputs); taps and the input tile plus its halo
//        are staged in LDS in chunks of 1024 taps; each lane owns 8 consecutive outputs and walks the taps in blocks of
//        8 with a 16-float register window (float4 LDS reads, 64 FMAs per 24 floats read).  The 8-tap partial sums are
//        fp32, the running sums fp64, so long filters (K = 4096) stay at fp32 rounding.  The adjoint of a stride-1
//        correlation is the correlation with reversed taps and pad K-1-pad, so it runs the same kernel.  The tile loop is
//        fir_tile of aid_fir_tile.h, which aid_fir_observed (aid_bwe_long.hip) instantiates too.
//   fir (stride > 1): one lane per output gathers straight from global memory (decimation, short strided low-passes).
//   iir: three launches (chunk zero-state recursion, carry scan of the N-sample state, correction), see aid_degrade.h.
//   clip: element-wise.
#include "aid_common.h"
#include "aid_degrade.h"
#include "aid_fir_tile.h"

#define DG_THREADS 256
#define FIR_MAX_STRIDE 16
#define FIR_MAX_K_STRIDED 4096
#define IIR_MAX_N 16

__device__ __forceinline__ int64_t dg_floordiv(int64_t a, int64_t b) {   // b > 0
    int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

__device__ __forceinline__ float dg_epilogue(float a, float c0, const float* add1, const float* add2, int64_t idx) {
    float v = c0 * a;
    if (add1) v += add1[idx];
    if (add2) v += add2[idx];
    return v;
}

// out[b, i] = c0 * sum_k hk[k] * in[b, i + k - pad] + add1 + add2,  hk[k] = rev ? h[K-1-k] : h[k]
__global__ __launch_bounds__(FIR_THREADS) void fir_unit_kernel(const float* __restrict__ in, int64_t in_ld, int64_t Lin,
                                                               float* __restrict__ out, int64_t out_ld, int64_t Lout,
                                                               const float* __restrict__ h, int K, int pad, int rev,
                                                               const float* add1, const float* add2, float c0) {
    const int b = blockIdx.y, t = threadIdx.x;
    const int64_t tile0 = (int64_t)blockIdx.x * FIR_TO;
    const float* x = in + (int64_t)b * in_ld;
    double accd[FIR_R];
    fir_tile([&](int64_t q) { return (q >= 0 && q < Lin) ? x[q] : 0.f; }, tile0, h, K, pad, rev, accd);
#pragma unroll
    for (int r = 0; r < FIR_R; ++r) {
        const int64_t i = tile0 + t * FIR_R + r;
        if (i < Lout) {
            const int64_t o = (int64_t)b * out_ld + i;
            out[o] = dg_epilogue((float)accd[r], c0, add1, add2, o);
        }
    }
}

// stride > 1, one lane per output.  forward: out[i] = sum_k h[k] x[i*s + k - pad];  adjoint: out[j] = sum_i h[j + pad - i*s] g[i]
__global__ __launch_bounds__(DG_THREADS) void fir_strided_kernel(const aid_fir_params p) {
    const int b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * DG_THREADS + threadIdx.x;
    const int64_t Lout = p.adjoint ? p.L : p.L_out;
    if (i >= Lout) return;
    const float* x = p.x + (int64_t)b * p.x_ld;
    const int s = p.stride;
    double acc = 0.0;
    if (!p.adjoint) {
        const int64_t q0 = i * s - p.pad_left;
        const int k0 = (int)max((int64_t)0, -q0);
        const int k1 = (int)min((int64_t)p.K, p.L - q0);
        for (int k = k0; k < k1; ++k) acc = fma((double)p.h[k], (double)x[q0 + k], acc);
    } else {
        const int64_t num = i + p.pad_left;
        const int64_t ilo = max((int64_t)0, dg_floordiv(num - p.K + 1 + s - 1, s));
        const int64_t ihi = min(p.L_out - 1, dg_floordiv(num, s));
        for (int64_t q = ilo; q <= ihi; ++q) acc = fma((double)p.h[num - q * s], (double)x[q], acc);
    }
    const int64_t o = (int64_t)b * p.out_ld + i;
    p.out[o] = dg_epilogue((float)acc, p.c0, p.add1, p.add2, o);
}

extern "C" int aid_degrade_abi_version(void) { return AID_DEGRADE_ABI_VERSION; }

extern "C" int aid_fir(const aid_fir_params* p, void* stream) {
    AID_REQUIRE(p && p->x && p->out && p->h, "aid_fir: null pointer");
    AID_REQUIRE(p->B > 0 && p->B <= 65535 && p->K > 0 && p->L > 0 && p->L_out > 0, "aid_fir: empty or oversized shape");
    AID_REQUIRE(p->stride >= 1 && p->stride <= FIR_MAX_STRIDE, "aid_fir: stride must be in [1, 16]");
    AID_REQUIRE(p->pad_left >= 0, "aid_fir: negative padding");
    const int64_t Lin = p->adjoint ? p->L_out : p->L, Lout = p->adjoint ? p->L : p->L_out;
    AID_REQUIRE(p->x_ld >= Lin && p->out_ld >= Lout, "aid_fir: row stride shorter than the row");
    hipStream_t st = (hipStream_t)stream;
    if (p->stride == 1) {
        const int pad = p->adjoint ? p->K - 1 - p->pad_left : p->pad_left;   // (may be negative: a plain shift)
        hipLaunchKernelGGL(fir_unit_kernel, dim3(aid_cdiv(Lout, FIR_TO), p->B), dim3(FIR_THREADS), 0, st,
                           p->x, p->x_ld, Lin, p->out, p->out_ld, Lout, p->h, p->K, pad, p->adjoint, p->add1, p->add2, p->c0);
    } else {
        AID_REQUIRE(p->K <= FIR_MAX_K_STRIDED, "aid_fir: strided filters take at most 4096 taps");
        hipLaunchKernelGGL(fir_strided_kernel, dim3(aid_cdiv(Lout, DG_THREADS), p->B), dim3(DG_THREADS), 0, st, *p);
    }
    AID_CHECK_LAUNCH();
    return AID_OK;
}

// ---- IIR ------------------------------------------------------------------------------------------------------------
// input sample q of the recursion (processing order): adjoint reads reversed and masked by the forward's clamp
__device__ __forceinline__ double iir_in(const aid_iir_params& p, const float* x, const float* pre, int64_t q) {
    if (q < 0) return 0.0;
    const int64_t ph = p.adjoint ? p.L - 1 - q : q;
    float v = x[ph];
    if (pre) {
        const float u = pre[ph];
        v = (u >= -1.f && u <= 1.f) ? v : 0.f;
    }
    return (double)v;
}

template <int NT>
__global__ __launch_bounds__(DG_THREADS) void iir_chunk_kernel(const aid_iir_params p, int64_t n_chunks) {
    const int64_t gid = (int64_t)blockIdx.x * DG_THREADS + threadIdx.x;
    if (gid >= (int64_t)p.B * n_chunks) return;
    const int b = (int)(gid / n_chunks);
    const int64_t c = gid - (int64_t)b * n_chunks;
    const float* x = p.x + (int64_t)b * p.x_ld;
    const float* pre = (p.adjoint && p.clamp) ? p.pre + (int64_t)b * p.L : nullptr;
    double bc[NT + 1], ac[NT + 1], xh[NT + 1], zh[NT];
#pragma unroll
    for (int k = 0; k <= NT; ++k) {
        bc[k] = k <= p.N ? p.coef[k] : 0.0;
        ac[k] = k <= p.N ? p.coef[p.N + 1 + k] : 0.0;
    }
    const int64_t n0 = c * p.C, n1 = min(n0 + p.C, p.L);
#pragma unroll
    for (int k = 0; k < NT; ++k) xh[k] = k < p.N ? iir_in(p, x, pre, n0 - 1 - k) : 0.0;     // inputs as of sample n0-1 (shifted in the loop)
    xh[NT] = 0.0;
#pragma unroll
    for (int k = 0; k < NT; ++k) zh[k] = 0.0;
    double* z = p.z + (int64_t)b * p.L;
    for (int64_t n = n0; n < n1; ++n) {
#pragma unroll
        for (int k = NT; k >= 1; --k) xh[k] = xh[k - 1];
        xh[0] = iir_in(p, x, pre, n);
        double v = 0.0;
#pragma unroll
        for (int k = 0; k <= NT; ++k) v = fma(bc[k], xh[k], v);
#pragma unroll
        for (int k = NT; k >= 2; --k) v = fma(-ac[k], zh[k - 1], v);
        const double zn = fma(-ac[1], zh[0], v);            // the only term on the sample-to-sample dependency chain
#pragma unroll
        for (int k = NT - 1; k >= 1; --k) zh[k] = zh[k - 1];
        zh[0] = zn;
        z[n] = zn;
    }
    double* st = p.state + (b * n_chunks + c) * p.N;
#pragma unroll
    for (int j = 0; j < NT; ++j)
        if (j < p.N) st[j] = zh[j];
}

// one wavefront per row; lane j < N owns state component j
__global__ __launch_bounds__(64) void iir_scan_kernel(const aid_iir_params p, int64_t n_chunks) {
    __shared__ double s[IIR_MAX_N];
    const int b = blockIdx.x, j = threadIdx.x;
    const bool own = j < p.N;
    double phi[IIR_MAX_N];
#pragma unroll
    for (int i = 0; i < IIR_MAX_N; ++i) phi[i] = (own && i < p.N) ? p.H[(int64_t)(p.C - 1 - j) * p.N + i] : 0.0;
    if (j < IIR_MAX_N) s[j] = 0.0;
    __syncthreads();
    double* st = p.state + (int64_t)b * n_chunks * p.N;
    for (int64_t c = 0; c < n_chunks; ++c) {
        double a0 = own ? st[c * p.N + j] : 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
        for (int i = 0; i < IIR_MAX_N; i += 4) {
            a0 = fma(phi[i], s[i], a0);
            a1 = fma(phi[i + 1], s[i + 1], a1);
            a2 = fma(phi[i + 2], s[i + 2], a2);
            a3 = fma(phi[i + 3], s[i + 3], a3);
        }
        if (own) st[c * p.N + j] = s[j];                    // incoming state of chunk c
        __syncthreads();
        if (j < IIR_MAX_N) s[j] = (a0 + a1) + (a2 + a3);
        __syncthreads();
    }
}

__global__ __launch_bounds__(DG_THREADS) void iir_out_kernel(const aid_iir_params p, int64_t n_chunks) {
    const int b = blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * DG_THREADS + threadIdx.x;
    if (n >= p.L) return;
    const int64_t c = n / p.C;
    const double* s = p.state + ((int64_t)b * n_chunks + c) * p.N;
    const double* Hm = p.H + (n - c * p.C) * p.N;
    double y = p.z[(int64_t)b * p.L + n];
    for (int i = 0; i < p.N; ++i) y = fma(Hm[i], s[i], y);
    float v = (float)y;
    const int64_t ph = p.adjoint ? p.L - 1 - n : n;
    if (!p.adjoint && p.clamp) {
        if (p.pre) p.pre[(int64_t)b * p.L + ph] = v;
        v = fminf(fmaxf(v, -1.f), 1.f);
    }
    const int64_t o = (int64_t)b * p.out_ld + ph;
    p.out[o] = dg_epilogue(v, p.c0, p.add1, p.add2, o);
}

extern "C" int aid_iir(const aid_iir_params* p, void* stream) {
    AID_REQUIRE(p && p->x && p->out && p->coef && p->H && p->z && p->state, "aid_iir: null pointer");
    AID_REQUIRE(p->B > 0 && p->B <= 65535 && p->L > 0 && p->x_ld >= p->L && p->out_ld >= p->L, "aid_iir: bad shape or row stride");
    AID_REQUIRE(p->N >= 1 && p->N <= IIR_MAX_N, "aid_iir: order must be in [1, 16]");
    AID_REQUIRE(p->C >= p->N && p->C <= 65536, "aid_iir: chunk length must be in [N, 65536]");
    AID_REQUIRE(!(p->adjoint && p->clamp) || p->pre, "aid_iir: the clamped adjoint needs the forward's unclamped output");
    const int64_t n_chunks = (p->L + p->C - 1) / p->C;
    hipStream_t st = (hipStream_t)stream;
    const dim3 g1(aid_cdiv((int64_t)p->B * n_chunks, DG_THREADS));
    if (p->N <= 2)      hipLaunchKernelGGL(iir_chunk_kernel<2>, g1, dim3(DG_THREADS), 0, st, *p, n_chunks);
    else if (p->N <= 4) hipLaunchKernelGGL(iir_chunk_kernel<4>, g1, dim3(DG_THREADS), 0, st, *p, n_chunks);
    else if (p->N <= 8) hipLaunchKernelGGL(iir_chunk_kernel<8>, g1, dim3(DG_THREADS), 0, st, *p, n_chunks);
    else                hipLaunchKernelGGL(iir_chunk_kernel<16>, g1, dim3(DG_THREADS), 0, st, *p, n_chunks);
    AID_CHECK_LAUNCH();
    hipLaunchKernelGGL(iir_scan_kernel, dim3(p->B), dim3(64), 0, st, *p, n_chunks);
    AID_CHECK_LAUNCH();
    hipLaunchKernelGGL(iir_out_kernel, dim3(aid_cdiv(p->L, DG_THREADS), p->B), dim3(DG_THREADS), 0, st, *p, n_chunks);
    AID_CHECK_LAUNCH();
    return AID_OK;
}

// ---- clip -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DG_THREADS) void clip_kernel(const aid_clip_params p) {
    const int b = blockIdx.y;
    for (int64_t i = (int64_t)blockIdx.x * DG_THREADS + threadIdx.x; i < p.L; i += (int64_t)gridDim.x * DG_THREADS) {
        const float v = p.x[(int64_t)b * p.x_ld + i];
        float a;
        if (p.adjoint) {
            const float r = p.xref[(int64_t)b * p.L + i];
            a = (r >= -p.clip && r <= p.clip) ? v : 0.f;
        } else {
            a = fminf(fmaxf(v, -p.clip), p.clip);
        }
        const int64_t o = (int64_t)b * p.out_ld + i;
        p.out[o] = dg_epilogue(a, p.c0, p.add1, p.add2, o);
    }
}

extern "C" int aid_clip(const aid_clip_params* p, void* stream) {
    AID_REQUIRE(p && p->x && p->out && (!p->adjoint || p->xref), "aid_clip: null pointer");
    AID_REQUIRE(p->B > 0 && p->B <= 65535 && p->L > 0 && p->x_ld >= p->L && p->out_ld >= p->L, "aid_clip: bad shape or row stride");
    AID_REQUIRE(p->clip >= 0.f, "aid_clip: negative clip value");
    int gx = aid_cdiv(p->L, DG_THREADS); if (gx > 2048) gx = 2048;
    hipLaunchKernelGGL(clip_kernel, dim3(gx, p->B), dim3(DG_THREADS), 0, (hipStream_t)stream, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}
