// The exact adjoint of aid_resample_poly (include/aid_resample_op.h): the transposed rational-ratio polyphase sinc resampler, which
// reconstruction guidance through the "resample" degradation of bandwidth extension needs once per denoiser evaluation.
//
//   gx[b, q] = sum over frames i with 0 <= t = q + width - i*orig < K, over phases j with i*new + j < Lout, of kT[t][j] * g[b, i*new + j]
//
//   grid (ceil(L / 256), B): one thread owns one gx[b, q] and gathers its terms -- no atomics, frames and phases in ascending order, so the
//   result is deterministic.  The frames that reach q are i_lo = ceil((q + width - K + 1) / orig) .. i_hi = floor((q + width) / orig), cut to
//   [0, (Lout - 1) / new]: about K / orig of them.  Of a frame's phases only [j_lo[t], j_hi[t]) is visited, the range outside which the host
//   found kT[t][.] exactly 0.0f (the clamped Hann window): at 147:100 about 12 terms per sample instead of about 112 (K * new / orig).  Tiny next to the
//   network (at 8 x 184184: 4 MB read, 6 MB written; the table, at most a few hundred KB, stays in cache), so no staging.
#include "aid_common.h"
#include "aid_resample_op.h"

#define RA_THREADS 256

__global__ __launch_bounds__(RA_THREADS) void resample_poly_adj_kernel(const aid_resample_poly_adj_params p) {
    const int64_t q = (int64_t)blockIdx.x * RA_THREADS + threadIdx.x;
    if (q >= p.L) return;
    const int64_t b = blockIdx.y;
    const int64_t orig = p.orig_freq, nw = p.new_freq;
    const float* __restrict__ g = p.g + b * p.g_ld;
    const int64_t top = q + p.width;                       // t = top - i*orig
    const int64_t num = top - (p.K - 1);                   // t <= K - 1  <=>  i*orig >= num
    int64_t i_lo = num <= 0 ? 0 : (num + orig - 1) / orig;
    int64_t i_hi = top / orig;                             // t >= 0
    const int64_t i_last = (p.Lout - 1) / nw;              // the last frame that holds an output sample
    if (i_hi > i_last) i_hi = i_last;
    float acc = 0.f;
    for (int64_t i = i_lo; i <= i_hi; ++i) {
        const int t = (int)(top - i * orig);               // in [0, K) by the bounds of i
        const int64_t n0 = i * nw;                         // < Lout
        int jl = p.j_lo[t], jh = p.j_hi[t];
        if (jl < 0) jl = 0;
        if (jh > p.new_freq) jh = p.new_freq;
        if (p.Lout - n0 < jh) jh = (int)(p.Lout - n0);     // the last frame is cut by Lout
        const float* __restrict__ k = p.kT + (int64_t)t * nw;
        for (int j = jl; j < jh; ++j) acc += k[j] * g[n0 + j];
    }
    p.gx[b * p.gx_ld + q] = acc;
}

extern "C" int aid_resample_op_abi_version(void) { return AID_RESAMPLE_OP_ABI_VERSION; }

extern "C" int aid_resample_poly_adj(const aid_resample_poly_adj_params* p, void* stream) {
    AID_REQUIRE(p && p->g && p->gx && p->kT && p->j_lo && p->j_hi, "aid_resample_poly_adj: null pointer");
    AID_REQUIRE(p->orig_freq > 0 && p->new_freq > 0 && p->width >= 0 && p->K == 2 * p->width + p->orig_freq && p->L > 0 && p->Lout > 0,
                "aid_resample_poly_adj: bad geometry (K must be 2*width + orig_freq)");
    AID_REQUIRE(p->B > 0 && p->B <= 65535, "aid_resample_poly_adj: empty or oversized batch (1 <= B <= 65535)");
    AID_REQUIRE(p->Lout <= (p->L * p->new_freq + p->orig_freq - 1) / p->orig_freq, "aid_resample_poly_adj: Lout exceeds ceil(new*L/orig)");
    AID_REQUIRE(p->g_ld >= p->Lout && p->gx_ld >= p->L, "aid_resample_poly_adj: a row stride is shorter than its row");
    AID_REQUIRE((p->L + RA_THREADS - 1) / RA_THREADS <= 0x7fffffffLL, "aid_resample_poly_adj: signal too long for one launch");
    hipLaunchKernelGGL(resample_poly_adj_kernel, dim3((unsigned)((p->L + RA_THREADS - 1) / RA_THREADS), p->B), dim3(RA_THREADS), 0,
                       (hipStream_t)stream, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}
