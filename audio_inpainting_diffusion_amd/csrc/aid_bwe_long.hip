// Bandwidth extension of whole recordings (include/aid_bwe_long.h): the observation operator of a window seen through a stride-1 FIR
// filter whose samples are filtered (state 0), known (> 0), unobserved (-1) or absent (<= -2) -- apply, adjoint and the data-consistency
// projection -- and the gather that builds the observations and states of all windows of a pass.
//
//   fir_observed: grid (tiles of 2048 outputs, rows), the tile loop of aid_fir (fir_tile, aid_fir_tile.h).  The state decides twice: what a
//        sample is when the tile is staged into LDS (an absent sample enters the filter as 0; the adjoint correlates the gradient of the
//        filtered samples only) and what the output is in the epilogue.  No LDS beyond fir_tile's, no atomics.  Per output 2 floats read
//        on the way in (sample and state, plus the halo of K - 1 per tile) and up to 3 in the epilogue, 1 written.
//   bwe_gather: grid (tiles, jobs), pure streaming as aid_declip_gather: float4 over the aligned body of the destination where a
//        float4 lies wholly inside the filtered part, element by element at the seams and at the ragged ends (aid_rows.h).  The job table
//        is device memory: every access is bounded here.
#include "aid_rows.h"
#include "aid_fir_tile.h"
#include "aid_bwe_long.h"

// MODE 0 apply, 1 adjoint, 2 projection
template <int MODE>
__global__ __launch_bounds__(FIR_THREADS) void fir_observed_kernel(const aid_fir_observed_params p) {
    const int64_t b = blockIdx.y, L = p.L;
    const int t = threadIdx.x;
    const int64_t tile0 = (int64_t)blockIdx.x * FIR_TO;
    const float* __restrict__ x = p.x + b * p.x_ld;
    const float* __restrict__ k = p.state + b * p.state_ld;
    const int P = (p.K - 1) / 2;
    double accd[FIR_R];
    if (MODE == 1) fir_tile([&](int64_t q) { return (q >= 0 && q < L && k[q] == 0.f) ? x[q] : 0.f; }, tile0, p.h, p.K, p.K - 1 - P, 1, accd);
    else           fir_tile([&](int64_t q) { return (q >= 0 && q < L && !rs_absent(k[q])) ? x[q] : 0.f; }, tile0, p.h, p.K, P, 0, accd);
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

__global__ __launch_bounds__(RS_THREADS) void bwe_gather_kernel(const aid_bwe_gather_params p) {
    const int j = blockIdx.y;
    const int64_t L = p.L;
    const int64_t tid = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x, nthreads = (int64_t)gridDim.x * RS_THREADS;
    const rs_window w = rs_load_window(p.jobs, j, p.R, L, p.N, 1);                   // (an invalid job gathers zeros, all absent)
    const int64_t n_in = w.n_in, head = w.head, tail0 = w.tail0, r = w.r, s = w.s;
    const int64_t P = (p.K - 1) / 2, Q = p.K - 1 - P;
    // unobserved: i < u0 or i >= u1 (the filter support of such a sample leaves the window although the recording goes on there)
    const int64_t u0 = s > 0 ? P : 0, u1 = (w.ok && s + L < p.N) ? L - Q : L;
    // filtered exactly on [f0, f1), when that is a range
    const int64_t f0 = head > u0 ? head : u0, f1 = tail0 < u1 ? (tail0 < n_in ? tail0 : n_in) : (u1 < n_in ? u1 : n_in);
    const float* __restrict__ rec = p.rec + r * p.rec_ld + s;                         // (dereferenced at i < n_in only)
    const float* __restrict__ out = p.out + r * p.out_ld + s;
    float* __restrict__ y = p.y + (int64_t)j * L;
    float* __restrict__ k = p.state + (int64_t)j * L;

    auto elem = [&](int64_t i, float& yv, float& kv) {
        const bool in = i < n_in, edge = i < head || i >= tail0, un = i < u0 || i >= u1;
        kv = in ? (edge ? 1.f : (un ? -1.f : 0.f)) : -2.f;
        yv = in ? (edge ? out[i] : (un ? 0.f : rec[i])) : 0.f;
    };

    const bool k_al = rs_aligned_as(k, y), rec_al = rs_aligned_as(rec, y);
    rs_walk(y, L, tid, nthreads, [&](int64_t i) {
        float4 yv, kv;
        if (i >= f0 && i + 4 <= f1) {                                                // wholly the filtered recording
            kv = make_float4(0.f, 0.f, 0.f, 0.f);
            yv = rs_ld4(rec + i, rec_al);
        } else {
            elem(i, yv.x, kv.x); elem(i + 1, yv.y, kv.y); elem(i + 2, yv.z, kv.z); elem(i + 3, yv.w, kv.w);
        }
        *reinterpret_cast<float4*>(y + i) = yv;
        rs_st4(k + i, k_al, kv);
    }, [&](int64_t i) { elem(i, y[i], k[i]); });
}

extern "C" int aid_bwe_long_abi_version(void) { return AID_BWE_LONG_ABI_VERSION; }

extern "C" int aid_fir_observed(const aid_fir_observed_params* p, void* stream) {
    AID_REQUIRE(p && p->x && p->state && p->h && p->out, "aid_fir_observed: null pointer");
    AID_REQUIRE(p->mode >= 0 && p->mode <= 2, "aid_fir_observed: mode must be 0 (apply), 1 (adjoint) or 2 (projection)");
    AID_REQUIRE(p->mode != 2 || (p->y && p->y_ld >= p->L), "aid_fir_observed: the projection needs y with a row stride >= L");
    AID_REQUIRE(p->B > 0 && p->B <= 65535 && p->K > 0 && p->L > 0, "aid_fir_observed: empty or oversized shape (1 <= B <= 65535, K >= 1)");
    AID_REQUIRE(p->x_ld >= p->L && p->out_ld >= p->L && (p->state_ld == 0 || p->state_ld >= p->L), "aid_fir_observed: a row stride is shorter than L");
    const dim3 grid(aid_cdiv(p->L, FIR_TO), p->B), block(FIR_THREADS);
    if (p->mode == 0) hipLaunchKernelGGL(fir_observed_kernel<0>, grid, block, 0, (hipStream_t)stream, *p);
    else if (p->mode == 1) hipLaunchKernelGGL(fir_observed_kernel<1>, grid, block, 0, (hipStream_t)stream, *p);
    else hipLaunchKernelGGL(fir_observed_kernel<2>, grid, block, 0, (hipStream_t)stream, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}

extern "C" int aid_bwe_gather(const aid_bwe_gather_params* p, void* stream) {
    AID_REQUIRE(p && p->rec && p->out && p->y && p->state && p->jobs, "aid_bwe_gather: null pointer");
    AID_REQUIRE(p->J > 0 && p->J <= 65535 && p->R > 0 && p->K > 0 && p->L > 0 && p->N > 0, "aid_bwe_gather: empty or oversized shape (1 <= J <= 65535, K >= 1)");
    AID_REQUIRE(p->rec_ld >= p->N && p->out_ld >= p->N, "aid_bwe_gather: a row stride is shorter than N");
    hipLaunchKernelGGL(bwe_gather_kernel, dim3(rs_tiles(p->L), p->J), dim3(RS_THREADS), 0, (hipStream_t)stream, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}
