// Bandwidth extension of whole recordings that are also clipped and have dropouts (include/aid_bwe_long.h: aid_fir_clip_observed;
// include/aid_restore.h: aid_gap_states): the observation operator of a window seen through a stride-1 FIR filter FOLLOWED BY a hard clipper,
// whose samples are filtered (state 0), known (> 0), unobserved (-1) or absent (<= -2) -- apply and adjoint, one launch each -- and the
// pass over the gathered rows of aid_bwe_gather that turns a dropped filtered sample into an unobserved one.
//
//   fir_clip_observed: fir_observed_kernel's structure (aid_bwe_long.hip) on fir_tile (aid_fir_tile.h): grid (tiles of 2048 outputs, rows);
//        the state decides when the tile is staged into LDS and again in the epilogue.  No LDS beyond fir_tile's, no atomics; the arithmetic
//        and its order are fir_tile's, so the sums carry aid_fir_observed's bits.  The level of row b stands behind the taps, h[K + b].
//        Apply: 2 floats read per staged sample (sample, state), 2 in the epilogue, 2 written (the observation, and the pre-clip sum the
//        adjoint gates on).  Adjoint: 3 floats read per staged sample (gradient, state, pre-clip sum), 2 in the epilogue, 1 written.
//   gap_states: grid (tiles, jobs), in place over the rows of y and m: float4 over the aligned body of a row of y where the four samples
//        exist, element by element at the ragged ends and across sample N (aid_rows.h); a float4 is written back only where one of its
//        samples changed.  The job table is device memory: every access is bounded here.
#include "aid_rows.h"
#include "aid_fir_tile.h"
#include "aid_bwe_long.h"

// MODE 0 apply (two planes), 1 adjoint
template <int MODE>
__global__ __launch_bounds__(FIR_THREADS) void fir_clip_observed_kernel(const aid_fir_observed_params p) {
    const int64_t b = blockIdx.y, L = p.L;
    const int t = threadIdx.x;
    const int64_t tile0 = (int64_t)blockIdx.x * FIR_TO;
    const float* __restrict__ x = p.x + b * p.x_ld;
    const float* __restrict__ k = p.state + b * p.state_ld;
    const int P = (p.K - 1) / 2;
    const float cb = p.h[p.K + b];
    double accd[FIR_R];
    if (MODE == 1) {
        const float* __restrict__ y = p.y + b * p.y_ld;                              // the pre-clip sums of the matching apply
        fir_tile([&](int64_t q) {
            if (q < 0 || q >= L || k[q] != 0.f) return 0.f;
            const float yv = y[q];
            return (yv >= -cb && yv <= cb) ? x[q] : 0.f;
        }, tile0, p.h, p.K, p.K - 1 - P, 1, accd);
    } else {
        fir_tile([&](int64_t q) { return (q >= 0 && q < L && !rs_absent(k[q])) ? x[q] : 0.f; }, tile0, p.h, p.K, P, 0, accd);
    }
    float* __restrict__ out = p.out + b * p.out_ld;
    float* __restrict__ pre = out + (int64_t)p.B * p.out_ld;                         // plane 1 (MODE 0)
#pragma unroll
    for (int r = 0; r < FIR_R; ++r) {
        const int64_t i = tile0 + t * FIR_R + r;
        if (i < L) {
            const float c = (float)accd[r], kv = k[i], xv = x[i];
            if (MODE == 0) {
                out[i] = rs_known(kv) ? xv : (kv == 0.f ? fminf(fmaxf(c, -cb), cb) : 0.f);
                pre[i] = kv == 0.f ? c : 0.f;
            } else {
                out[i] = rs_absent(kv) ? 0.f : (rs_known(kv) ? c + xv : c);
            }
        }
    }
}

__global__ __launch_bounds__(RS_THREADS) void gap_states_kernel(const aid_window_gather_params p) {
    const int j = blockIdx.y;
    const int64_t L = p.L;
    const int64_t tid = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x, nthreads = (int64_t)gridDim.x * RS_THREADS;
    const rs_window w = rs_load_window(p.jobs, j, p.R, L, p.N, 1);
    if (!w.ok) return;                                                               // (an invalid job's rows stay as they are)
    const int64_t n_in = w.n_in;
    const float* __restrict__ mask = p.mask + w.r * p.mask_ld + w.s;                 // (dereferenced at i < n_in only)
    float* __restrict__ y = p.y + (int64_t)j * L;
    float* __restrict__ m = p.m + (int64_t)j * L;

    auto elem = [&](int64_t i) {
        if (i < n_in && m[i] == 0.f && mask[i] == 0.f) { m[i] = -1.f; y[i] = 0.f; }
    };

    const bool m_al = rs_aligned_as(m, y), mask_al = rs_aligned_as(mask, y);
    rs_walk(y, L, tid, nthreads, [&](int64_t i) {
        if (i >= n_in) return;
        if (i + 4 > n_in) { elem(i); elem(i + 1); elem(i + 2); elem(i + 3); return; }
        float4 mv = rs_ld4(m + i, m_al);
        const float4 kv = rs_ld4(mask + i, mask_al);
        const bool gx = mv.x == 0.f && kv.x == 0.f, gy = mv.y == 0.f && kv.y == 0.f, gz = mv.z == 0.f && kv.z == 0.f, gw = mv.w == 0.f && kv.w == 0.f;
        if (!(gx || gy || gz || gw)) return;
        float4 yv = *reinterpret_cast<const float4*>(y + i);
        if (gx) { mv.x = -1.f; yv.x = 0.f; }
        if (gy) { mv.y = -1.f; yv.y = 0.f; }
        if (gz) { mv.z = -1.f; yv.z = 0.f; }
        if (gw) { mv.w = -1.f; yv.w = 0.f; }
        *reinterpret_cast<float4*>(y + i) = yv;
        rs_st4(m + i, m_al, mv);
    }, elem);
}

extern "C" int aid_fir_clip_observed(const aid_fir_observed_params* p, void* stream) {
    AID_REQUIRE(p && p->x && p->state && p->h && p->out, "aid_fir_clip_observed: null pointer");
    AID_REQUIRE(p->mode == 0 || p->mode == 1, "aid_fir_clip_observed: mode must be 0 (apply) or 1 (adjoint): the clipped filter has no projection");
    AID_REQUIRE(p->mode != 1 || (p->y && p->y_ld >= p->L), "aid_fir_clip_observed: the adjoint needs y, plane 1 of the matching apply, with a row stride >= L");
    AID_REQUIRE(p->B > 0 && p->B <= 65535 && p->K > 0 && p->L > 0, "aid_fir_clip_observed: empty or oversized shape (1 <= B <= 65535, K >= 1)");
    AID_REQUIRE(p->x_ld >= p->L && p->out_ld >= p->L && (p->state_ld == 0 || p->state_ld >= p->L), "aid_fir_clip_observed: a row stride is shorter than L");
    const dim3 grid(aid_cdiv(p->L, FIR_TO), p->B), block(FIR_THREADS);
    if (p->mode == 0) hipLaunchKernelGGL(fir_clip_observed_kernel<0>, grid, block, 0, (hipStream_t)stream, *p);
    else hipLaunchKernelGGL(fir_clip_observed_kernel<1>, grid, block, 0, (hipStream_t)stream, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}

extern "C" int aid_gap_states(const aid_window_gather_params* p, void* stream) {
    AID_REQUIRE(p && p->mask && p->y && p->m && p->jobs, "aid_gap_states: null pointer (mask, y, m and jobs are read; rec and out are unused)");
    AID_REQUIRE(p->J > 0 && p->J <= 65535 && p->R > 0 && p->L > 0 && p->N > 0, "aid_gap_states: empty or oversized shape (1 <= J <= 65535)");
    AID_REQUIRE(p->mask_ld == 0 || p->mask_ld >= p->N, "aid_gap_states: the row stride of mask is shorter than N");
    hipLaunchKernelGGL(gap_states_kernel, dim3(rs_tiles(p->L), p->J), dim3(RS_THREADS), 0, (hipStream_t)stream, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}
