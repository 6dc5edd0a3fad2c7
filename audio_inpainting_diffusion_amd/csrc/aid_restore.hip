// Window gather / scatter of whole-recording restoration (include/aid_restore.h): one pass of the restoration gathers the observations
// and masks of all its windows into one batch and, after the sampler ran, writes back the samples every window owns.  Pure streaming
// copies: J * L floats of y and of m written per gather, as many read; at most J * L floats moved per scatter.
//
//   grid (tiles, J): block row j handles job j.  Rows go by float4 over the aligned body of the destination and by scalars at its ragged
//   ends (aid_rows.h).  A float4 of the gather that straddles the end of the leading observed part, the start of the trailing one or
//   sample N goes element by element.
#include "aid_rows.h"

__global__ __launch_bounds__(RS_THREADS) void window_gather_kernel(const aid_window_gather_params p) {
    const int j = blockIdx.y;
    const int64_t L = p.L;
    const int64_t tid = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x, nthreads = (int64_t)gridDim.x * RS_THREADS;
    const rs_window w = rs_load_window(p.jobs, j, p.R, L, p.N, 1);                   // (an invalid job gathers zeros with mask 0)
    const int64_t n_in = w.n_in, head = w.head, tail0 = w.tail0, r = w.r, s = w.s;
    const float* __restrict__ rec = p.rec + r * p.rec_ld + s;                         // (dereferenced at i < n_in only)
    const float* __restrict__ out = p.out + r * p.out_ld + s;
    const float* __restrict__ mask = p.mask + r * p.mask_ld + s;
    float* __restrict__ y = p.y + (int64_t)j * L;
    float* __restrict__ m = p.m + (int64_t)j * L;

    auto elem = [&](int64_t i, float& yv, float& mv) {
        const bool in = i < n_in, edge = i < head || i >= tail0;
        mv = edge ? 1.f : (in ? mask[i] : 0.f);
        yv = mv * (in ? (edge ? out[i] : rec[i]) : 0.f);
    };

    const bool m_al = rs_aligned_as(m, y), rec_al = rs_aligned_as(rec, y), out_al = rs_aligned_as(out, y), mask_al = rs_aligned_as(mask, y);
    rs_walk(y, L, tid, nthreads, [&](int64_t i) {
        float4 yv, mv;
        if (i + 4 <= n_in && (i + 4 <= head || i >= tail0)) {                       // wholly observed from the result so far
            mv = make_float4(1.f, 1.f, 1.f, 1.f);
            yv = rs_ld4(out + i, out_al);
        } else if (i + 4 <= n_in && i >= head && i + 4 <= tail0) {                   // wholly the recording under its mask
            mv = rs_ld4(mask + i, mask_al);
            const float4 x = rs_ld4(rec + i, rec_al);
            yv = make_float4(mv.x * x.x, mv.y * x.y, mv.z * x.z, mv.w * x.w);
        } else {
            elem(i, yv.x, mv.x); elem(i + 1, yv.y, mv.y); elem(i + 2, yv.z, mv.z); elem(i + 3, yv.w, mv.w);
        }
        *reinterpret_cast<float4*>(y + i) = yv;
        rs_st4(m + i, m_al, mv);
    }, [&](int64_t i) { elem(i, y[i], m[i]); });
}

// dst[i] = src[i] for i < n   (tid / nthreads: this lane's index and the lane count over the row)
__device__ __forceinline__ void rs_copy_row(float* __restrict__ dst, const float* __restrict__ src, int64_t n, int64_t tid, int64_t nthreads) {
    const bool src_al = rs_aligned_as(src, dst);
    rs_walk(dst, n, tid, nthreads, [&](int64_t i) { *reinterpret_cast<float4*>(dst + i) = rs_ld4(src + i, src_al); },
            [&](int64_t i) { dst[i] = src[i]; });
}

__global__ __launch_bounds__(RS_THREADS) void window_scatter_kernel(const aid_window_scatter_params p) {
    const int j = blockIdx.y;
    const int64_t tid = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x, nthreads = (int64_t)gridDim.x * RS_THREADS;
    const rs_job b = rs_load_job(p.jobs, j, p.R, p.L, p.N);
    if (!b.ok) return;
    const int64_t hi = p.N - b.s < b.hi ? p.N - b.s : b.hi;                          // samples at or past N do not exist
    if (hi <= b.lo) return;
    rs_copy_row(p.out + b.r * p.out_ld + b.s + b.lo, p.x + (int64_t)j * p.L + b.lo, hi - b.lo, tid, nthreads);
}

extern "C" int aid_restore_abi_version(void) { return AID_RESTORE_ABI_VERSION; }

extern "C" int aid_window_gather(const aid_window_gather_params* p, void* stream) {
    AID_REQUIRE(p && p->rec && p->out && p->mask && p->y && p->m && p->jobs, "aid_window_gather: null pointer");
    AID_REQUIRE(p->J > 0 && p->J <= 65535 && p->R > 0 && p->L > 0 && p->N > 0, "aid_window_gather: empty or oversized shape (1 <= J <= 65535)");
    AID_REQUIRE(p->rec_ld >= p->N && p->out_ld >= p->N && (p->mask_ld == 0 || p->mask_ld >= p->N), "aid_window_gather: a row stride is shorter than N");
    hipLaunchKernelGGL(window_gather_kernel, dim3(rs_tiles(p->L), p->J), dim3(RS_THREADS), 0, (hipStream_t)stream, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}

extern "C" int aid_window_scatter(const aid_window_scatter_params* p, void* stream) {
    AID_REQUIRE(p && p->x && p->out && p->jobs, "aid_window_scatter: null pointer");
    AID_REQUIRE(p->J > 0 && p->J <= 65535 && p->R > 0 && p->L > 0 && p->N > 0, "aid_window_scatter: empty or oversized shape (1 <= J <= 65535)");
    AID_REQUIRE(p->out_ld >= p->N, "aid_window_scatter: the row stride of out is shorter than N");
    hipLaunchKernelGGL(window_scatter_kernel, dim3(rs_tiles(p->L), p->J), dim3(RS_THREADS), 0, (hipStream_t)stream, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}
