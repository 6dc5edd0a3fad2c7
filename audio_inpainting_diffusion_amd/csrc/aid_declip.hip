// Declipping of whole recordings (include/aid_declip.h): the observation operator of a window whose samples are clipped (state 0),
// known (state > 0) or absent (state < 0) -- apply, adjoint and the projection onto the signals consistent with the observation -- and
// the gather that builds the observations, states and clip levels of all windows of a pass.  Pure streaming: per element of
// aid_clip_known 2 (apply) or 3 floats read and 1 written; J * L floats of y and of k written per gather, as many read.
//
//   grid (tiles, rows): block row b handles signal / job b.  Rows go by float4 over the aligned body of the destination and by scalars
//   at its ragged ends (aid_rows.h).  A float4 of the gather that straddles the end of the leading known part, the start of the trailing
//   one or sample N goes element by element.  No atomics; selections, comparisons, min and max only, so every result is exact.
#include "aid_rows.h"
#include "aid_declip.h"

// a: xref (MODE 1) or y (MODE 2); unused in MODE 0
template <int MODE>
__device__ __forceinline__ float ck_elem(float x, float a, float k, float c) {
    if (MODE == 0) return k > 0.f ? x : (k < 0.f ? 0.f : fminf(fmaxf(x, -c), c));
    if (MODE == 1) return k > 0.f ? x : (k < 0.f ? 0.f : ((a >= -c && a <= c) ? x : 0.f));
    return k > 0.f ? a : (k < 0.f ? x : (a >= c ? fmaxf(x, c) : (a <= -c ? fminf(x, -c) : a)));
}

template <int MODE>
__global__ __launch_bounds__(RS_THREADS) void clip_known_kernel(const aid_clip_known_params p) {
    const int64_t b = blockIdx.y, L = p.L;
    const int64_t tid = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x, nthreads = (int64_t)gridDim.x * RS_THREADS;
    const float c = p.clip[b];
    const float* __restrict__ x = p.x + b * p.x_ld;
    const float* __restrict__ k = p.state + b * p.state_ld;
    const float* __restrict__ a = MODE == 1 ? p.xref + b * p.xref_ld : (MODE == 2 ? p.y + b * p.y_ld : x);    // (MODE 0 never reads it)
    float* __restrict__ out = p.out + b * p.out_ld;

    auto elem = [&](int64_t i) { out[i] = ck_elem<MODE>(x[i], MODE ? a[i] : 0.f, k[i], c); };

    const bool x_al = rs_aligned_as(x, out), k_al = rs_aligned_as(k, out), a_al = rs_aligned_as(a, out);
    rs_walk(out, L, tid, nthreads, [&](int64_t i) {
        const float4 xv = rs_ld4(x + i, x_al), kv = rs_ld4(k + i, k_al);
        const float4 av = MODE ? rs_ld4(a + i, a_al) : xv;
        *reinterpret_cast<float4*>(out + i) = make_float4(ck_elem<MODE>(xv.x, av.x, kv.x, c), ck_elem<MODE>(xv.y, av.y, kv.y, c),
                                                          ck_elem<MODE>(xv.z, av.z, kv.z, c), ck_elem<MODE>(xv.w, av.w, kv.w, c));
    }, elem);
}

__global__ __launch_bounds__(RS_THREADS) void declip_gather_kernel(const aid_declip_gather_params p) {
    const int j = blockIdx.y;
    const int64_t L = p.L;
    const int64_t tid = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x, nthreads = (int64_t)gridDim.x * RS_THREADS;
    const rs_window w = rs_load_window(p.jobs, j, p.R, L, p.N, 1);                   // (an invalid job gathers zeros, all absent)
    const int64_t n_in = w.n_in, head = w.head, tail0 = w.tail0, r = w.r, s = w.s;
    const float* __restrict__ rec = p.rec + r * p.rec_ld + s;                         // (dereferenced at i < n_in only)
    const float* __restrict__ out = p.out + r * p.out_ld + s;
    float* __restrict__ y = p.y + (int64_t)j * L;
    float* __restrict__ k = p.k + (int64_t)j * L;
    if (tid == 0) p.c[j] = w.ok ? p.clip[r] : 0.f;

    auto elem = [&](int64_t i, float& yv, float& kv) {
        const bool in = i < n_in, edge = i < head || i >= tail0;
        kv = in ? (edge ? 1.f : 0.f) : -1.f;
        yv = in ? (edge ? out[i] : rec[i]) : 0.f;
    };

    const bool k_al = rs_aligned_as(k, y), rec_al = rs_aligned_as(rec, y), out_al = rs_aligned_as(out, y);
    rs_walk(y, L, tid, nthreads, [&](int64_t i) {
        float4 yv, kv;
        if (i + 4 <= n_in && (i + 4 <= head || i >= tail0)) {                       // wholly known from the result so far
            kv = make_float4(1.f, 1.f, 1.f, 1.f);
            yv = rs_ld4(out + i, out_al);
        } else if (i + 4 <= n_in && i >= head && i + 4 <= tail0) {                   // wholly the clipped recording
            kv = make_float4(0.f, 0.f, 0.f, 0.f);
            yv = rs_ld4(rec + i, rec_al);
        } else if (i >= n_in) {                                                      // wholly past the end of the recording
            kv = make_float4(-1.f, -1.f, -1.f, -1.f);
            yv = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            elem(i, yv.x, kv.x); elem(i + 1, yv.y, kv.y); elem(i + 2, yv.z, kv.z); elem(i + 3, yv.w, kv.w);
        }
        *reinterpret_cast<float4*>(y + i) = yv;
        rs_st4(k + i, k_al, kv);
    }, [&](int64_t i) { elem(i, y[i], k[i]); });
}

extern "C" int aid_declip_abi_version(void) { return AID_DECLIP_ABI_VERSION; }

extern "C" int aid_clip_known(const aid_clip_known_params* p, void* stream) {
    AID_REQUIRE(p && p->x && p->state && p->clip && p->out, "aid_clip_known: null pointer");
    AID_REQUIRE(p->mode >= 0 && p->mode <= 2, "aid_clip_known: mode must be 0 (apply), 1 (adjoint) or 2 (projection)");
    AID_REQUIRE(p->mode != 1 || (p->xref && p->xref_ld >= p->L), "aid_clip_known: the adjoint needs xref with a row stride >= L");
    AID_REQUIRE(p->mode != 2 || (p->y && p->y_ld >= p->L), "aid_clip_known: the projection needs y with a row stride >= L");
    AID_REQUIRE(p->B > 0 && p->B <= 65535 && p->L > 0, "aid_clip_known: empty or oversized shape (1 <= B <= 65535)");
    AID_REQUIRE(p->x_ld >= p->L && p->out_ld >= p->L && (p->state_ld == 0 || p->state_ld >= p->L), "aid_clip_known: a row stride is shorter than L");
    const dim3 grid(rs_tiles(p->L), p->B), block(RS_THREADS);
    if (p->mode == 0) hipLaunchKernelGGL(clip_known_kernel<0>, grid, block, 0, (hipStream_t)stream, *p);
    else if (p->mode == 1) hipLaunchKernelGGL(clip_known_kernel<1>, grid, block, 0, (hipStream_t)stream, *p);
    else hipLaunchKernelGGL(clip_known_kernel<2>, grid, block, 0, (hipStream_t)stream, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}

extern "C" int aid_declip_gather(const aid_declip_gather_params* p, void* stream) {
    AID_REQUIRE(p && p->rec && p->out && p->clip && p->y && p->k && p->c && p->jobs, "aid_declip_gather: null pointer");
    AID_REQUIRE(p->J > 0 && p->J <= 65535 && p->R > 0 && p->L > 0 && p->N > 0, "aid_declip_gather: empty or oversized shape (1 <= J <= 65535)");
    AID_REQUIRE(p->rec_ld >= p->N && p->out_ld >= p->N, "aid_declip_gather: a row stride is shorter than N");
    hipLaunchKernelGGL(declip_gather_kernel, dim3(rs_tiles(p->L), p->J), dim3(RS_THREADS), 0, (hipStream_t)stream, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}
