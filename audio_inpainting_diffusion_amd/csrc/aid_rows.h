// Row helpers shared by the kernels of whole-recording restoration (aid_restore.hip, aid_declip.hip, aid_bwe_long.hip, aid_bwe_declip_long.hip,
// aid_lowrate_long.hip, aid_phase_long.hip, aid_spec_long.hip): the job table of include/aid_restore.h and the window of a job, the state codes of a window's
// entries, float4 access over the 16-byte-aligned body of a row with scalars at its ragged ends, and the tile count.
//
//   STATE CODES of an entry of a window (float32, one per sample and, where a mode has them, one per low-rate sample or frame):
//         1  known        the sample is taken from the result so far (head / tail of a pass-B window)
//         0  observed     the entry is seen through the degradation: y holds the recording's own value
//        -1  unobserved   the entry exists, but its observation depends on samples outside the window (or there is no direct one)
//        -2  absent       beyond the end of the recording; a sample enters the operator as 0
//     rs_known / rs_absent are the two tests the operator kernels make (k > 0, k <= -2); 0 is tested as k == 0.
//     Declipping keeps three codes of its own (aid_declip.h: 1 known, 0 clipped, -1 = ABSENT; its kernel tests k < 0), since a clipped
//     sample is always observed.
//   A row is written with float4 stores over the 16-byte-aligned body of the DESTINATION and scalar stores over its head (< 4 elements)
//   and tail; a source is read as float4 where it is aligned at the same element and as four scalars otherwise (window starts, owned
//   ranges and row strides are in general not multiples of 4).
//   The job table is device memory the launcher cannot inspect: every access is bounded by the kernels (r in [0, R), 0 <= s < N, q < N).
#pragma once
#include "aid_common.h"
#include "aid_restore.h"

#define RS_THREADS 256

struct rs_job { int64_t r, s, head, tail, lo, hi; bool ok; };

__device__ __forceinline__ int64_t rs_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__device__ __forceinline__ rs_job rs_load_job(const int64_t* __restrict__ jobs, int j, int R, int64_t L, int64_t N) {
    const int64_t* t = jobs + (int64_t)j * AID_RESTORE_JOB_FIELDS;
    rs_job b;
    b.r = t[0]; b.s = t[1];
    b.head = rs_clamp(t[2], L); b.tail = rs_clamp(t[3], L); b.lo = rs_clamp(t[4], L); b.hi = rs_clamp(t[5], L);
    b.ok = b.r >= 0 && b.r < R && b.s >= 0 && b.s < N;
    return b;
}

__device__ __forceinline__ bool rs_known(float k) { return k > 0.f; }
__device__ __forceinline__ bool rs_absent(float k) { return k <= -2.f; }

// The window of job j as a gather reads it: sample s + i of recording r exists for i < n_in (at most L), and is known from the result so
// far for i < head or i >= tail0.  A job that is not ok -- r outside [0, R), s outside [0, N) or no multiple of ``period`` (1: any start) --
// gathers nothing: r = s = n_in = head = 0 and tail0 = L.
struct rs_window { int64_t r, s, n_in, head, tail0; bool ok; };

__device__ __forceinline__ rs_window rs_load_window(const int64_t* __restrict__ jobs, int j, int R, int64_t L, int64_t N, int64_t period) {
    const rs_job b = rs_load_job(jobs, j, R, L, N);
    rs_window w;
    w.ok = b.ok && b.s % period == 0;
    w.r = w.ok ? b.r : 0; w.s = w.ok ? b.s : 0;
    w.n_in = w.ok ? (N - b.s < L ? N - b.s : L) : 0;
    w.head = w.ok ? b.head : 0; w.tail0 = L - (w.ok ? b.tail : 0);
    return w;
}

__device__ __forceinline__ float4 rs_ld4(const float* __restrict__ p, bool aligned) {
    return aligned ? *reinterpret_cast<const float4*>(p) : make_float4(p[0], p[1], p[2], p[3]);
}

__device__ __forceinline__ void rs_st4(float* __restrict__ p, bool aligned, float4 v) {
    if (aligned) *reinterpret_cast<float4*>(p) = v;
    else { p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w; }
}

// elements before the first 16-byte boundary of p, at most n
__device__ __forceinline__ int64_t rs_lead(const float* p, int64_t n) {
    const int64_t a = (int64_t)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
    return a > n ? n : a;
}

// a float4 of src is aligned wherever the float4 of dst at the same element is
__device__ __forceinline__ bool rs_aligned_as(const float* src, const float* dst) { return ((((uintptr_t)src) - ((uintptr_t)dst)) & 15u) == 0; }

// The walk over a row of n elements written at dst, by this lane of ``nthreads`` (tid < nthreads; every lane below 4 exists): vec(i) for
// every fourth i of the body, where dst + i is 16-byte aligned, and elem(i) for the fewer than 4 elements before and after it.
template <class Vec, class Elem>
__device__ __forceinline__ void rs_walk(const float* dst, int64_t n, int64_t tid, int64_t nthreads, Vec vec, Elem elem) {
    const int64_t lead = rs_lead(dst, n);
    const int64_t nvec = (n - lead) >> 2, body_end = lead + nvec * 4;
    for (int64_t v = tid; v < nvec; v += nthreads) vec(lead + 4 * v);
    if (tid < lead) elem(tid);
    if (tid < n - body_end) elem(body_end + tid);
}

static inline int rs_tiles(int64_t L) {
    int gx = aid_cdiv(aid_cdiv(L, 4), RS_THREADS);                                   // >= 1 tile; every lane of tile 0 exists for the head / tail (< 4 elements each)
    return gx > 1024 ? 1024 : gx;
}
