// Row helpers shared by the streaming kernels of whole-recording restoration (aid_restore.hip, aid_declip.hip, aid_bwe_long.hip): the job table of
// include/aid_restore.h, float4 access over the 16-byte-aligned body of a row with scalars at its ragged ends, and the tile count.
//
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

__device__ __forceinline__ bool rs_al16(const float* p) { return (((uintptr_t)p) & 15u) == 0; }

static inline int rs_tiles(int64_t L) {
    int gx = aid_cdiv(aid_cdiv(L, 4), RS_THREADS);                                   // >= 1 tile; every lane of tile 0 exists for the head / tail (< 4 elements each)
    return gx > 1024 ? 1024 : gx;
}
