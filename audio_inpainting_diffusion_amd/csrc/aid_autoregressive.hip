// Window carry of autoregressive generation (include/aid_autoregressive.h): between two windows ONE launch writes the next
// window's observations (the tail of the window just sampled, zeros after it) and appends the new part of that window to
// the result.  HBM-trivial: B * (2L - skip) floats written, as many read.
//
//   grid (tiles, B, jobs): job 0 fills y, job 1 appends to out (only job 1 when y is null).  A row is copied with float4
//   stores over the 16-byte-aligned body of the DESTINATION and scalar stores over its head (< 4 elements) and tail; the
//   source is read as float4 where it is aligned at the same element and as four scalars otherwise.
#include "aid_common.h"
#include "aid_autoregressive.h"

#define AR_THREADS 256

// dst[i] = i < ncopy ? src[i] : 0  for i < n   (tid / nthreads: this lane's index and the lane count over the row)
__device__ __forceinline__ void ar_copy_row(float* __restrict__ dst, const float* __restrict__ src, int64_t ncopy, int64_t n,
                                            int64_t tid, int64_t nthreads) {
    int64_t head = (int64_t)(((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u) >> 2);
    if (head > n) head = n;
    const int64_t nvec = (n - head) >> 2;
    const int64_t tail0 = head + nvec * 4;
    const bool src_aligned = (((uintptr_t)(src + head)) & 15u) == 0;
    for (int64_t v = tid; v < nvec; v += nthreads) {
        const int64_t i = head + 4 * v;
        float4 r;
        if (i + 4 <= ncopy) {
            if (src_aligned) r = *reinterpret_cast<const float4*>(src + i);
            else r = make_float4(src[i], src[i + 1], src[i + 2], src[i + 3]);
        } else {
            r.x = i < ncopy ? src[i] : 0.f;
            r.y = i + 1 < ncopy ? src[i + 1] : 0.f;
            r.z = i + 2 < ncopy ? src[i + 2] : 0.f;
            r.w = i + 3 < ncopy ? src[i + 3] : 0.f;
        }
        *reinterpret_cast<float4*>(dst + i) = r;
    }
    if (tid < head) dst[tid] = tid < ncopy ? src[tid] : 0.f;
    if (tid < n - tail0) { const int64_t i = tail0 + tid; dst[i] = i < ncopy ? src[i] : 0.f; }
}

__global__ __launch_bounds__(AR_THREADS) void ar_carry_kernel(const aid_ar_carry_params p) {
    const int b = blockIdx.y;
    const int job = p.y ? (int)blockIdx.z : 1;
    const int64_t tid = (int64_t)blockIdx.x * AR_THREADS + threadIdx.x, nthreads = (int64_t)gridDim.x * AR_THREADS;
    const float* x = p.x + (int64_t)b * p.L;
    if (job == 0) {
        ar_copy_row(p.y + (int64_t)b * p.L, x + (p.L - p.end), p.end, p.L, tid, nthreads);
    } else {
        const int64_t skip = p.first ? 0 : p.end;
        ar_copy_row(p.out + (int64_t)b * p.out_ld + p.off, x + skip, p.L - skip, p.L - skip, tid, nthreads);
    }
}

extern "C" int aid_ar_abi_version(void) { return AID_AR_ABI_VERSION; }

extern "C" int aid_ar_carry(const aid_ar_carry_params* p, void* stream) {
    AID_REQUIRE(p && p->x && p->out, "aid_ar_carry: null pointer");
    AID_REQUIRE(p->B > 0 && p->B <= 65535 && p->L > 1, "aid_ar_carry: empty or oversized shape");
    AID_REQUIRE(p->end >= 1 && p->end < p->L, "aid_ar_carry: 1 <= end < L");
    const int64_t n_new = p->L - (p->first ? 0 : p->end);
    AID_REQUIRE(p->off >= 0 && p->off + n_new <= p->out_ld, "aid_ar_carry: the appended part must lie inside a row of out (off + L - skip <= out_ld)");
    int gx = aid_cdiv(aid_cdiv(p->L, 4), AR_THREADS); if (gx > 1024) gx = 1024;   // >= 1 tile; every lane of tile 0 exists for the head / tail (< 4 elements each)
    hipLaunchKernelGGL(ar_carry_kernel, dim3(gx, p->B, p->y ? 2 : 1), dim3(AR_THREADS), 0, (hipStream_t)stream, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}
