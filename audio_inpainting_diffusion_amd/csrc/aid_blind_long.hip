// Blind bandwidth extension of whole recordings (blind_long.py): one fitted low-pass per recording.  Declared in include/aid_bwe_long.h
// (aid_window_energy, on the parameter block of aid_bwe_gather) and include/aid_phase.h (aid_lowpass_fit_groups, on that of aid_lowpass_fit).
//
//   window_energy_kernel      : one workgroup of 256 lanes per job (recording, window start) of a job table.  A lane adds the squares of the
//                               samples i = lane, lane + 256, ... of the window in fp64, ascending; the 256 partial sums are added as a binary
//                               tree in LDS.  A fixed order, no atomics.  Samples from N on do not exist; an invalid job has energy 0.
//   lowpass_fit_groups_kernel : one workgroup of 1024 lanes per item b.  The statistics of the items of b's group are added in fp64, in
//                               ascending item order, into the two tables Ek of the fit's LDS (free until the candidate loop); then the
//                               fit and the tap design of aid_lowpass_fit.h read them there.  Every item of a group does the same sums in
//                               the same order: the same bits.  The group ids come in host memory: the launcher checks them and hands them
//                               to the kernel with its arguments.
#include "aid_common.h"
#include "aid_lowpass_fit.h"
#include "aid_restore.h"
#include "aid_phase.h"
#include "aid_bwe_long.h"

#define WE_THREADS 256

__global__ __launch_bounds__(WE_THREADS) void window_energy_kernel(const aid_bwe_gather_params p) {
    __shared__ double part[WE_THREADS];
    const int j = blockIdx.x, t = threadIdx.x;
    const int64_t r = p.jobs[(int64_t)j * AID_RESTORE_JOB_FIELDS], s = p.jobs[(int64_t)j * AID_RESTORE_JOB_FIELDS + 1];
    const bool valid = r >= 0 && r < p.R && s >= 0 && s < p.N;                  // (uniform over the workgroup)
    const int64_t n = valid ? min(p.L, p.N - s) : 0;                           // the samples of the window that exist
    const float* __restrict__ y = p.rec + (valid ? r * p.rec_ld + s : 0);
    double a = 0.0;
    for (int64_t i = t; i < n; i += WE_THREADS) {
        const double v = (double)y[i];
        a = fma(v, v, a);
    }
    part[t] = a;
    __syncthreads();
#pragma unroll
    for (int o = WE_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) part[t] += part[t + o];
        __syncthreads();
    }
    if (t == 0) ((double*)p.y)[j] = part[0];
}

extern "C" int aid_window_energy(const aid_bwe_gather_params* p, void* stream) {
    AID_REQUIRE(p && p->rec && p->y && p->jobs, "aid_window_energy: null pointer");
    AID_REQUIRE(p->J > 0 && p->R > 0 && p->L > 0 && p->N > 0, "aid_window_energy: empty shape (J, R, L, N >= 1)");
    AID_REQUIRE(p->rec_ld >= p->N, "aid_window_energy: the row stride is shorter than N");
    AID_REQUIRE(((uintptr_t)p->y & 7) == 0, "aid_window_energy: the energies are doubles: y must be 8-byte aligned");
    hipLaunchKernelGGL(window_energy_kernel, dim3(p->J), dim3(WE_THREADS), 0, (hipStream_t)stream, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}

struct lf_groups_args {                                          // the kernel's arguments: the caller's block and the checked group ids
    aid_matrix_norm_params p;
    int group[AID_LOWPASS_FIT_MAX_ITEMS];
};

__global__ __launch_bounds__(LF_THREADS) void lowpass_fit_groups_kernel(const lf_groups_args a) {
    __shared__ lf_lds lds;
    const aid_matrix_norm_params& p = a.p;
    const int b = blockIdx.x, F = p.F, g = a.group[b];
    for (int k = threadIdx.x; k < F; k += LF_THREADS) {
        double sxx = 0.0, sxy = 0.0;
        for (int o = 0; o < p.B; ++o) {
            if (a.group[o] != g) continue;
            const float* __restrict__ st = p.den + (int64_t)o * 2 * F;
            sxx += (double)st[k];
            sxy += (double)st[F + k];
        }
        lds.Ek[0][k] = sxx;
        lds.Ek[1][k] = sxy;
    }
    __syncthreads();
    const double (*S)[LF_MAX_F] = lds.Ek;
    lf_fit_and_design(lds, [&](int s, int k) { return S[s][k]; }, F, p.T, p.ord, p.max_iter, p.y, p.tol, p.r,
                      p.norm + (int64_t)b * 4, p.g + (int64_t)b * p.max_iter);
}

extern "C" int aid_lowpass_fit_groups(const aid_matrix_norm_params* p, void* stream) {
    AID_REQUIRE(p && p->den && p->y && p->r && p->g && p->norm && p->diag, "aid_lowpass_fit_groups: null pointer");
    AID_REQUIRE(p->B > 0 && p->B <= AID_LOWPASS_FIT_MAX_ITEMS, "aid_lowpass_fit_groups: 1 <= B <= AID_LOWPASS_FIT_MAX_ITEMS items");
    lf_groups_args a;
    a.p = *p;
    const int* group = (const int*)p->diag;                       // (host memory: see include/aid_phase.h)
    for (int b = 0; b < AID_LOWPASS_FIT_MAX_ITEMS; ++b) a.group[b] = b < p->B ? group[b] : 0;
    for (int b = 0; b < p->B; ++b)
        AID_REQUIRE(a.group[b] >= 0 && a.group[b] < p->B, "aid_lowpass_fit_groups: a group id outside [0, B)");
    const int N = 2 * (p->F - 1);
    AID_REQUIRE(p->F <= LF_MAX_F && N >= 16 && (N & (N - 1)) == 0, "aid_lowpass_fit_groups: F must be n_fft / 2 + 1 for a power of two n_fft in [16, 2048]");
    AID_REQUIRE(p->T >= 1 && p->ord >= 1 && (int64_t)p->T * p->ord < 0x7fffffff, "aid_lowpass_fit_groups: the candidate tables must hold 1 <= NC, NA and NC * NA < 2^31");
    AID_REQUIRE(p->max_iter >= 1 && (p->max_iter & 1) && p->max_iter <= N - 1, "aid_lowpass_fit_groups: K must be odd and in [1, n_fft - 1]");
    AID_REQUIRE(p->tol >= 0.0, "aid_lowpass_fit_groups: eps must be >= 0");
    hipLaunchKernelGGL(lowpass_fit_groups_kernel, dim3(p->B), dim3(LF_THREADS), 0, (hipStream_t)stream, a);
    AID_CHECK_LAUNCH();
    return AID_OK;
}
