// Phase retrieval of whole recordings (include/aid_phase_long.h): the observation operator of a window seen through the STFT magnitude
// -- L sample entries (known, no direct observation, absent) and an [F, Tw] magnitude block whose frames are observed, unobserved or
// absent -- and the gather that builds the observations and states of all windows of a pass.
//
//   mag_observed_kernel:        grid B * Tw, one workgroup per (item, frame), the frame body of aid_stft_mag (aid_stft_mag_tile.h) with a
//        select on the sample (an absent one enters as 0).  A frame that is not observed runs no FFT and writes F zeros.  Frame t also
//        writes the sample entries [t*hop, (t+1)*hop) of the row (selects; Tw * hop > L, so every sample has one writer): one launch.
//   mag_observed_vjp_frames_kernel: the same grid; the VJP frame body into the scratch [B, Tw, N].  A frame that is not observed returns at
//        once and leaves its scratch unwritten.
//   mag_observed_ola_kernel:    grid (tiles, B), one lane per sample: the overlap-add gather of aid_stft_mag over the observed frames only
//        (it reads no scratch of another frame), then the select of the epilogue.  No atomics, a fixed order.
//   pr_gather_kernel:           grid (tiles, jobs), grid-stride over the L + F*Tw entries of a row, element by element: copies and constants
//        only.  The job table is device memory: every access is bounded here.
#include "aid_rows.h"
#include "aid_stft_mag_tile.h"
#include "aid_phase_long.h"

struct po_row {                                                    // sample q of the row: 0 at and past L and where it is absent
    const float* __restrict__ x; const float* __restrict__ kh; int64_t L;
    __device__ __forceinline__ float operator()(int64_t q) const { return q < L && !rs_absent(kh[q]) ? x[q] : 0.f; }
};
struct po_observed {                                               // frame t was written to the scratch
    const float* __restrict__ kf;
    __device__ __forceinline__ bool operator()(int64_t t) const { return kf[t] == 0.f; }
};

__global__ __launch_bounds__(STFT_THREADS) void mag_observed_kernel(const aid_stft_mag_observed_params p) {
    const int b = blockIdx.x / p.n_frames, t = blockIdx.x - b * p.n_frames;
    extern __shared__ __attribute__((aligned(16))) float2 po_lds[];
    const int N = p.n_fft, F = (N >> 1) + 1;
    const int64_t L = p.L, s0 = (int64_t)t * p.hop;
    const float* __restrict__ x = p.x + (int64_t)b * p.x_ld;
    const float* __restrict__ kh = p.state + (int64_t)b * p.state_ld;
    float* __restrict__ out = p.out + (int64_t)b * p.out_ld;
    for (int64_t q = s0 + threadIdx.x; q < s0 + p.hop && q < L; q += STFT_THREADS) out[q] = rs_known(kh[q]) ? x[q] : 0.f;
    float* __restrict__ mag = out + L + t;                          // [F, Tw], frames contiguous
    if (kh[L + t] != 0.f) {                                         // (the same for every lane of the workgroup)
        for (int k = threadIdx.x; k < F; k += STFT_THREADS) mag[(int64_t)k * p.n_frames] = 0.f;
        return;
    }
    pm_mag_frame(po_row{x, kh, L}, s0, N, p.window, p.twiddle, po_lds, mag, p.n_frames);
}

__global__ __launch_bounds__(STFT_THREADS) void mag_observed_vjp_frames_kernel(const aid_stft_mag_observed_params p) {
    const int b = blockIdx.x / p.n_frames, t = blockIdx.x - b * p.n_frames;
    extern __shared__ __attribute__((aligned(16))) float2 po_lds[];
    const int N = p.n_fft;
    const int64_t L = p.L;
    const float* __restrict__ kh = p.state + (int64_t)b * p.state_ld;
    if (kh[L + t] != 0.f) return;                                   // (the same for every lane of the workgroup)
    pm_vjp_frame(po_row{p.x + (int64_t)b * p.x_ld, kh, L}, (int64_t)t * p.hop, N, p.window, p.twiddle, po_lds,
                 p.g + (int64_t)b * p.g_ld + L + t, p.n_frames, p.frames + ((int64_t)b * p.n_frames + t) * N);
}

__global__ __launch_bounds__(256) void mag_observed_ola_kernel(const aid_stft_mag_observed_params p) {
    const int b = blockIdx.y, N = p.n_fft;
    const int64_t L = p.L;
    const float* __restrict__ kh = p.state + (int64_t)b * p.state_ld;
    const float* __restrict__ g = p.g + (int64_t)b * p.g_ld;
    const float* __restrict__ fr = p.frames + (int64_t)b * p.n_frames * N;
    float* __restrict__ out = p.out + (int64_t)b * p.out_ld;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < L; q += (int64_t)gridDim.x * 256) {
        const float kv = kh[q];
        if (rs_absent(kv)) {
            out[q] = 0.f;
            continue;
        }
        const float a = pm_ola(po_observed{kh + L}, fr, q, N, p.hop);
        out[q] = rs_known(kv) ? a + g[q] : a;
    }
}

__global__ __launch_bounds__(RS_THREADS) void pr_gather_kernel(const aid_pr_gather_params p) {
    const int j = blockIdx.y;
    const int64_t L = p.L, Tw = p.n_frames, F = (p.n_fft >> 1) + 1, row = L + F * Tw;
    const int64_t tid = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x, nthreads = (int64_t)gridDim.x * RS_THREADS;
    const rs_window w = rs_load_window(p.jobs, j, p.R, L, p.N, p.hop);                   // (an invalid job gathers zeros, all absent)
    const int64_t n_in = w.n_in, head = w.head, tail0 = w.tail0, r = w.r, s = w.s;
    const int64_t t0 = s / p.hop;                                                    // the recording's frame of window frame 0
    const int64_t t_in = w.ok ? (p.T_rec - t0 < 0 ? 0 : (p.T_rec - t0 < Tw ? p.T_rec - t0 : Tw)) : 0;   // f < t_in  <=>  frame t0 + f exists
    const bool cut_r = s + L < p.N;                                                  // the recording goes on after the window
    const float* __restrict__ rec = p.rec + r * p.rec_ld + t0;                        // (dereferenced at f < t_in only)
    const float* __restrict__ out = p.out + r * p.out_ld + s;                         // (dereferenced at i < n_in only)
    float* __restrict__ y = p.y + (int64_t)j * row;
    float* __restrict__ st = p.state + (int64_t)j * (L + Tw);
    for (int64_t e = tid; e < row; e += nthreads) {
        float yv = 0.f, kv = -2.f;
        if (e < L) {
            if (e < n_in) {
                const bool edge = e < head || e >= tail0;
                kv = edge ? 1.f : -1.f;
                if (edge) yv = out[e];
            }
            st[e] = kv;
        } else {
            const int64_t k = (e - L) / Tw, f = (e - L) - k * Tw;
            if (f < t_in) {
                const bool un = cut_r && f * p.hop + p.n_fft > L;
                kv = un ? -1.f : 0.f;
                if (!un) yv = rec[k * p.rec_bin_ld + f];
            }
            if (k == 0) st[L + f] = kv;
        }
        y[e] = yv;
    }
}

extern "C" int aid_phase_long_abi_version(void) { return AID_PHASE_LONG_ABI_VERSION; }

extern "C" int aid_stft_mag_observed(const aid_stft_mag_observed_params* p, void* stream) {
    AID_REQUIRE(p && p->x && p->state && p->out && p->window && p->twiddle, "aid_stft_mag_observed: null pointer");
    AID_REQUIRE(p->mode == 0 || p->mode == 1, "aid_stft_mag_observed: mode must be 0 (apply) or 1 (VJP)");
    AID_REQUIRE(p->mode == 0 || (p->g && p->frames), "aid_stft_mag_observed: the VJP needs g and the frame scratch");
    AID_REQUIRE(p->n_fft >= 16 && p->n_fft <= 8192 && (p->n_fft & (p->n_fft - 1)) == 0, "aid_stft_mag_observed: n_fft must be a power of two in [16, 8192]");
    AID_REQUIRE(p->hop > 0 && p->hop <= p->n_fft, "aid_stft_mag_observed: hop must be in [1, n_fft]");
    AID_REQUIRE(p->B > 0 && p->B <= 65535 && p->L > 0, "aid_stft_mag_observed: empty signal, or empty or oversized batch (1 <= B <= 65535)");
    AID_REQUIRE(p->n_frames == 1 + p->L / p->hop, "aid_stft_mag_observed: n_frames must be 1 + L / hop");
    AID_REQUIRE((int64_t)p->B * p->n_frames <= 0x7fffffff, "aid_stft_mag_observed: too many frames");
    const int64_t F = (p->n_fft >> 1) + 1, row = p->L + F * p->n_frames;
    AID_REQUIRE(p->x_ld >= p->L && (p->state_ld == 0 || p->state_ld >= p->L + p->n_frames) && p->out_ld >= (p->mode == 0 ? row : p->L)
                && (p->mode == 0 || p->g_ld >= row), "aid_stft_mag_observed: a row stride is shorter than its row");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)p->n_fft * 2 * sizeof(float2);
    if (p->mode == 0) {
        hipLaunchKernelGGL(mag_observed_kernel, dim3(p->B * p->n_frames), dim3(STFT_THREADS), lds, st, *p);
        AID_CHECK_LAUNCH();
        return AID_OK;
    }
    hipLaunchKernelGGL(mag_observed_vjp_frames_kernel, dim3(p->B * p->n_frames), dim3(STFT_THREADS), lds, st, *p);
    AID_CHECK_LAUNCH();
    int gx = aid_cdiv(p->L, 256); if (gx > 2048) gx = 2048;
    hipLaunchKernelGGL(mag_observed_ola_kernel, dim3(gx, p->B), dim3(256), 0, st, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}

extern "C" int aid_pr_gather(const aid_pr_gather_params* p, void* stream) {
    AID_REQUIRE(p && p->rec && p->out && p->y && p->state && p->jobs, "aid_pr_gather: null pointer");
    AID_REQUIRE(p->J > 0 && p->J <= 65535 && p->R > 0 && p->L > 0 && p->N > 0, "aid_pr_gather: empty or oversized shape (1 <= J <= 65535)");
    AID_REQUIRE(p->n_fft >= 16 && p->n_fft <= 8192 && (p->n_fft & (p->n_fft - 1)) == 0, "aid_pr_gather: n_fft must be a power of two in [16, 8192]");
    AID_REQUIRE(p->hop > 0 && p->hop <= p->n_fft, "aid_pr_gather: hop must be in [1, n_fft]");
    AID_REQUIRE(p->n_frames == 1 + p->L / p->hop && p->T_rec == 1 + p->N / p->hop, "aid_pr_gather: n_frames must be 1 + L / hop and T_rec 1 + N / hop");
    const int64_t F = (p->n_fft >> 1) + 1;
    AID_REQUIRE(p->rec_bin_ld >= p->T_rec && p->rec_ld >= (F - 1) * p->rec_bin_ld + p->T_rec && p->out_ld >= p->N,
                "aid_pr_gather: a stride is shorter than what it steps over");
    hipLaunchKernelGGL(pr_gather_kernel, dim3(rs_tiles(p->L + F * p->n_frames), p->J), dim3(RS_THREADS), 0, (hipStream_t)stream, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}
