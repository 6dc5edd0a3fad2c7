// Spectrogram inpainting of whole recordings (include/aid_spec_long.h): the observation operator of a window seen through the
// STFT-domain masking operator -- L samples that are observed (state 0), known (> 0), unobserved (-1) or absent (<= -2) and Tw window
// frames that are computable (0) or not -- in its three modes, and the gather that builds the observations, states and items of all
// windows of a pass.  Positions are in recording coordinates: window frame j is recording frame s / hop + j.
//
//   mask_observed_frames_kernel: grid B * Tw, one workgroup per (item, window frame), the frame body of aid_stft_frames
//        (aid_stft_tile.h).  A frame whose state is not 0 (or whose item is invalid) returns before any LDS traffic: the branch is the
//        same for every lane of the workgroup and sits ahead of every barrier; its scratch stays unwritten.  A computable frame reads the
//        window through the recording's reflection rule (forward) or plainly, times 1/env, where the sample is observed (adjoint), and
//        multiplies by column s / hop + j of the recording's own mask, read in place.
//   mask_observed_ola_kernel:    grid (tiles, B), one lane per sample: the overlap-add gather of aid_stft_ola over the computable frames
//        only (it reads no scratch of another frame), 1/env of the recording at s + i, then the select of the mode.  No atomics, a
//        fixed order.
//   spec_gather_kernel:          grid (tiles, jobs), grid-stride over the L + Tw entries of a state row, element by element: copies and
//        constants only.  The job table is device memory: every access is bounded here.
#include "aid_rows.h"
#include "aid_stft_tile.h"
#include "aid_spec_long.h"

// Frame t in [0, T_rec) of a recording of N samples padded to Np is computable in the window [s, s + L): the positions it reads are
// [a, a + n_fft), a = t*hop - half; folded at 0 they are [max(a, 0), max(a + n_fft - 1, -a)], folded at Np (a < Np) the part at and
// past Np lands on [2 (Np - 1) - hi, Np - 2], next to the part below Np: one range again.  What of it lies below N must lie in the window.
__device__ __forceinline__ bool so_computable(int64_t t, int64_t s, int64_t L, int64_t N, int64_t Np, int n_fft, int hop) {
    const int64_t a = t * hop - (n_fft >> 1), b = a + n_fft - 1;
    int64_t lo = a < 0 ? 0 : a, hi = b > -a ? b : -a;
    if (hi >= Np) {
        const int64_t m = 2 * (Np - 1) - hi;
        lo = m < lo ? m : lo;
        hi = Np - 1;
    }
    if (hi > N - 1) hi = N - 1;
    return lo > hi || (lo >= s && hi < s + L);
}

struct so_item { int64_t r, s, N, t0; bool ok; };

__device__ __forceinline__ so_item so_load_item(const aid_stft_mask_observed_params& p, int b) {
    const int64_t* t = p.items + (int64_t)b * AID_SPEC_ITEM_FIELDS;
    so_item it;
    it.r = t[0]; it.s = t[1]; it.N = t[2];
    it.ok = it.s >= 0 && it.s % p.hop == 0 && it.N >= 1 && it.N < p.Np && it.N >= p.Np - p.n_fft && it.s < it.N
            && (p.mask_sB == 0 || (it.r >= 0 && it.r < p.Rm));
    if (p.mask_sB == 0 || !it.ok) it.r = 0;
    if (!it.ok) { it.s = 0; it.N = 0; }
    it.t0 = it.s / p.hop;
    return it;
}

struct so_computed {                                               // window frame j was written to the scratch
    const float* __restrict__ kf; bool ok;
    __device__ __forceinline__ bool operator()(int64_t j) const { return ok && kf[j] == 0.f; }
};

template <bool ADJ>
__global__ __launch_bounds__(STFT_THREADS) void mask_observed_frames_kernel(const aid_stft_mask_observed_params p) {
    const int b = blockIdx.x / p.n_frames, j = blockIdx.x - b * p.n_frames;
    const int64_t L = p.L;
    const float* __restrict__ kh = p.state + (int64_t)b * p.state_ld;
    if (kh[L + j] != 0.f) return;                                   // (the same for every lane of the workgroup)
    const so_item it = so_load_item(p, b);
    const int64_t t = it.t0 + j, T_rec = 1 + p.Np / p.hop;
    if (!it.ok || t >= T_rec) return;                               // (likewise)
    extern __shared__ __attribute__((aligned(16))) float2 so_lds[];
    const int N = p.n_fft;
    const float* __restrict__ x = p.x + (int64_t)b * p.x_ld;
    const int64_t start = t * p.hop - (N >> 1);
    auto load = [&](int e) {
        int64_t q = start + e;
        if (ADJ) {
            if (q < 0 || q >= it.N) return 0.f;                     // R'_t: nothing outside the (trimmed) istft support
        } else {
            if (q < 0) q = -q;                                      // R_t: the recording's reflection rule
            if (q >= p.Np) q = 2 * (p.Np - 1) - q;
            if (q >= it.N) return 0.f;
        }
        const int64_t i = q - it.s;
        if (i < 0 || i >= L) return 0.f;                            // (a computable frame never gets here)
        const float kv = kh[i];
        if (ADJ) {
            float v = 0.f;
            if (kv == 0.f) {
                v = x[i];
                v *= p.inv_env[q];
            }
            return v;
        }
        return rs_absent(kv) ? 0.f : x[i];
    };
    st_mask_frame(load, N, p.window, p.twiddle, p.mask + it.r * p.mask_sB + t, p.mask_ld, so_lds, so_lds + N,
                  p.frames + ((int64_t)b * p.n_frames + j) * N);
}

// MODE 0 apply, 1 adjoint, 2 projection
template <int MODE>
__global__ __launch_bounds__(256) void mask_observed_ola_kernel(const aid_stft_mask_observed_params p) {
    const int b = blockIdx.y, N = p.n_fft, half = N >> 1;
    const int64_t L = p.L, Tw = p.n_frames, T_rec = 1 + p.Np / p.hop;
    const so_item it = so_load_item(p, b);
    const float* __restrict__ kh = p.state + (int64_t)b * p.state_ld;
    const float* __restrict__ x = p.x + (int64_t)b * p.x_ld;
    const float* __restrict__ fr = p.frames + (int64_t)b * Tw * N;
    float* __restrict__ out = p.out + (int64_t)b * p.out_ld;
    const so_computed use{kh + L, it.ok};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < L; i += (int64_t)gridDim.x * 256) {
        const float kv = kh[i], xv = x[i];
        const int64_t n = it.s + i;
        const bool in = it.ok && n < it.N;
        float v;
        if (MODE == 1) {
            float a = 0.f;
            if (in) {
                a = st_cover(use, fr, n, N, p.hop, T_rec, it.t0, Tw);
                if (n >= 1 && n <= half) a += st_cover(use, fr, -n, N, p.hop, T_rec, it.t0, Tw);           // left reflection
                const int64_t r = 2 * (p.Np - 1) - n;
                if (r >= p.Np && r < p.Np + half) a += st_cover(use, fr, r, N, p.hop, T_rec, it.t0, Tw);   // right reflection
            }
            v = rs_absent(kv) ? 0.f : (rs_known(kv) ? a + xv : a);
        } else {
            float c = 0.f;
            if (kv == 0.f && in) c = __fmul_rn(st_cover(use, fr, n, N, p.hop, T_rec, it.t0, Tw), p.inv_env[n]);
            if (MODE == 0) v = rs_known(kv) ? xv : (kv == 0.f ? c : 0.f);
            else {
                const float yv = p.y[(int64_t)b * p.y_ld + i];
                v = rs_known(kv) ? yv : (kv == 0.f ? __fadd_rn(__fadd_rn(-c, yv), xv) : xv);
            }
        }
        out[i] = v;
    }
}

__global__ __launch_bounds__(RS_THREADS) void spec_gather_kernel(const aid_spec_gather_params p) {
    const int j = blockIdx.y;
    const int64_t L = p.L, Tw = p.n_frames, row = L + Tw, T_rec = 1 + p.Np / p.hop;
    const int half = p.n_fft >> 1;
    const int64_t tid = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x, nthreads = (int64_t)gridDim.x * RS_THREADS;
    const rs_window w = rs_load_window(p.jobs, j, p.R, L, p.N, p.hop);                   // (an invalid job gathers zeros, all absent)
    const int64_t n_in = w.n_in, head = w.head, tail0 = w.tail0, r = w.r, s = w.s;
    const int64_t t0 = s / p.hop;
    const float* __restrict__ rec = p.rec + r * p.rec_ld + s;                         // (dereferenced at i < n_in only)
    const float* __restrict__ out = p.out + r * p.out_ld + s;
    float* __restrict__ y = p.y + (int64_t)j * L;
    float* __restrict__ st = p.state + (int64_t)j * row;
    if (tid == 0) {
        int64_t* it = p.items + (int64_t)j * AID_SPEC_ITEM_FIELDS;
        it[0] = w.ok ? r : -1; it[1] = w.ok ? s : -1; it[2] = w.ok ? p.N : 0;
    }
    for (int64_t e = tid; e < row; e += nthreads) {
        float kv = -2.f;
        if (e < L) {
            float yv = 0.f;
            if (e < n_in) {
                if (e < head || e >= tail0) {
                    kv = 1.f;
                    yv = out[e];
                } else {
                    // the frames of the recording that cover q = s + e
                    const int64_t q = s + e + half;
                    int64_t t1 = q / p.hop, ta = q - (p.n_fft - 1) < 0 ? 0 : (q - (p.n_fft - 1) + p.hop - 1) / p.hop;
                    if (t1 > T_rec - 1) t1 = T_rec - 1;
                    bool all = true;
                    for (int64_t t = ta; t <= t1; ++t) all = all && so_computable(t, s, L, p.N, p.Np, p.n_fft, p.hop);
                    kv = all ? 0.f : -1.f;
                    if (all) yv = rec[e];
                }
            }
            y[e] = yv;
        } else if (w.ok) {
            const int64_t t = t0 + (e - L);
            if (t < T_rec) kv = so_computable(t, s, L, p.N, p.Np, p.n_fft, p.hop) ? 0.f : -1.f;
        }
        st[e] = kv;
    }
}

extern "C" int aid_spec_long_abi_version(void) { return AID_SPEC_LONG_ABI_VERSION; }

static int spec_sizes_check(int n_fft, int hop, int64_t L, int64_t Np, int n_frames, const char* msg) {
    AID_REQUIRE(n_fft >= 16 && n_fft <= 8192 && (n_fft & (n_fft - 1)) == 0 && hop > 0 && n_fft % hop == 0 && L > 0 && Np >= n_fft && Np % n_fft == 0
                && n_frames == 1 + (L + n_fft) / hop, msg);
    return AID_OK;
}

extern "C" int aid_stft_mask_observed(const aid_stft_mask_observed_params* p, void* stream) {
    AID_REQUIRE(p && p->x && p->state && p->items && p->window && p->twiddle && p->inv_env && p->mask && p->frames && p->out,
                "aid_stft_mask_observed: null pointer");
    AID_REQUIRE(p->mode >= 0 && p->mode <= 2, "aid_stft_mask_observed: mode must be 0 (apply), 1 (adjoint) or 2 (projection)");
    AID_REQUIRE(p->mode != 2 || (p->y && p->y_ld >= p->L), "aid_stft_mask_observed: the projection needs y with a row stride >= L");
    int rc = spec_sizes_check(p->n_fft, p->hop, p->L, p->Np, p->n_frames,
                              "aid_stft_mask_observed: n_fft must be a power of two in [16, 8192], hop must divide it, Np must be a multiple of "
                              "n_fft and n_frames 1 + (L + n_fft) / hop");
    if (rc) return rc;
    AID_REQUIRE(p->B > 0 && p->B <= 65535 && p->Rm > 0, "aid_stft_mask_observed: empty or oversized batch (1 <= B <= 65535), or no mask");
    AID_REQUIRE((int64_t)p->B * p->n_frames <= 0x7fffffff, "aid_stft_mask_observed: too many frames");
    const int64_t F = (p->n_fft >> 1) + 1, T_rec = 1 + p->Np / p->hop;
    AID_REQUIRE(p->x_ld >= p->L && p->out_ld >= p->L && p->state_ld >= p->L + p->n_frames, "aid_stft_mask_observed: a row stride is shorter than its row");
    AID_REQUIRE(p->mask_ld >= T_rec && (p->mask_sB == 0 || p->mask_sB >= (F - 1) * p->mask_ld + T_rec),
                "aid_stft_mask_observed: a mask stride is shorter than what it steps over");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)p->n_fft * 2 * sizeof(float2);
    const dim3 fgrid(p->B * p->n_frames), fblock(STFT_THREADS);
    if (p->mode == 1) hipLaunchKernelGGL(mask_observed_frames_kernel<true>, fgrid, fblock, lds, st, *p);
    else hipLaunchKernelGGL(mask_observed_frames_kernel<false>, fgrid, fblock, lds, st, *p);
    AID_CHECK_LAUNCH();
    int gx = aid_cdiv(p->L, 256); if (gx > 2048) gx = 2048;
    const dim3 ogrid(gx, p->B), oblock(256);
    if (p->mode == 0) hipLaunchKernelGGL(mask_observed_ola_kernel<0>, ogrid, oblock, 0, st, *p);
    else if (p->mode == 1) hipLaunchKernelGGL(mask_observed_ola_kernel<1>, ogrid, oblock, 0, st, *p);
    else hipLaunchKernelGGL(mask_observed_ola_kernel<2>, ogrid, oblock, 0, st, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}

extern "C" int aid_spec_gather(const aid_spec_gather_params* p, void* stream) {
    AID_REQUIRE(p && p->rec && p->out && p->y && p->state && p->items && p->jobs, "aid_spec_gather: null pointer");
    AID_REQUIRE(p->J > 0 && p->J <= 65535 && p->R > 0 && p->N > 0, "aid_spec_gather: empty or oversized shape (1 <= J <= 65535)");
    int rc = spec_sizes_check(p->n_fft, p->hop, p->L, p->Np, p->n_frames,
                              "aid_spec_gather: n_fft must be a power of two in [16, 8192], hop must divide it, Np must be a multiple of n_fft and "
                              "n_frames 1 + (L + n_fft) / hop");
    if (rc) return rc;
    AID_REQUIRE(p->Np == p->N + (p->n_fft - p->N % p->n_fft), "aid_spec_gather: Np must be N + (n_fft - N % n_fft)");
    AID_REQUIRE(p->rec_ld >= p->N && p->out_ld >= p->N, "aid_spec_gather: a row stride is shorter than N");
    hipLaunchKernelGGL(spec_gather_kernel, dim3(rs_tiles(p->L + p->n_frames), p->J), dim3(RS_THREADS), 0, (hipStream_t)stream, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}
