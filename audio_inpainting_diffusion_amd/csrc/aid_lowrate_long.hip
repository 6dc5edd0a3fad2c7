// Bandwidth extension of whole low-sample-rate recordings (include/aid_lowrate_long.h): the observation operator of a window seen
// through the rational-ratio polyphase resampler -- L high-rate entries (known, no direct observation, absent) and Mw low-rate entries
// (observed, unobserved, absent) per row -- and the gather that builds the observations and states of all windows of a pass.
//
//   rate_observed<0>: grid (ceil((L + Mw) / 256), B), one thread per output entry.  A high-rate entry is a select; a low-rate entry that
//        is observed runs the tap loop of resample_poly_kernel (aid_resample.hip) with a select on the sample (an absent one enters as 0).
//   rate_observed<1>: grid (ceil(L / 256), B), one thread per sample: the frame and phase loops of resample_poly_adj_kernel
//        (aid_resample_adj.hip) with a select on the gradient (that of the observed entries only), then the select of the epilogue.
//        No LDS, no atomics, a fixed order.  The table (at most a few hundred KB) and the K-tap neighbourhoods stay in cache; next to
//        the network both are tiny (at 8 x 184184 and 147:100: 165 taps over 125296 outputs per item).
//   lowrate_gather: grid (tiles, jobs), grid-stride over the L + Mw entries of a row, element by element: copies and constants only.
//        The job table is device memory: every access is bounded here.
#include "aid_rows.h"
#include "aid_lowrate_long.h"

#define RO_THREADS 256

// MODE 0 apply, 1 adjoint
template <int MODE>
__global__ __launch_bounds__(RO_THREADS) void rate_observed_kernel(const aid_rate_observed_params p) {
    const int64_t e = (int64_t)blockIdx.x * RO_THREADS + threadIdx.x;
    const int64_t b = blockIdx.y, L = p.L, Mw = p.Mw;
    const int64_t orig = p.orig_freq, nw = p.new_freq;
    const float* __restrict__ x = p.x + b * p.x_ld;
    const float* __restrict__ kh = p.state + b * p.state_ld;            // high-rate states [L]
    const float* __restrict__ kl = kh + L;                              // low-rate states [Mw]
    float* __restrict__ out = p.out + b * p.out_ld;
    if (MODE == 0) {
        if (e >= L + Mw) return;
        if (e < L) {
            out[e] = rs_known(kh[e]) ? x[e] : 0.f;
            return;
        }
        const int64_t n = e - L;
        float acc = 0.f;
        if (kl[n] == 0.f) {
            const int64_t i = n / nw;
            const int j = (int)(n - i * nw);
            const float* __restrict__ k = p.k + (int64_t)j * p.K;
            const int64_t base = i * orig - p.width;
            for (int t = 0; t < p.K; ++t) {
                const int64_t q = base + t;
                if (q >= 0 && q < L) acc += k[t] * (rs_absent(kh[q]) ? 0.f : x[q]);
            }
        }
        out[e] = acc;
    } else {
        const int64_t q = e;
        if (q >= L) return;
        const float kv = kh[q];
        if (rs_absent(kv)) {
            out[q] = 0.f;
            return;
        }
        const float* __restrict__ g = x + L;                            // the gradient of the low-rate entries [Mw]
        const int64_t top = q + p.width;                                // t = top - i*orig
        const int64_t num = top - (p.K - 1);                            // t <= K - 1  <=>  i*orig >= num
        int64_t i_lo = num <= 0 ? 0 : (num + orig - 1) / orig;
        int64_t i_hi = top / orig;                                      // t >= 0
        const int64_t i_last = (Mw - 1) / nw;                           // the last frame that holds a low-rate entry
        if (i_hi > i_last) i_hi = i_last;
        float acc = 0.f;
        for (int64_t i = i_lo; i <= i_hi; ++i) {
            const int t = (int)(top - i * orig);                        // in [0, K) by the bounds of i
            const int64_t n0 = i * nw;                                  // < Mw
            int jl = p.j_lo[t], jh = p.j_hi[t];
            if (jl < 0) jl = 0;
            if (jh > p.new_freq) jh = p.new_freq;
            if (Mw - n0 < jh) jh = (int)(Mw - n0);                      // the last frame is cut by Mw
            const float* __restrict__ k = p.kT + (int64_t)t * nw;
            for (int j = jl; j < jh; ++j) acc += k[j] * (kl[n0 + j] == 0.f ? g[n0 + j] : 0.f);
        }
        out[q] = rs_known(kv) ? acc + x[q] : acc;
    }
}

__global__ __launch_bounds__(RS_THREADS) void lowrate_gather_kernel(const aid_lowrate_gather_params p) {
    const int j = blockIdx.y;
    const int64_t L = p.L, Mw = p.Mw, row = L + Mw;
    const int64_t tid = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x, nthreads = (int64_t)gridDim.x * RS_THREADS;
    const rs_window w = rs_load_window(p.jobs, j, p.R, L, p.N, p.orig_freq);                   // (an invalid job gathers zeros, all absent)
    const int64_t n_in = w.n_in, head = w.head, tail0 = w.tail0, r = w.r, s = w.s;
    const int64_t m0 = (s / p.orig_freq) * p.new_freq;                               // the recording's low-rate sample of entry 0
    const int64_t m_in = w.ok ? (p.M - m0 < 0 ? 0 : (p.M - m0 < Mw ? p.M - m0 : Mw)) : 0;   // n < m_in  <=>  low-rate sample m0 + n exists
    const bool cut_l = s > 0, cut_r = s + L < p.N;                                   // the recording goes on before / after the window
    const float* __restrict__ rec = p.rec + r * p.rec_ld + m0;                        // (dereferenced at n < m_in only)
    const float* __restrict__ out = p.out + r * p.out_ld + s;                         // (dereferenced at i < n_in only)
    float* __restrict__ y = p.y + (int64_t)j * row;
    float* __restrict__ k = p.state + (int64_t)j * row;
    for (int64_t e = tid; e < row; e += nthreads) {
        float yv = 0.f, kv = -2.f;
        if (e < L) {
            if (e < n_in) {
                const bool edge = e < head || e >= tail0;
                kv = edge ? 1.f : -1.f;
                if (edge) yv = out[e];
            }
        } else {
            const int64_t n = e - L;
            if (n < m_in) {
                const int64_t a0 = (n / p.new_freq) * p.orig_freq - p.width;
                const bool un = (cut_l && a0 < 0) || (cut_r && a0 + p.K > L);
                kv = un ? -1.f : 0.f;
                if (!un) yv = rec[n];
            }
        }
        y[e] = yv;
        k[e] = kv;
    }
}

extern "C" int aid_lowrate_long_abi_version(void) { return AID_LOWRATE_LONG_ABI_VERSION; }

extern "C" int aid_rate_observed(const aid_rate_observed_params* p, void* stream) {
    AID_REQUIRE(p && p->x && p->state && p->out, "aid_rate_observed: null pointer");
    AID_REQUIRE(p->mode == 0 || p->mode == 1, "aid_rate_observed: mode must be 0 (apply) or 1 (adjoint)");
    AID_REQUIRE(p->mode == 0 ? p->k != nullptr : (p->kT && p->j_lo && p->j_hi), "aid_rate_observed: null table (mode 0 needs k; mode 1 kT, j_lo and j_hi)");
    AID_REQUIRE(p->orig_freq > 0 && p->new_freq > 0 && p->width >= 0 && p->K == 2 * p->width + p->orig_freq && p->L > 0,
                "aid_rate_observed: bad geometry (K must be 2*width + orig_freq)");
    AID_REQUIRE(p->B > 0 && p->B <= 65535, "aid_rate_observed: empty or oversized batch (1 <= B <= 65535)");
    AID_REQUIRE(p->Mw == (p->L * p->new_freq + p->orig_freq - 1) / p->orig_freq, "aid_rate_observed: Mw must be ceil(new*L/orig)");
    const int64_t row = p->L + p->Mw, n_in = p->mode == 0 ? p->L : row, n_out = p->mode == 0 ? row : p->L;
    AID_REQUIRE(p->x_ld >= n_in && p->out_ld >= n_out && (p->state_ld == 0 || p->state_ld >= row), "aid_rate_observed: a row stride is shorter than its row");
    AID_REQUIRE((n_out + RO_THREADS - 1) / RO_THREADS <= 0x7fffffffLL, "aid_rate_observed: signal too long for one launch");
    const dim3 grid((unsigned)((n_out + RO_THREADS - 1) / RO_THREADS), p->B), block(RO_THREADS);
    if (p->mode == 0) hipLaunchKernelGGL(rate_observed_kernel<0>, grid, block, 0, (hipStream_t)stream, *p);
    else hipLaunchKernelGGL(rate_observed_kernel<1>, grid, block, 0, (hipStream_t)stream, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}

extern "C" int aid_lowrate_gather(const aid_lowrate_gather_params* p, void* stream) {
    AID_REQUIRE(p && p->rec && p->out && p->y && p->state && p->jobs, "aid_lowrate_gather: null pointer");
    AID_REQUIRE(p->J > 0 && p->J <= 65535 && p->R > 0 && p->L > 0 && p->N > 0 && p->M > 0, "aid_lowrate_gather: empty or oversized shape (1 <= J <= 65535)");
    AID_REQUIRE(p->orig_freq > 0 && p->new_freq > 0 && p->width >= 0 && p->K == 2 * p->width + p->orig_freq,
                "aid_lowrate_gather: bad geometry (K must be 2*width + orig_freq)");
    AID_REQUIRE(p->Mw == (p->L * p->new_freq + p->orig_freq - 1) / p->orig_freq, "aid_lowrate_gather: Mw must be ceil(new*L/orig)");
    AID_REQUIRE(p->rec_ld >= p->M && p->out_ld >= p->N, "aid_lowrate_gather: a row stride is shorter than its row");
    hipLaunchKernelGGL(lowrate_gather_kernel, dim3(rs_tiles(p->L + p->Mw), p->J), dim3(RS_THREADS), 0, (hipStream_t)stream, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}
