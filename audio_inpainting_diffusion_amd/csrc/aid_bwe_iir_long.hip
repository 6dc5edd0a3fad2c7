// Bandwidth extension of whole recordings through an IIR filter (include/aid_bwe_long.h): the observation operator of a window whose first
// samples SEED the recursion (state -3) and whose other samples are filtered (0), known (> 0), unobserved (-1) or absent (<= -2) -- apply,
// adjoint, the data-consistency projection and the preparation of the observation row -- and the gather that builds the raw rows and states
// of all windows of a pass.
//
//   iir_observed: ONE workgroup of 256 threads per row; nothing but registers and 35 KiB of static LDS (the parameter block has no scratch
//        pointer).  With S = the row's leading run of -3 states (found first, one tile of states in the common case), the recursion runs over
//        the region behind the run: [S, L) forwards for modes 0, 2, 3; [0, L - S) of the reversed row for the adjoint, continued by min(N, S)
//        samples so that the b taps reach into the run.  The region is cut into at most 256 chunks of C samples (C a multiple of 16), one per
//        thread, and the all-pole recursion (fp64) runs the way aid_iir's does, with the state carried in LDS instead of global scratch:
//          sweep 1  every thread but the last runs its chunk from a zero state and keeps the last NP outputs z; beside it, in the same
//                   loop, it runs the input-free recursion from the unit state e_(t % NP): column t of the chunk transition M, which all
//                   chunks share (they are all C long)
//          carry    wave 0: s_(j+1) = M s_j + z_j over the chunks, lane l holding row l of M and s[l]; s_(j+1) replaces z_j in LDS
//          sweep 2  every thread re-runs its chunk from its true incoming state and stores
//        The state of the recursion is the last NP outputs, NP = 4, 8 or 16 >= N = K - 1 with the coefficients zero-padded (exact), so that a
//        block of NP samples is unrolled with static indices: no register shuffling.  Forwards the b taps come first (u = b * xin, read from
//        the row with the NP samples before the chunk), then the poles; the adjoint runs the poles on the gated gradient first and applies
//        the b taps to w, gated at the run (w counts as 0 inside it) -- the two orders differ next to S, and this is the transpose.
//        Deterministic: no atomics but the integer min that finds S.  A thread reads and writes its own contiguous chunk (stride C between
//        lanes): 2 x 4 bytes read per sample and sweep, served from L2 after the first touch of a line; 4 bytes written.
//   iir_gather: grid (tiles, jobs), pure streaming as bwe_gather_kernel: float4 where a float4 of the destination lies wholly inside the
//        filtered part, element by element at the seams (aid_rows.h).  The job table is device memory: every access is bounded here.
#include "aid_rows.h"
#include "aid_bwe_long.h"

#define IO_THREADS 256
#define IO_SEED (-3.f)

__device__ __forceinline__ bool io_absent(float k) { return k <= -2.f && k != IO_SEED; }

// One block of NP samples of the recursion y[j] = v[j] - sum_{k=1..NP} a[k] y[j - k]: prev holds the NP outputs before the block, cur receives
// the block's (in position order).
template <int NP>
__device__ __forceinline__ void io_poles(const double (&a)[17], const double (&v)[NP], const double (&prev)[NP], double (&cur)[NP]) {
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        double acc = v[j];
#pragma unroll
        for (int k = 1; k <= NP; ++k) acc -= a[k] * (j - k >= 0 ? cur[j - k] : prev[NP + j - k]);
        cur[j] = acc;
    }
}

// MODE 0 apply, 1 adjoint, 2 projection, 3 preparation of the observation row
template <int NP, int MODE>
__global__ __launch_bounds__(IO_THREADS) void iir_observed_kernel(const aid_fir_observed_params p) {
    __shared__ double zs[IO_THREADS][NP];           // z of chunk j, then the incoming state of chunk j + 1
    __shared__ double Ms[NP][NP + 1];               // M[r][c]: state element r after C input-free steps from the unit state e_c
    __shared__ int s_run;
    const int t = threadIdx.x;
    const int64_t row = blockIdx.x, L = p.L;
    const int N = p.K - 1;
    const float* __restrict__ x = p.x + row * p.x_ld;
    const float* __restrict__ ks = p.state + row * p.state_ld;
    float* __restrict__ out = p.out + row * p.out_ld;

    double a[17], b[17];
#pragma unroll
    for (int k = 0; k <= NP; ++k) {
        b[k] = k <= N ? (double)p.h[k] : 0.0;
        a[k] = k <= N ? (double)p.h[p.K + k] : 0.0;
    }

    // S: the length of the leading run of seed states
    if (t == 0) s_run = (int)L;
    __syncthreads();
    for (int64_t base = 0; base < L; base += IO_THREADS) {
        const int64_t i = base + t;
        const bool stop = i < L && ks[i] != IO_SEED;
        if (stop) atomicMin(&s_run, (int)i);
        if (__syncthreads_or(stop)) break;
    }
    const int64_t S = s_run;
    const int64_t Lu = L - S;                                                    // the samples behind the run
    const int64_t Le = (MODE == 1 && Lu > 0) ? Lu + (S < N ? S : N) : Lu;        // ... and, for the adjoint, those of the run the b taps reach
    const int64_t C = 16 * (Le > 4096 ? (Le + 4095) / 4096 : 1);
    const int nchunks = (int)((Le + C - 1) / C);                                 // <= 256

    // region coordinate n -> sample i
    auto at = [&](int64_t n) -> int64_t { return MODE == 1 ? L - 1 - n : S + n; };

    // the samples outside the region: the run itself (all of state -3)
    {
        const int64_t fill = MODE == 1 ? L - Le : S;
        for (int64_t i = t; i < fill; i += IO_THREADS) out[i] = MODE == 2 ? x[i] : 0.f;
    }

    // v of one block (nb = its first region coordinate) and, when STORE, what the epilogue needs
    auto load_block = [&](int64_t nb, float (&xv)[NP], float (&kv)[NP]) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int64_t n = nb + j;
            const bool in = n < Le && (MODE == 1 ? n >= 0 : S + n >= 0);         // (forwards the b taps reach back into the run)
            xv[j] = 0.f; kv[j] = -1.f;
            if (in) { const int64_t i = at(n); xv[j] = x[i]; kv[j] = ks[i]; }
        }
    };
    auto feed = [&](float xv, float kv) -> double {           // what a sample feeds into the operator
        if (MODE == 1) return kv == 0.f ? (double)xv : 0.0;    // (the gradient of the filtered samples)
        if (MODE == 3) return 0.0;
        return io_absent(kv) ? 0.0 : (double)xv;
    };

    const int64_t c0 = (int64_t)t * C;
    const bool carry_out = t < nchunks - 1;                    // a full chunk whose outgoing state another chunk needs
    if (nchunks > 1 && (carry_out || t < NP)) {
        // ---- sweep 1: zero-state run of the chunk, and column t % NP of M
        double prev[NP], cur[NP], fprev[NP], fcur[NP], zero[NP], fin_prev[NP], fin_cur[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) { prev[j] = 0.0; fprev[j] = (t % NP) == j ? 1.0 : 0.0; zero[j] = 0.0; fin_prev[j] = 0.0; }
        if (MODE == 0 || MODE == 2) {                          // the inputs before the chunk, for the b taps
            float xv[NP], kv[NP];
            load_block(c0 - NP, xv, kv);
#pragma unroll
            for (int j = 0; j < NP; ++j) fin_prev[j] = feed(xv[j], kv[j]);
        }
        for (int64_t nb = c0; nb < c0 + C; nb += NP) {
            float xv[NP], kv[NP];
            double v[NP];
            load_block(nb, xv, kv);
#pragma unroll
            for (int j = 0; j < NP; ++j) fin_cur[j] = feed(xv[j], kv[j]);
            if (MODE == 0 || MODE == 2) {
#pragma unroll
                for (int j = 0; j < NP; ++j) {
                    double acc = 0.0;
#pragma unroll
                    for (int k = 0; k <= NP; ++k) acc += b[k] * (j - k >= 0 ? fin_cur[j - k] : fin_prev[NP + j - k]);
                    v[j] = acc;
                }
            } else {
#pragma unroll
                for (int j = 0; j < NP; ++j) v[j] = fin_cur[j];
            }
            io_poles<NP>(a, v, prev, cur);
            io_poles<NP>(a, zero, fprev, fcur);
#pragma unroll
            for (int j = 0; j < NP; ++j) { prev[j] = cur[j]; fprev[j] = fcur[j]; fin_prev[j] = fin_cur[j]; }
        }
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            if (carry_out) zs[t][j] = prev[j];
            if (t < NP) Ms[j][t] = fprev[j];
        }
    }
    __syncthreads();

    // ---- the carry: wave 0, lane l < NP holds row l of M and element l of the state
    if (t < 64 && nchunks > 1) {
        const int l = t < NP ? t : 0;
        double Mrow[NP];
#pragma unroll
        for (int m = 0; m < NP; ++m) Mrow[m] = Ms[l][m];
        double s = 0.0;
        if (MODE == 3 && t < NP && S - NP + t >= 0) s = (double)x[S - NP + t];       // (the seed samples are the state the free response starts from)
        for (int j = 0; j < nchunks - 1; ++j) {
            double acc = zs[j][l];
#pragma unroll
            for (int m = 0; m < NP; ++m) acc += Mrow[m] * __shfl(s, m);
            s = acc;
            if (t < NP) zs[j][t] = s;
        }
    }
    __syncthreads();

    // ---- sweep 2: the chunk from its true incoming state, and the epilogue
    if (t < nchunks) {
        double prev[NP], cur[NP], fin_prev[NP], fin_cur[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            fin_prev[j] = 0.0;
            if (t > 0) prev[j] = zs[t - 1][j];
            else prev[j] = (MODE == 3 && S - NP + j >= 0) ? (double)x[S - NP + j] : 0.0;
        }
        if (MODE == 0 || MODE == 2) {
            float xv[NP], kv[NP];
            load_block(c0 - NP, xv, kv);
#pragma unroll
            for (int j = 0; j < NP; ++j) fin_prev[j] = feed(xv[j], kv[j]);
        }
        const int64_t c1 = c0 + C < Le ? c0 + C : Le;
        for (int64_t nb = c0; nb < c1; nb += NP) {
            float xv[NP], kv[NP];
            double v[NP], res[NP];
            load_block(nb, xv, kv);
#pragma unroll
            for (int j = 0; j < NP; ++j) fin_cur[j] = feed(xv[j], kv[j]);
            if (MODE == 0 || MODE == 2) {
#pragma unroll
                for (int j = 0; j < NP; ++j) {
                    double acc = 0.0;
#pragma unroll
                    for (int k = 0; k <= NP; ++k) acc += b[k] * (j - k >= 0 ? fin_cur[j - k] : fin_prev[NP + j - k]);
                    v[j] = acc;
                }
            } else {
#pragma unroll
                for (int j = 0; j < NP; ++j) v[j] = fin_cur[j];
            }
            io_poles<NP>(a, v, prev, cur);
            if (MODE == 1) {
                // a = b taps over w, w counting as 0 inside the run (region coordinates >= Lu) and before the row's end (< 0: the zero state)
                const bool gate = nb + NP > Lu;
#pragma unroll
                for (int j = 0; j < NP; ++j) {
                    double acc = 0.0;
#pragma unroll
                    for (int k = 0; k <= NP; ++k) {
                        const double w = j - k >= 0 ? cur[j - k] : prev[NP + j - k];
                        acc += b[k] * ((gate && nb + j - k >= Lu) ? 0.0 : w);
                    }
                    res[j] = acc;
                }
            } else {
#pragma unroll
                for (int j = 0; j < NP; ++j) res[j] = cur[j];
            }
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const int64_t n = nb + j;
                if (n < c1) {
                    const int64_t i = at(n);
                    const float k = kv[j], xi = xv[j];
                    const bool seed = k == IO_SEED, known = rs_known(k);
                    float o;
                    if (MODE == 0) o = known ? xi : (k == 0.f ? (float)res[j] : 0.f);
                    else if (MODE == 1) o = seed ? (float)res[j] : (rs_absent(k) ? 0.f : (known ? (float)res[j] + xi : (float)res[j]));
                    else if (MODE == 2) {
                        const float yv = p.y[row * p.y_ld + i];
                        o = known ? yv : (k == 0.f ? (yv - (float)res[j]) + xi : xi);
                    } else o = known ? xi : (k == 0.f ? (float)((double)xi - res[j]) : 0.f);
                    out[i] = o;
                }
                prev[j] = cur[j]; fin_prev[j] = fin_cur[j];
            }
        }
    }
}

__global__ __launch_bounds__(RS_THREADS) void iir_gather_kernel(const aid_bwe_gather_params p) {
    const int j = blockIdx.y;
    const int64_t L = p.L;
    const int64_t tid = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x, nthreads = (int64_t)gridDim.x * RS_THREADS;
    const rs_window w = rs_load_window(p.jobs, j, p.R, L, p.N, 1);                   // (an invalid job gathers zeros, all absent)
    const int64_t n_in = w.n_in, head = w.head, tail0 = w.tail0, r = w.r, s = w.s;
    const int64_t seeds = (w.ok && s > 0) ? p.K - 1 : 0;                             // the first ``order`` samples of a window that does not start the recording
    // filtered exactly on [f0, f1), when that is a range
    const int64_t f0 = head > seeds ? head : seeds, f1 = tail0 < n_in ? tail0 : n_in;
    const float* __restrict__ rec = p.rec + r * p.rec_ld + s;                         // (dereferenced at i < n_in only)
    const float* __restrict__ out = p.out + r * p.out_ld + s;
    float* __restrict__ y = p.y + (int64_t)j * L;
    float* __restrict__ k = p.state + (int64_t)j * L;

    auto elem = [&](int64_t i, float& yv, float& kv) {
        const bool in = i < n_in, seed = i < seeds, edge = i < head || i >= tail0;
        kv = in ? (seed ? IO_SEED : (edge ? 1.f : 0.f)) : -2.f;
        yv = in ? ((edge && !seed) ? out[i] : rec[i]) : 0.f;
    };

    const bool k_al = rs_aligned_as(k, y), rec_al = rs_aligned_as(rec, y);
    rs_walk(y, L, tid, nthreads, [&](int64_t i) {
        float4 yv, kv;
        if (i >= f0 && i + 4 <= f1) {                                                // wholly the filtered recording
            kv = make_float4(0.f, 0.f, 0.f, 0.f);
            yv = rs_ld4(rec + i, rec_al);
        } else {
            elem(i, yv.x, kv.x); elem(i + 1, yv.y, kv.y); elem(i + 2, yv.z, kv.z); elem(i + 3, yv.w, kv.w);
        }
        *reinterpret_cast<float4*>(y + i) = yv;
        rs_st4(k + i, k_al, kv);
    }, [&](int64_t i) { elem(i, y[i], k[i]); });
}

template <int NP>
static void iir_observed_launch(const aid_fir_observed_params* p, hipStream_t stream) {
    const dim3 grid(p->B), block(IO_THREADS);
    if (p->mode == 0) hipLaunchKernelGGL((iir_observed_kernel<NP, 0>), grid, block, 0, stream, *p);
    else if (p->mode == 1) hipLaunchKernelGGL((iir_observed_kernel<NP, 1>), grid, block, 0, stream, *p);
    else if (p->mode == 2) hipLaunchKernelGGL((iir_observed_kernel<NP, 2>), grid, block, 0, stream, *p);
    else hipLaunchKernelGGL((iir_observed_kernel<NP, 3>), grid, block, 0, stream, *p);
}

extern "C" int aid_iir_observed(const aid_fir_observed_params* p, void* stream) {
    AID_REQUIRE(p && p->x && p->state && p->h && p->out, "aid_iir_observed: null pointer");
    AID_REQUIRE(p->mode >= 0 && p->mode <= 3, "aid_iir_observed: mode must be 0 (apply), 1 (adjoint), 2 (projection) or 3 (preparation)");
    AID_REQUIRE(p->mode != 2 || (p->y && p->y_ld >= p->L), "aid_iir_observed: the projection needs y with a row stride >= L");
    AID_REQUIRE(p->B > 0 && p->B <= 65535 && p->K >= 2 && p->K <= 17 && p->L > 0 && p->L <= (1 << 20),
                "aid_iir_observed: empty or oversized shape (1 <= B <= 65535, K = order + 1 in [2, 17], 1 <= L <= 2^20)");
    AID_REQUIRE(p->x_ld >= p->L && p->out_ld >= p->L && (p->state_ld == 0 || p->state_ld >= p->L), "aid_iir_observed: a row stride is shorter than L");
    const int N = p->K - 1;
    if (N <= 4) iir_observed_launch<4>(p, (hipStream_t)stream);
    else if (N <= 8) iir_observed_launch<8>(p, (hipStream_t)stream);
    else iir_observed_launch<16>(p, (hipStream_t)stream);
    AID_CHECK_LAUNCH();
    return AID_OK;
}

extern "C" int aid_iir_gather(const aid_bwe_gather_params* p, void* stream) {
    AID_REQUIRE(p && p->rec && p->out && p->y && p->state && p->jobs, "aid_iir_gather: null pointer");
    AID_REQUIRE(p->J > 0 && p->J <= 65535 && p->R > 0 && p->K >= 2 && p->K <= 17 && p->L > 0 && p->N > 0,
                "aid_iir_gather: empty or oversized shape (1 <= J <= 65535, K = order + 1 in [2, 17])");
    AID_REQUIRE(p->rec_ld >= p->N && p->out_ld >= p->N, "aid_iir_gather: a row stride is shorter than N");
    hipLaunchKernelGGL(iir_gather_kernel, dim3(rs_tiles(p->L), p->J), dim3(RS_THREADS), 0, (hipStream_t)stream, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}
