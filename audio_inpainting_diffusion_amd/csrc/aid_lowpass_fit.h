// The fit and the tap design of blind bandwidth extension (blind.py), shared by lowpass_fit_kernel (aid_blind_bwe.hip: the statistics of one
// item) and lowpass_fit_groups_kernel (aid_blind_long.hip: the statistics of a group of items, summed in fp64).  One workgroup of LF_THREADS
// lanes per item, all in fp64.  ``load(s, k)`` hands out statistic s (0: Sxx, 1: Sxy) of bin k as a double; it is called in the first two
// sweeps only, before the tables Ek are written, so a loader may read its numbers from lf_lds::Ek.
//
// g_k and the valid bins -> LDS; the pass band left of a cut-off and the stop band at the floor are prefix / suffix sums, so a candidate
// (c_j, A_i) costs only the bins of its transition: H = k^(A s) / c^(A s), s = log2(10) / 20, with k^(A s) tabulated once per slope.  The two
// halves of the workgroup take two slopes at a time; a lane takes a low and a high cut-off (a long and a short transition); the arg-min
// carries (cost, j * NA + i) and breaks ties by the lower index.  Then H on the grid and the taps by frequency sampling, cosines from a
// quarter-wave-exact table of N/2 + 1 entries.
#ifndef AID_LOWPASS_FIT_H
#define AID_LOWPASS_FIT_H

#include "aid_common.h"

#define LF_THREADS 1024
#define LF_WAVES (LF_THREADS / AID_WAVE)
#define LF_MAX_F 1025                     // n_fft <= 2048: five fp64 tables of F entries in static LDS

struct lf_lds {
    double gk[LF_MAX_F];                  // g_k, -1 where the bin is not valid
    double Ek[2][LF_MAX_F];               // k^(A s) of the two slopes in hand; [0]: H_k of the winner at the end
    double P1[LF_MAX_F + 1];              // P1[m] = sum over the valid k < m of (1 - g_k)^2; the cosine table at the end
    double S3[LF_MAX_F + 1];              // S3[m] = sum over the valid k >= m of (gmin - g_k)^2
    double redv[LF_WAVES];
    int redi[LF_WAVES];
};

__device__ __forceinline__ double lf_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// cand = [NC cut-offs | NA slopes | floor_dB, k_lo], w = tap window [K]; writes fit[0..4) and taps[0..K) of the item
template <class Load>
__device__ __forceinline__ void lf_fit_and_design(lf_lds& m, Load load, int F, int NC, int NA, int K, const float* __restrict__ cand, double tol,
                                                  const float* __restrict__ w, float* __restrict__ fit, float* __restrict__ taps) {
    double* gk = m.gk;
    double* P1 = m.P1;
    double* S3 = m.S3;
    double* redv = m.redv;
    int* redi = m.redi;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = 2 * (F - 1);
    const float* __restrict__ cc = cand;
    const float* __restrict__ ca = cc + NC;
    const double floor_dB = (double)ca[NA], s20 = 0.16609640474436813;       // log2(10) / 20
    const double gmin = exp2(floor_dB * s20);
    const int k_lo = (int)fminf(fmaxf(ca[NA + 1], 0.f), (float)F);

    // the largest Sxx, then g_k and the valid bins
    double mx = 0.0;
    for (int k = tid; k < F; k += LF_THREADS) mx = fmax(mx, load(0, k));
    mx = lf_wave_max(mx);
    if (lane == 0) redv[wave] = mx;
    __syncthreads();
    mx = redv[0];
    for (int i = 1; i < LF_WAVES; ++i) mx = fmax(mx, redv[i]);
    const double thr = tol * mx;
    for (int k = tid; k < F; k += LF_THREADS) {
        const double xx = load(0, k);
        const bool valid = k >= k_lo && xx > 0.0 && xx >= thr;
        gk[k] = valid ? fmin(fmax(load(1, k) / xx, gmin), 1.0) : -1.0;
    }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0;
        P1[0] = 0.0;
        for (int k = 0; k < F; ++k) {
            const double g = gk[k], d = 1.0 - g;
            if (g >= 0.0) a = fma(d, d, a);
            P1[k + 1] = a;
        }
    } else if (tid == AID_WAVE) {
        double a = 0.0;
        int n = 0;
        S3[F] = 0.0;
        for (int k = F - 1; k >= 0; --k) {
            const double g = gk[k], d = gmin - g;
            if (g >= 0.0) { a = fma(d, d, a); ++n; }
            S3[k] = a;
        }
        redi[0] = n;
    }
    __syncthreads();
    const int n_valid = redi[0];
    const double inv_n = n_valid > 0 ? 1.0 / (double)n_valid : 0.0;
    __syncthreads();                                          // (redi is written again below)

    // every candidate: lane-private best (cost, j * NA + i), ties to the lower index.  The transition of a low cut-off is long and that of a
    // high one short, so lane q of a half takes the cut-offs j = q and NC - 1 - q (q += 512): about F bins per lane and slope whatever q.
    // The two halves of the workgroup take the two slopes of a pair, each with its own table k^(A s).
    const int half_id = tid >> 9, q0 = tid & (LF_THREADS / 2 - 1), n_pairs = (NC + 1) / 2;
    double bc = INFINITY;
    int bi = 0x7fffffff;
    for (int i0 = 0; i0 < NA; i0 += 2) {
        for (int e = tid; e < 2 * F; e += LF_THREADS) {
            const int s = e >= F, k = e - s * F, i = i0 + s;
            m.Ek[s][k] = (k && i < NA) ? exp2((double)ca[i] * s20 * log2((double)k)) : 1.0;
        }
        __syncthreads();
        const int i = i0 + half_id;
        if (i < NA) {
            const double As = (double)ca[i] * s20;
            const double* __restrict__ E = m.Ek[half_id];
            for (int q = q0; q < n_pairs; q += LF_THREADS / 2) {
                for (int side = 0; side < 2; ++side) {
                    const int j = side ? NC - 1 - q : q;
                    if (side && j <= q) break;                 // (the middle cut-off of an odd NC is taken once)
                    const double c = (double)cc[j];
                    const double inv = exp2(-As * log2(c));
                    const int k0 = min((int)floor(fmin(fmax(c, 0.0), (double)F)) + 1, F);      // the first bin right of the cut-off
                    double acc = P1[k0];
                    for (int k = k0; k < F; ++k) {
                        double h = E[k] * inv;
                        if (h <= gmin) { acc += S3[k]; break; }      // at the floor from here on (k^(A s) falls with k)
                        h = fmin(h, 1.0);
                        const double g = gk[k], d = h - g;
                        if (g >= 0.0) acc = fma(d, d, acc);
                    }
                    const double cost = acc * inv_n;
                    const int idx = j * NA + i;
                    if (cost < bc || (cost == bc && idx < bi)) { bc = cost; bi = idx; }
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double oc = __shfl_xor(bc, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (oc < bc || (oc == bc && oi < bi)) { bc = oc; bi = oi; }
    }
    if (lane == 0) { redv[wave] = bc; redi[wave] = bi; }
    __syncthreads();
    bc = redv[0]; bi = redi[0];
    for (int i = 1; i < LF_WAVES; ++i)
        if (redv[i] < bc || (redv[i] == bc && redi[i] < bi)) { bc = redv[i]; bi = redi[i]; }
    if (bi == 0x7fffffff) bi = 0;                             // (no cost compared: statistics that are not numbers)
    const double c = (double)cc[bi / NA], A = (double)ca[bi % NA];
    if (tid == 0) {
        fit[0] = (float)c; fit[1] = (float)A; fit[2] = (float)bc; fit[3] = (float)n_valid;
    }

    // H on the grid, cos(2 pi m / N) for m <= N/2, then the taps
    const double lc = log2(c);
    double* __restrict__ Hk = m.Ek[0];
    for (int k = tid; k < F; k += LF_THREADS) {
        Hk[k] = (double)k <= c ? 1.0 : exp2(fmax(floor_dB, fmin(0.0, A * (log2((double)k) - lc))) * s20);
        P1[k] = cospi(2.0 * (double)k / (double)N);
    }
    __syncthreads();
    const int P = (K - 1) / 2, half = N >> 1;
    for (int n = tid; n < K; n += LF_THREADS) {
        const int d = n - P;
        double acc = Hk[0];
        for (int k = 1; k < half; ++k) {
            const int mq = (k * d) & (N - 1), mm = mq > half ? N - mq : mq;
            acc = fma(2.0 * Hk[k], P1[mm], acc);
        }
        acc += (d & 1) ? -Hk[half] : Hk[half];
        taps[n] = (float)((double)w[n] / (double)N * acc);
    }
}

#endif
