// aid_time_attention_long / aid_time_attention_long_bwd: the attention core of aid_attn.hip (same layouts, same MFMA operand mapping, same exact
// two-pass softmax -- read that file's header first) for sequences up to T = AID_ATTN_LONG_MAX_T = 1024, on v_mfma_f32_32x32x2_f32 throughout.
//
// forward, grid (B*H, ceil(T/32) query tiles), 4 waves, template on NT = key tiles per wave (1, 2, 4, 8 <-> T <= 128, 256, 512, 1024):
//   wave w owns the key tiles kt = w + 4 i (i < NT), i.e. ONE tile of every 128-key chunk, and keeps their S^T tiles in 16 NT accumulators.  A query's
//   <= 1024 logits therefore all sit in the registers of its workgroup: max and sum reduce over the lane's registers, one shuffle across the half-waves
//   and one LDS exchange between the four waves -- no running rescale.
//   P V walks the keys in chunks of 128: the four waves lay tile i of P^T into the 17 KB LDS tile, barrier, every wave fetches the chunk's 64 B
//   fragments, barrier, and feeds the accumulators of its F tiles.  A wave carries ATL_FG = 4 F tiles (16 of them per workgroup = 512 rows of F, the
//   largest head the shipped networks have); a larger F takes another trip through the chunks, with P still in registers (probs may be NULL).
//   budget: 16 NT score accumulators + 64 B fragments + 64 O accumulators + the V loads in flight; as compiled (VGPR + AGPR, no scratch):
//   NT = 1: 146 + 64, NT = 2: 177 + 64 (two workgroups per CU), NT = 4: 256 + 84, NT = 8: 256 + 196 (one); static LDS 18 KB (17 KB P^T tile + reductions).
//   The row sum and 1 / sum are carried in double, and so are d and dP - d in the backward: see the comment at the sum.
// backward:
//   attn_long_bwd_ds<NT>: the forward's tiling for dP^T = V^T dO; d_n = <P[n,:], dP[n,:]> reduces over all of the lane's tiles, the half-waves and the
//                         four waves BEFORE any dS is written; P is read a second time (L1 / L2) for the store instead of being held in 16 NT registers.
//   attn_long_bwd_fr    : aid_attn.hip's attn_bwd_fr_kernel<4> with a column-group dimension: grid (B*H, ceil(F/32), ceil(T/128)), wave w of group z
//                         owns columns [128 z + 32 w, +32); the contraction runs over all T.
// Deterministic (no atomics), nothing allocated, no dynamic LDS and no function attributes: the launches are captured into HIP graphs.
#include "aid_common.h"
#include "aid_mfma_dma.h"

#define ATL_TMAX AID_ATTN_LONG_MAX_T
#define ATL_CHUNK 128         // keys per P V chunk (one 32-key tile per wave)
#define ATL_LDP 33            // leading dimension of the P^T exchange tile in LDS (conflict-free column access)
#define ATL_FG 4              // F tiles (32 rows each) a wave accumulates per trip through the key chunks

namespace {

__device__ __forceinline__ float4 atl_ld4(const float* __restrict__ row, int c, int T, bool row_ok, bool vec_ok) {
    // four consecutive columns c..c+3 of one row; zeros outside [0,T) or when the row does not exist
    if (!row_ok) return make_float4(0.f, 0.f, 0.f, 0.f);
    if (vec_ok && c + 3 < T) return *reinterpret_cast<const float4*>(row + c);
    float4 v;
    v.x = (c + 0 < T) ? row[c + 0] : 0.f;
    v.y = (c + 1 < T) ? row[c + 1] : 0.f;
    v.z = (c + 2 < T) ? row[c + 2] : 0.f;
    v.w = (c + 3 < T) ? row[c + 3] : 0.f;
    return v;
}

__device__ __forceinline__ void atl_st4(float* __restrict__ row, int c, int T, bool vec_ok, float4 v) {
    if (vec_ok && c + 3 < T) { *reinterpret_cast<float4*>(row + c) = v; return; }
    if (c + 0 < T) row[c + 0] = v.x;
    if (c + 1 < T) row[c + 1] = v.y;
    if (c + 2 < T) row[c + 2] = v.z;
    if (c + 3 < T) row[c + 3] = v.w;
}

// acc[i] = sum_f A[f][ma_i] * Bm[f][nb] for the wave's NT tiles (rows: columns (wave + 4 i) * 32 .. of A, cols: columns nb0.. of Bm); A, Bm are [F][T].
// The B operand is loaded once per k-step and shared by the NT tiles; every tile sums over f in the order of aid_attn.hip's att_scores_tile.
template <int NT>
__device__ __forceinline__ void atl_scores(f32x16 (&acc)[NT], const float* __restrict__ A, const float* __restrict__ Bm, int F, int T, int wave,
                                           int l32, int nb, int half) {
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    const bool bok = nb < T;
    const float* bp = Bm + nb;
    for (int f = 0; f < F; f += 16) {                        // 8 k-steps per trip
        float b[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int fr = f + 2 * u + half;
            b[u] = (bok && fr < F) ? bp[(int64_t)fr * T] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int m0 = (wave + 4 * i) * 32;
            if (m0 < T) {                                     // (wave-uniform)
                const int ma = m0 + l32;
                float a[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int fr = f + 2 * u + half;
                    a[u] = (ma < T && fr < F) ? A[(int64_t)fr * T + ma] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc[i], 0, 0, 0);
            }
        }
    }
}

// =====================================================================================================
// forward
// =====================================================================================================
template <int NT>
__global__ __launch_bounds__(256) void time_attention_long_kernel(const aid_attention_params p) {
    const int bh = blockIdx.x;
    const int b = bh / p.H, h = bh - b * p.H;
    const int n0 = blockIdx.y * 32;
    const int T = p.T, F = p.F;
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l32 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool vec = ((T & 3) == 0) && ((((uintptr_t)p.v) | ((uintptr_t)p.probs)) & 15) == 0;
    __shared__ float red[4][32];
    __shared__ double redd[4][32];
    __shared__ float Pt[ATL_CHUNK * ATL_LDP];              // P^T[m][n] of this query tile, one 128-key chunk at a time
    const float* Q = p.qk + ((int64_t)b * p.H * 2 * F + (int64_t)h * 2 * F) * T;
    const float* K = Q + (int64_t)F * T;
    const float* V = p.v + (int64_t)bh * F * T;
    float* O = p.out + (int64_t)bh * F * T;
    const int n = n0 + l32;

    f32x16 acc[NT];
    atl_scores<NT>(acc, K, Q, F, T, wave, l32, n, half);      // S^T[m][n]; tiles past T stay zero
    if (p.bias && n < T) {                                   // sim = (q k^T + bias[h][n][m]) * scale
        const float* brow = p.bias + ((int64_t)h * T + n) * T;
        const bool bvec = vec && ((((uintptr_t)p.bias) & 15) == 0);
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int m0 = (wave + 4 * i) * 32;
            if (m0 < T) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int mb = m0 + 8 * q + 4 * half;
                    const float4 bb = atl_ld4(brow, mb, T, mb < T, bvec);
                    acc[i][4 * q] += bb.x; acc[i][4 * q + 1] += bb.y; acc[i][4 * q + 2] += bb.z; acc[i][4 * q + 3] += bb.w;
                }
            }
        }
    }
    // ---- softmax over the keys of query n: registers (all NT tiles) -> half-waves (shuffle) -> waves (LDS) --------------------------------------
    float mx = -3.0e38f;
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = (wave + 4 * i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            acc[i][r] *= p.scale;
            if (m < T) mx = fmaxf(mx, acc[i][r]);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (half == 0) red[wave][l32] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0][l32], red[1][l32]), fmaxf(red[2][l32], red[3][l32]));
    // The row sum and the normalisation are carried in double (a few VALU operations per accumulator, nothing next to the products): a row that one
    // key dominates has p -> 1, and the backward amplifies the rounding of that p by 1 / (1 - p); with up to 1024 terms added at magnitude 1 a float
    // sum is off by several ulp, the double one leaves p correctly rounded.
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = (wave + 4 * i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            acc[i][r] = (m < T) ? expf(acc[i][r] - mx) : 0.f;
            sum += (double)acc[i][r];
        }
    sum += __shfl_xor(sum, 32, 64);
    if (half == 0) redd[wave][l32] = sum;
    __syncthreads();
    const double inv = 1.0 / ((redd[0][l32] + redd[1][l32]) + (redd[2][l32] + redd[3][l32]));
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int m0 = (wave + 4 * i) * 32;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = (float)((double)acc[i][r] * inv);
        if (p.probs && n < T && m0 < T) {
            float* prow = p.probs + ((int64_t)bh * T + n) * T;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int mb = m0 + 8 * q + 4 * half;
                if (mb < T) atl_st4(prow, mb, T, vec, make_float4(acc[i][4 * q], acc[i][4 * q + 1], acc[i][4 * q + 2], acc[i][4 * q + 3]));
            }
        }
    }
    // ---- O[f][n] = sum_m V[f][m] P[n][m], keys in chunks of 128, pairing (m, m+4) inside a chunk ------------------------------------------------
    const int ntile = (F + 31) >> 5;
    for (int g0 = 0; g0 < ntile; g0 += 4 * ATL_FG) {          // (one trip for F <= 512)
        f32x16 o[ATL_FG];
#pragma unroll
        for (int t = 0; t < ATL_FG; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
        // (expanded at compile time: the body is past the size up to which a loop pragma unrolls, and acc[i] must stay a register index)
        aid_static_for<NT>([&](auto ic) __attribute__((always_inline)) {
            constexpr int i = decltype(ic)::value;
            const int k0 = i * ATL_CHUNK;                     // first key of this chunk
            if (k0 < T) {                                     // (uniform over the workgroup: the barriers below are met by all or by none)
                __syncthreads();                              // the previous chunk's fragments have been fetched by every wave
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int ml = wave * 32 + 8 * q + 4 * half;     // row inside the chunk (rows of keys >= T hold zeros)
                    Pt[(ml + 0) * ATL_LDP + l32] = acc[i][4 * q];
                    Pt[(ml + 1) * ATL_LDP + l32] = acc[i][4 * q + 1];
                    Pt[(ml + 2) * ATL_LDP + l32] = acc[i][4 * q + 2];
                    Pt[(ml + 3) * ATL_LDP + l32] = acc[i][4 * q + 3];
                }
                __syncthreads();
                float bf[ATL_CHUNK / 2];
#pragma unroll
                for (int j = 0; j < ATL_CHUNK / 8; ++j)
#pragma unroll
                    for (int s = 0; s < 4; ++s) bf[4 * j + s] = (k0 + 8 * j < T) ? Pt[(8 * j + s + 4 * half) * ATL_LDP + l32] : 0.f;
#pragma unroll
                for (int t = 0; t < ATL_FG; ++t) {
                    const int ft = g0 + wave + 4 * t;
                    if (ft < ntile) {                         // (wave-uniform)
                        const int row = ft * 32 + l32;
                        const float* vr = V + (int64_t)row * T;
#pragma unroll
                        for (int j = 0; j < ATL_CHUNK / 8; ++j) {
                            if (k0 + 8 * j < T) {             // (wave-uniform)
                                const float4 a = atl_ld4(vr, k0 + 8 * j + 4 * half, T, row < F, vec);
                                o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bf[4 * j + 0], o[t], 0, 0, 0);
                                o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bf[4 * j + 1], o[t], 0, 0, 0);
                                o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bf[4 * j + 2], o[t], 0, 0, 0);
                                o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bf[4 * j + 3], o[t], 0, 0, 0);
                            }
                        }
                    }
                }
            }
        });
        if (n < T) {
#pragma unroll
            for (int t = 0; t < ATL_FG; ++t) {
                const int ft = g0 + wave + 4 * t;
                if (ft < ntile) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int f = ft * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                        if (f < F) O[(int64_t)f * T + n] = o[t][r];
                    }
                }
            }
        }
    }
}

// =====================================================================================================
// backward: dS = P (dP - rowsum(P dP)) * scale -> ws, then dV, dQ, dK
// =====================================================================================================
template <int NT>
__global__ __launch_bounds__(256) void attn_long_bwd_ds_kernel(const aid_attention_bwd_params p, float* __restrict__ dS) {
    const int bh = blockIdx.x;
    const int n0 = blockIdx.y * 32;
    const int T = p.T, F = p.F;
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l32 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool vec = ((T & 3) == 0) && ((((uintptr_t)p.probs) | ((uintptr_t)dS)) & 15) == 0;
    __shared__ double red[4][32];
    const float* V = p.v + (int64_t)bh * F * T;
    const float* dO = p.gout + (int64_t)bh * F * T;
    const int n = n0 + l32;
    f32x16 acc[NT];
    atl_scores<NT>(acc, V, dO, F, T, wave, l32, n, half);     // dP^T[m][n]
    const float* Prow = p.probs + ((int64_t)bh * T + n) * T;
    // d and dP - d in double (see the forward's row sum): where one key takes p -> 1, dP - d cancels down to (1 - p) of its terms, and a float d
    // summed over up to 1024 keys would leave its own rounding, amplified by 1 / (1 - p), in that row of dS and in the column of dQ it feeds
    double d = 0.0;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int m0 = (wave + 4 * i) * 32;
        if (m0 < T) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int mb = m0 + 8 * q + 4 * half;
                const float4 v = atl_ld4(Prow, mb, T, n < T && mb < T, vec);
                d += ((double)v.x * (double)acc[i][4 * q] + (double)v.y * (double)acc[i][4 * q + 1]) +
                     ((double)v.z * (double)acc[i][4 * q + 2] + (double)v.w * (double)acc[i][4 * q + 3]);
            }
        }
    }
    d += __shfl_xor(d, 32, 64);
    if (half == 0) red[wave][l32] = d;
    __syncthreads();
    d = (red[0][l32] + red[1][l32]) + (red[2][l32] + red[3][l32]);
    if (n >= T) return;
    float* o = dS + ((int64_t)bh * T + n) * T;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int m0 = (wave + 4 * i) * 32;
        if (m0 < T) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int mb = m0 + 8 * q + 4 * half;
                if (mb < T) {
                    const float4 v = atl_ld4(Prow, mb, T, true, vec);
                    const double sx = (double)v.x * p.scale, sy = (double)v.y * p.scale, sz = (double)v.z * p.scale, sw = (double)v.w * p.scale;
                    atl_st4(o, mb, T, vec, make_float4((float)(sx * ((double)acc[i][4 * q] - d)), (float)(sy * ((double)acc[i][4 * q + 1] - d)),
                                                       (float)(sz * ((double)acc[i][4 * q + 2] - d)), (float)(sw * ((double)acc[i][4 * q + 3] - d))));
                }
            }
        }
    }
}

// one wave = 32 rows of F x 32 columns of T; a workgroup = 32 rows x the 128 columns of column group blockIdx.z
__global__ __launch_bounds__(256) void attn_long_bwd_fr_kernel(const aid_attention_bwd_params p, const float* __restrict__ dS) {
    const int bh = blockIdx.x;
    const int b = bh / p.H, h = bh - b * p.H;
    const int T = p.T, F = p.F;
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l32 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int f0 = blockIdx.y * 32;
    const int c0 = (blockIdx.z * 4 + wave) * 32;
    if (f0 >= F || c0 >= T) return;                           // (no barriers below)
    const float* Q = p.qk + ((int64_t)b * p.H * 2 * F + (int64_t)h * 2 * F) * T;
    const float* K = Q + (int64_t)F * T;
    const float* dO = p.gout + (int64_t)bh * F * T;
    float* dQ = p.gqk + ((int64_t)b * p.H * 2 * F + (int64_t)h * 2 * F) * T;
    float* dK = dQ + (int64_t)F * T;
    float* dV = p.gv + (int64_t)bh * F * T;
    const float* Pg = p.probs + (int64_t)bh * T * T;
    const float* Sg = dS + (int64_t)bh * T * T;
    const bool vec = ((T & 3) == 0) && ((((uintptr_t)p.qk) | ((uintptr_t)p.gout) | ((uintptr_t)dS)) & 15) == 0;
    const int row = f0 + l32;                                 // A-fragment row of this lane
    const bool rok = row < F;
    const int col = c0 + l32;                                 // B-fragment / output column of this lane
    const bool cok = col < T;
    f32x16 aV, aQ, aK;
#pragma unroll
    for (int r = 0; r < 16; ++r) { aV[r] = 0.f; aQ[r] = 0.f; aK[r] = 0.f; }
    const float* dOr = dO + (int64_t)row * T;
    const float* Kr = K + (int64_t)row * T;
    const float* Qr = Q + (int64_t)row * T;
    const float* Srow = Sg + (int64_t)col * T;                // dS[n = col][.]
    for (int j = 0; 8 * j < T; ++j) {
        const int k0 = 8 * j + 4 * half;                      // this half-wave's four contraction indices k0..k0+3
        const float4 a_do = atl_ld4(dOr, k0, T, rok, vec);
        const float4 a_k = atl_ld4(Kr, k0, T, rok, vec);
        const float4 a_q = atl_ld4(Qr, k0, T, rok, vec);
        const float4 b_s = atl_ld4(Srow, k0, T, cok, vec);    // dS[col][k0..k0+3]: B of dQ (contraction over keys m = k)
        float bp[4], bs[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const bool ok = cok && (k0 + s) < T;
            bp[s] = ok ? Pg[(int64_t)(k0 + s) * T + col] : 0.f;      // P[n = k][m = col]
            bs[s] = ok ? Sg[(int64_t)(k0 + s) * T + col] : 0.f;      // dS[n = k][m = col]
        }
        aV = __builtin_amdgcn_mfma_f32_32x32x2f32(a_do.x, bp[0], aV, 0, 0, 0);
        aV = __builtin_amdgcn_mfma_f32_32x32x2f32(a_do.y, bp[1], aV, 0, 0, 0);
        aV = __builtin_amdgcn_mfma_f32_32x32x2f32(a_do.z, bp[2], aV, 0, 0, 0);
        aV = __builtin_amdgcn_mfma_f32_32x32x2f32(a_do.w, bp[3], aV, 0, 0, 0);
        aQ = __builtin_amdgcn_mfma_f32_32x32x2f32(a_k.x, b_s.x, aQ, 0, 0, 0);
        aQ = __builtin_amdgcn_mfma_f32_32x32x2f32(a_k.y, b_s.y, aQ, 0, 0, 0);
        aQ = __builtin_amdgcn_mfma_f32_32x32x2f32(a_k.z, b_s.z, aQ, 0, 0, 0);
        aQ = __builtin_amdgcn_mfma_f32_32x32x2f32(a_k.w, b_s.w, aQ, 0, 0, 0);
        aK = __builtin_amdgcn_mfma_f32_32x32x2f32(a_q.x, bs[0], aK, 0, 0, 0);
        aK = __builtin_amdgcn_mfma_f32_32x32x2f32(a_q.y, bs[1], aK, 0, 0, 0);
        aK = __builtin_amdgcn_mfma_f32_32x32x2f32(a_q.z, bs[2], aK, 0, 0, 0);
        aK = __builtin_amdgcn_mfma_f32_32x32x2f32(a_q.w, bs[3], aK, 0, 0, 0);
    }
    if (!cok) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int f = f0 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (f >= F) continue;
        const int64_t o = (int64_t)f * T + col;
        dV[o] = (p.accumulate_gv ? dV[o] : 0.f) + aV[r];
        dQ[o] = aQ[r];
        dK[o] = aK[r];
    }
}

}  // namespace

extern "C" int aid_time_attention_long(const aid_attention_params* p, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    AID_REQUIRE(p && p->qk && p->v && p->out, "aid_time_attention_long: null pointer");
    AID_REQUIRE(p->T >= 1 && p->T <= ATL_TMAX, "aid_time_attention_long: T must be in [1,1024]");
    AID_REQUIRE(p->B > 0 && p->H > 0 && p->F > 0, "aid_time_attention_long: empty shape");
    const dim3 grid((unsigned)(p->B * p->H), (unsigned)aid_cdiv(p->T, 32));
    if (p->T <= 128) hipLaunchKernelGGL(time_attention_long_kernel<1>, grid, dim3(256), 0, st, *p);
    else if (p->T <= 256) hipLaunchKernelGGL(time_attention_long_kernel<2>, grid, dim3(256), 0, st, *p);
    else if (p->T <= 512) hipLaunchKernelGGL(time_attention_long_kernel<4>, grid, dim3(256), 0, st, *p);
    else hipLaunchKernelGGL(time_attention_long_kernel<8>, grid, dim3(256), 0, st, *p);
    AID_CHECK_LAUNCH();
    return AID_OK;
}

extern "C" int aid_time_attention_long_bwd(const aid_attention_bwd_params* p, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    AID_REQUIRE(p && p->qk && p->v && p->probs && p->gout && p->gqk && p->gv && p->ws, "aid_time_attention_long_bwd: null pointer");
    AID_REQUIRE(p->T >= 1 && p->T <= ATL_TMAX, "aid_time_attention_long_bwd: T must be in [1,1024]");
    AID_REQUIRE(p->B > 0 && p->H > 0 && p->F > 0, "aid_time_attention_long_bwd: empty shape");
    const dim3 gds((unsigned)(p->B * p->H), (unsigned)aid_cdiv(p->T, 32));
    if (p->T <= 128) hipLaunchKernelGGL(attn_long_bwd_ds_kernel<1>, gds, dim3(256), 0, st, *p, p->ws);
    else if (p->T <= 256) hipLaunchKernelGGL(attn_long_bwd_ds_kernel<2>, gds, dim3(256), 0, st, *p, p->ws);
    else if (p->T <= 512) hipLaunchKernelGGL(attn_long_bwd_ds_kernel<4>, gds, dim3(256), 0, st, *p, p->ws);
    else hipLaunchKernelGGL(attn_long_bwd_ds_kernel<8>, gds, dim3(256), 0, st, *p, p->ws);
    AID_CHECK_LAUNCH();
    const dim3 gfr((unsigned)(p->B * p->H), (unsigned)aid_cdiv(p->F, 32), (unsigned)aid_cdiv(p->T, 128));
    hipLaunchKernelGGL(attn_long_bwd_fr_kernel, gfr, dim3(256), 0, st, *p, (const float*)p->ws);
    AID_CHECK_LAUNCH();
    return AID_OK;
}
