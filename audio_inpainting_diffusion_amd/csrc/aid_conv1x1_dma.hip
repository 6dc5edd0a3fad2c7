// conv11_dma_kernel: 1x1 channel projections (res_conv / skip projections, unet...py:412-415,:488-491) as an
// fp32-MFMA GEMM with DIRECT-TO-LDS staging and small workgroup footprints.
//
// Why a third 1x1 kernel: these layers sit at the ridge (40-130 FLOP/B).  The register-staged tiled kernel
// (conv_mfma_kernel) runs a tile's load, MFMA and store phases back to back with one workgroup per CU; the streaming kernel
// (aid_conv1x1.hip) never overlaps a wave's loads, MFMAs and stores either.  Measured 12-20 % ahead of both.  Here
//   * both operands go HBM/L2 -> LDS with global_load_lds_dwordx4 into two STATIC buffers (see aid_conv_wino.hip: distinct
//     LDS objects keep the loads of chunk c+1 in flight while chunk c is multiplied);
//   * a buffer is 24 KB (16 channels x 256 positions + 16 x 128 weights) and a wave holds 64 accumulators, so two to three
//     workgroups share a CU: one tile's store-heavy epilogue overlaps another tile's K loop;
//   * a lane's NT = 2 position tiles are INTERLEAVED (tile j = positions 2n + j), so the B fragments of both tiles are ONE
//     conflict-free ds_read_b64 and the epilogue stores float2.
// Per-(b,ci) prologue scale (in_scale) is applied to the A fragment (a tile never straddles two samples: host-checked).
// Geometry record, tile origin (XCD-aware order) and row table are the shared frame of aid_conv_tile.h; the pieces (two K segments),
// the K loop and the float2 epilogue are this kernel's own.
#include "aid_conv_tile.h"
#include "aid_conv1x1_plan.h"
#include <type_traits>

int aid_conv_splitk_reduce(const aid_conv2d_params* p, const float* ws, int splits, hipStream_t st);      // aid_conv.hip
bool aid_conv_splitk_scratch_ok(const aid_conv2d_params* p, int S);

struct C11Dev {
    aid_conv2d_params p;
    const float* zero;
    ConvTileGeo g;             // XCD-aware 1-D grid (x); blockIdx.y is the K split
    int nch1;                  // chunks served by p.x (all of them unless p.x2 is given: then chunks >= nch1 read channels of p.x2)
    int splits, cps;           // split-K (grid-starved GEMMs: the qk projections, N = B*T columns only): blockIdx.y walks `splits` ranges of
    float* ws;                 // `cps` chunks; raw partial sums go to ws[z][B][Cout][F][T], reduced in a fixed order by aid_conv_splitk_reduce
};

// MT m-tiles (32 cout) x 2 interleaved position tiles per wave; WGM x WGN waves; N_BLK = 64 * WGN positions
template <int MT, int WGM, int WGN, int RMAX, int KC, int MINW>
__global__ __launch_bounds__(64 * WGM * WGN, MINW) void conv11_dma_kernel(const C11Dev a) {
    constexpr int NT = 2;
    constexpr int NW = WGM * WGN;
    constexpr int NTHREADS = 64 * NW;
    constexpr int M_BLK = 32 * MT * WGM;
    constexpr int N_BLK = 32 * NT * WGN;
    constexpr int XSZ = KC * N_BLK;
    constexpr int WROW = (M_BLK % 64 == 0) ? M_BLK : ((M_BLK + 63) / 64) * 64;
    constexpr int WSZ = KC * WROW;
    constexpr int BUFSZ = XSZ + WSZ;
    constexpr int NXP = XSZ / 256;
    constexpr int NWP = WSZ / 256;
    constexpr int NP = NXP + NWP;
    constexpr int PPW = (NP + NW - 1) / NW;
    constexpr int NSTEP = KC / 2;
    static_assert(N_BLK % 256 == 0 && WSZ % 256 == 0, "whole 1-KiB pieces");

    const aid_conv2d_params& p = a.p;
    const int TT = 1 << a.g.tt_log2;

    __shared__ __attribute__((aligned(16))) float sbuf0[BUFSZ];
    __shared__ __attribute__((aligned(16))) float sbuf1[BUFSZ];
    __shared__ int rowinfo[2 * RMAX];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WGN;
    const int wn = wave % WGN;

    ConvTileOrigin o;                                    // XCD-aware tile order: one contiguous (row-group, Cout-tile) range per XCD, Cout tile fastest
    if (!conv_tile_origin<M_BLK>(a.g, o)) return;
    conv_tile_rows<NTHREADS>(a.g, p.F, o.row0, rowinfo);
    const int tile_t = o.tile_t, row0 = o.row0, t0 = o.t0, m0 = o.m0;

    // ---- DMA piece descriptors ---------------------------------------------------------------------------------------
    const float* psrc[PPW];
    const float* psrc2[PPW];                             // second K segment (p.x2): same piece, channels of the other tensor
    int pstride[PPW], pstride2[PPW], plds[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int pc = wave + i * NW;
        psrc[i] = a.zero; pstride[i] = 0; plds[i] = -1;
        psrc2[i] = a.zero; pstride2[i] = 0;
        if (pc < NXP) {
            const int ci = pc / (N_BLK / 256), sub = pc % (N_BLK / 256);
            const int n = sub * 256 + 4 * lane;
            const int rr = n >> a.g.tt_log2, tt = n & (TT - 1);
            const int b = rowinfo[2 * rr];
            const int f = rowinfo[2 * rr + 1];
            plds[i] = ci * N_BLK + sub * 256;
            if (b >= 0 && t0 + tt < p.T) {
                psrc[i] = p.x.p + (int64_t)b * p.x.sB + (int64_t)ci * p.x.sC + (int64_t)f * p.x.sF + t0 + tt;
                pstride[i] = (int)(KC * p.x.sC);
                if (p.x2.p) {
                    psrc2[i] = p.x2.p + (int64_t)b * p.x2.sB + (int64_t)ci * p.x2.sC + (int64_t)f * p.x2.sF + t0 + tt;
                    pstride2[i] = (int)(KC * p.x2.sC);
                }
            }
        } else if (pc < NP) {
            const int wp_ = pc - NXP;
            const int e = wp_ * 256 + 4 * lane;
            const int ci = e / WROW, col = e % WROW;
            plds[i] = XSZ + wp_ * 256;
            if (col < M_BLK) {
                psrc[i] = p.wp + (int64_t)ci * p.Cout_pad + m0 + col;
                pstride[i] = KC * p.Cout_pad;
                psrc2[i] = psrc[i] + (int64_t)a.nch1 * pstride[i];       // (weights: one stacked pack, K continues)
                pstride2[i] = pstride[i];
            }
        }
    }
    // ---- operand addresses ---------------------------------------------------------------------------------------------
    const int half = lane >> 5;
    const int vB = half * N_BLK + wn * 64 + 2 * (lane & 31);        // float2: positions (2n, 2n+1) of this wave's 64
    int vA[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) vA[i] = XSZ + half * WROW + (wm * MT + i) * 32 + (lane & 31);
    const int b_tile = rowinfo[0];
    const float* sp = (p.in_scale && b_tile >= 0) ? p.in_scale + (int64_t)b_tile * p.in_scale_ld + half : nullptr;

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    auto issue_dma = [&](int ch, float* buf) {
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            if (plds[i] >= 0) {
                const float* src = ch < a.nch1 ? psrc[i] + (int64_t)ch * pstride[i] : psrc2[i] + (int64_t)(ch - a.nch1) * pstride2[i];
                AID_GLDS16(src, buf + plds[i]);
            }
        }
    };
    float sc[2][NSTEP];                                              // prologue scales of the current / next chunk
    auto load_scales = [&](int ch, int q) {
#pragma unroll
        for (int s = 0; s < NSTEP; ++s) {
            const int ci = ch * KC + 2 * s + half;
            sc[q][s] = (sp && ci < p.Cin) ? sp[ch * KC + 2 * s] : 1.f;
        }
    };

    const int ch_lo = blockIdx.y * a.cps;                            // this workgroup's K range (the whole K unless split)
    const int ch_hi = min(a.g.nchunks, ch_lo + a.cps);
    issue_dma(ch_lo, sbuf0);
    load_scales(ch_lo, 0);
    __syncthreads();

    auto chunk = [&](auto curc, int ch) {
        constexpr int cur = decltype(curc)::value;
        const float* Bf = cur ? sbuf1 : sbuf0;
        float* Nx = cur ? sbuf0 : sbuf1;
        const bool more = (ch + 1) < ch_hi;
        if (more) { issue_dma(ch + 1, Nx); load_scales(ch + 1, cur ^ 1); }
        float2 bv[2];
        float av[2][MT];
        auto load_step = [&](int s, int buf) {
            bv[buf] = *reinterpret_cast<const float2*>(Bf + vB + 2 * s * N_BLK);
#pragma unroll
            for (int i = 0; i < MT; ++i) av[buf][i] = Bf[vA[i] + 2 * s * WROW];
        };
        load_step(0, 0);
#pragma unroll
        for (int s = 0; s < NSTEP; ++s) {
            if (s + 1 < NSTEP) load_step(s + 1, (s + 1) & 1);
            const int bq = s & 1;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const float aw = av[bq][i] * sc[cur][s];
                acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(aw, bv[bq].x, acc[i][0], 0, 0, 0);
                acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(aw, bv[bq].y, acc[i][1], 0, 0, 0);
            }
        }
        __syncthreads();
    };
    for (int ch = ch_lo; ch < ch_hi; ch += 2) {
        chunk(std::integral_constant<int, 0>{}, ch);
        if (ch + 1 < ch_hi) chunk(std::integral_constant<int, 1>{}, ch + 1);
    }

    // ---- epilogue: two consecutive positions per lane and output channel ---------------------------------------------
    const int n = wn * 64 + 2 * (lane & 31);
    const int rr = n >> a.g.tt_log2, tt = n & (TT - 1);
    const int b = rowinfo[2 * rr];
    const int f = rowinfo[2 * rr + 1];
    const int t = t0 + tt;
    const bool live = !(b < 0 || t >= p.T);                          // T % 2 == 0: both samples in range together
    if (!live && !p.dot_ws) return;
    if (live && a.splits > 1) {                                      // split-K: raw partial sums (float2 per output channel)
        const int64_t ft = (int64_t)p.F * p.T;
        float* wsb = a.ws + (((int64_t)blockIdx.y * p.B + b) * p.Cout) * ft + (int64_t)f * p.T + t;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int mbase = m0 + (wm * MT + i) * 32 + 4 * half;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mbase + (r & 3) + 8 * (r >> 2);
                if (m < p.Cout) *reinterpret_cast<float2*>(wsb + (int64_t)m * ft) = make_float2(acc[i][0][r], acc[i][1][r]);
            }
        }
    }
    if (a.splits > 1) return;
    const int64_t ybase = (int64_t)b * p.y.sB + (int64_t)f * p.y.sF + t;
    const int64_t rbase = p.res.p ? ((int64_t)b * p.res.sB + (int64_t)f * p.res.sF + t) : 0;
    const int64_t abase = p.aux.p ? ((int64_t)b * p.aux.sB + (int64_t)f * p.aux.sF + t) : 0;
    float dsum[MT][4];                                               // <y, aux> per block of 4 rows (dot_ws)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) dsum[i][q] = 0.f;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        if (!live) break;
        const int mbase = m0 + (wm * MT + i) * 32 + 4 * half;
#pragma unroll
        for (int r0 = 0; r0 < 16; r0 += 4) {             // gather 4 rows, then compute + store (res may alias y)
            float2 rv[4], uv[4];
            float sv[4], as[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = r0 + q;
                const int m = mbase + (r & 3) + 8 * (r >> 2);
                const bool ok = m < p.Cout;
                rv[q] = (ok && p.res.p) ? *reinterpret_cast<const float2*>(p.res.p + rbase + (int64_t)m * p.res.sC) : make_float2(0.f, 0.f);
                sv[q] = (ok && p.out_scale) ? p.out_scale[(int64_t)b * p.out_scale_ld + m] : 1.f;
                if (ok && p.epi == 1) {
                    as[q] = p.aux_scale[(int64_t)b * p.aux_scale_ld + m];
                    uv[q] = *reinterpret_cast<const float2*>(p.aux.p + abase + (int64_t)m * p.aux.sC);
                } else { as[q] = 0.f; uv[q] = make_float2(0.f, 0.f); }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = r0 + q;
                const int m = mbase + (r & 3) + 8 * (r >> 2);
                if (m >= p.Cout) continue;
                float y0 = acc[i][0][r] * sv[q], y1 = acc[i][1][r] * sv[q];
                if (p.epi == 1) { y0 *= aid_dgelu(uv[q].x * as[q]); y1 *= aid_dgelu(uv[q].y * as[q]); }
                y0 += p.res_scale * rv[q].x;
                y1 += p.res_scale * rv[q].y;
                y0 *= p.alpha; y1 *= p.alpha;
                *reinterpret_cast<float2*>(p.y.p + ybase + (int64_t)m * p.y.sC) = make_float2(y0, y1);
                if (p.dot_ws) dsum[i][r0 >> 2] += y0 * uv[q].x + y1 * uv[q].y;
            }
        }
    }
    if (p.dot_ws) {                                                  // per (sample, channel group): one partial per position tile (as conv53_wino4r_kernel)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float v = live ? dsum[i][q] : 0.f;
#pragma unroll
                for (int off = 16; off >= 1; off >>= 1) v += __shfl_xor(v, off, 32);
                dsum[i][q] = v;
            }
        float* red = sbuf0;                                          // (every wave is past the last chunk's barrier)
        if ((lane & 31) == 0) {
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) red[((wave * 2 + half) * MT + i) * 4 + q] = dsum[i][q];
        }
        __syncthreads();
        const int cpg = p.Cout >> 3;                                 // channels per group (8 groups); M_BLK % cpg == 0 and cpg % 4 == 0 (host-checked)
        const int grp = m0 / cpg + tid;
        if (tid < M_BLK / cpg && grp < 8) {
            float sacc = 0.f;
            for (int w = 0; w < NW; ++w)                             // fixed order: deterministic
                for (int h = 0; h < 2; ++h)
                    for (int i = 0; i < MT; ++i)
                        for (int q = 0; q < 4; ++q) {
                            const int mrow = m0 + ((w / WGN) * MT + i) * 32 + 4 * h + 8 * q;
                            if (mrow < p.Cout && mrow / cpg == grp) sacc += red[((w * 2 + h) * MT + i) * 4 + q];
                        }
            const int bt = rowinfo[0];
            const int ptile = ((row0 - bt * p.F) >> a.g.rows_log2) * a.g.tiles_t + tile_t;
            p.dot_ws[((int64_t)bt * 8 + grp) * p.dot_n + ptile] = (double)sacc;
        }
    }
}

template <int MT, int WGM, int WGN, int RMAX, int KC, int MINW>
static int launch_c11(const aid_conv2d_params* p, hipStream_t st, const C11Plan& pl) {
    C11Dev a;
    a.p = *p;
    a.zero = aid_zero_page();
    if (!a.zero) return AID_E_LAUNCH;
    a.g.tt_log2 = aid_ilog2(pl.TT);
    a.g.rows_log2 = aid_ilog2(pl.ROWS);
    a.g.tiles_t = pl.tiles_t;
    a.g.nrows = pl.nrows;
    a.g.nchunks = pl.nchunks;
    a.nch1 = pl.nch1;
    a.g.nx = pl.nx;
    a.g.ny = pl.ny;
    a.g.per_xcd = (int)(((int64_t)a.g.nx * a.g.ny + 7) / 8);
    a.cps = pl.kps / KC;
    a.splits = aid_cdiv(a.g.nchunks, a.cps);
    a.ws = (float*)p->ws;
    hipLaunchKernelGGL((conv11_dma_kernel<MT, WGM, WGN, RMAX, KC, MINW>), dim3((unsigned)(8 * a.g.per_xcd), (unsigned)a.splits), dim3(64 * WGM * WGN), 0, st, a);
    AID_CHECK_LAUNCH();
    aid_note_kernel(a.splits > 1 ? "conv11_dma_kernel+splitk" : "conv11_dma_kernel");
    if (a.splits > 1) return aid_conv_splitk_reduce(p, (const float*)p->ws, a.splits, st);
    return AID_OK;
}

// ---- skinny GEMM: the qk projections when N = B*T <= 128 columns (the reference's testers run B = 1) -------------------------------------
// y[M, N] = W^T x with K, M in the thousands and N of 32 ... 128: the weights (52 ... 103 MB per layer) are read once and nothing else matters.
// The tiled kernels stage one 8-KB weight chunk per workgroup at a time: 0.7 TB/s (latency-bound: Little's law wants ~48 KB in flight per CU).
// Here a wave owns 32 output rows x all N columns of one K range and loads BOTH operands straight from global memory into the MFMA fragments
// (weights: 2 x 128 contiguous bytes per load, x: L2-resident), U = 8 k-pairs unrolled = 16 independent loads in flight per wave, no LDS, no
// barriers; K is split over blockIdx.y and the partial sums go through the same fixed-order reduction as the other split-K paths.
template <int NT>
__global__ __launch_bounds__(256) void gemm_skinny_kernel(const aid_conv2d_params p, float* __restrict__ ws, int kps) {
    constexpr int U = 8;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m0 = (blockIdx.x * 4 + wave) * 32;
    if (m0 >= p.Cout_pad) return;
    const int half = lane >> 5, l31 = lane & 31;
    const int k0 = blockIdx.y * kps, k1 = min(p.Cin, k0 + kps);
    const float* wp = p.wp + m0 + l31;
    const float* xq[NT];
    bool ok[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = j * 32 + l31;
        const int b = n / p.T, t = n - b * p.T;
        ok[j] = b < p.B;
        xq[j] = p.x.p + (ok[j] ? ((int64_t)b * p.x.sB + t) : 0);
    }
    f32x16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    for (int kk = k0; kk < k1; kk += 2 * U) {
        float a[U], bv[U][NT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = kk + 2 * u + half;
            const bool kin = k < k1;
            a[u] = kin ? wp[(int64_t)k * p.Cout_pad] : 0.f;
#pragma unroll
            for (int j = 0; j < NT; ++j) bv[u][j] = (kin && ok[j]) ? xq[j][(int64_t)k * p.x.sC] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], bv[u][j], acc[j], 0, 0, 0);
    }
    const int64_t ft = p.T;                                         // F = 1
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = j * 32 + l31;
        const int b = n / p.T, t = n - b * p.T;
        if (b >= p.B) continue;
        float* wsb = ws + (((int64_t)blockIdx.y * p.B + b) * p.Cout) * ft + t;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + 4 * half + (r & 3) + 8 * (r >> 2);
            if (m < p.Cout) wsb[(int64_t)m * ft] = acc[j][r];
        }
    }
}

// returns 1 if this kernel took the launch, 0 if not eligible, <0 on error
int aid_conv1x1_dma_try(const aid_conv2d_params* p, hipStream_t st) {
    if (!(p->KH == 1 && p->KW == 1)) return 0;
    C11Shape s = c11_shape_of(*p);
    C11Plan pl = c11_dma_plan(s);
    if (!pl.family) return 0;
    if (!aid_view_aligned(p->x, 4) || !aid_view_aligned(p->y, 2) || (p->res.p && !aid_view_aligned(p->res, 2)) || (p->aux.p && !aid_view_aligned(p->aux, 2))) return 0;
    if ((int64_t)4 * 16 * p->x.sC >= (1LL << 31)) return 0;
    if (p->x2.p && (!aid_view_aligned(p->x2, 4) || (int64_t)4 * 16 * p->x2.sC >= (1LL << 31))) return 0;
    if (p->dot_ws && p->dot_n != pl.slots) return 0;
    if (pl.S > 1 && !aid_conv_splitk_scratch_ok(p, pl.S)) {      // y or res not aligned for the reduction: the plan without scratch (a single pass)
        s.ws = false;
        pl = c11_dma_plan(s);
    }
    int rc;
    if (pl.family == C11_SKINNY) {
        const dim3 grid((unsigned)pl.gx, (unsigned)pl.S);
        switch (pl.nt) {
            case 1: hipLaunchKernelGGL(gemm_skinny_kernel<1>, grid, dim3(256), 0, st, *p, (float*)p->ws, pl.kps); break;
            case 2: hipLaunchKernelGGL(gemm_skinny_kernel<2>, grid, dim3(256), 0, st, *p, (float*)p->ws, pl.kps); break;
            case 3: hipLaunchKernelGGL(gemm_skinny_kernel<3>, grid, dim3(256), 0, st, *p, (float*)p->ws, pl.kps); break;
            default: hipLaunchKernelGGL(gemm_skinny_kernel<4>, grid, dim3(256), 0, st, *p, (float*)p->ws, pl.kps); break;
        }
        AID_CHECK_LAUNCH();
        aid_note_kernel("gemm_skinny_kernel+splitk");
        rc = aid_conv_splitk_reduce(p, (const float*)p->ws, pl.S, st);
    } else if (pl.MT == 2) rc = launch_c11<2, 2, 4, 16, 16, 4>(p, st, pl);      // 128 x 256, 8 waves, 2 workgroups / CU
    else if (pl.MT == 1) rc = launch_c11<1, 2, 4, 16, 16, 4>(p, st, pl);        //  64 x 256
    else                 rc = launch_c11<3, 1, 4, 16, 16, 2>(p, st, pl);        //  96 x 256, 4 waves
    return rc == AID_OK ? 1 : rc;
}
