// The tile frame of the position-tiled convolution kernels: conv_mfma_kernel (aid_conv.hip), conv53_dma_kernel (aid_conv_dma.hip),
// conv53_wino4_kernel / conv53_wino4v_kernel (aid_conv_wino.hip) and conv11_dma_kernel (aid_conv1x1_dma.hip).
//
// All five tile a convolution the same way: a tile is M_BLK output channels by N_BLK positions, and the positions are ROWS = N_BLK / TT
// rows of (b, f) by TT samples.  What they share lives here, once: the geometry record and the host function that fills it, the tile
// origin with the XCD-aware order, the row table, the direct-to-LDS piece descriptors of the 5x3 kernels, and the two epilogues.
// K loops, LDS layouts and operand addresses stay with the kernels.
#pragma once
#include "aid_common.h"
#include "aid_mfma_dma.h"

// ---- geometry ----------------------------------------------------------------------------------------------------------------------
struct ConvTileGeo {
    int tt_log2;      // log2(TT)
    int rows_log2;    // log2(ROWS)
    int tiles_t;      // ceil(T / TT)
    int nrows;        // B*F
    int nchunks;      // ceil(Cin / KC)
    int nx, ny;       // position tiles (row groups x tiles_t) and Cout tiles
    int per_xcd;      // > 0: 1-D grid of 8*per_xcd workgroups in the XCD-aware order (conv_tile_origin); 0: plain 2-D grid (nx, ny)
};

// Fills the record from the launch shape and gives the grid.  TT = pow2ceil(T) clamped to [min_tt, N_BLK].  Returns 1000 when the tile would
// span more than RMAX rows (the row table and the halo area hold RMAX rows: the caller falls back), AID_OK otherwise.
// (Chunks are rounded up: the direct-to-LDS kernels only take Cin % KC == 0, where that is the exact quotient.)
static inline int conv_tile_geo(ConvTileGeo* g, dim3* grid, const aid_conv2d_params* p, int N_BLK, int M_BLK, int KC, int RMAX, int min_tt, bool xcd) {
    int TT = aid_pow2ceil(p->T);
    if (TT > N_BLK) TT = N_BLK;
    if (TT < min_tt) TT = min_tt;
    const int ROWS = N_BLK / TT;
    if (ROWS > RMAX) return 1000;
    g->tt_log2 = aid_ilog2(TT);
    g->rows_log2 = aid_ilog2(ROWS);
    g->tiles_t = aid_cdiv(p->T, TT);
    g->nrows = p->B * p->F;
    g->nchunks = aid_cdiv(p->Cin, KC);
    g->nx = aid_cdiv(g->nrows, ROWS) * g->tiles_t;
    g->ny = p->Cout_pad / M_BLK;
    g->per_xcd = xcd ? (int)(((int64_t)g->nx * g->ny + 7) / 8) : 0;
    *grid = xcd ? dim3((unsigned)(8 * g->per_xcd), 1) : dim3((unsigned)g->nx, (unsigned)g->ny);
    return AID_OK;
}

// ---- tile origin and row table -------------------------------------------------------------------------------------------------------
struct ConvTileOrigin { int tile_t, row0, t0, m0; };

// XCD-aware tile order.  Hardware deals consecutive workgroup ids round-robin to the 8 XCDs (each with its own L2).
// Logical tile L = xcd * per_xcd + (id / 8): every XCD walks ONE contiguous range of (row-group, m-tile) pairs, m-tile
// fastest, so the Cout tiles of the same activations and the row groups that share dilated rows meet in the same L2.
// false: this workgroup id lies past the last tile of the padded 1-D grid (the kernel returns).
template <int M_BLK>
__device__ __forceinline__ bool conv_tile_origin(const ConvTileGeo& g, ConvTileOrigin& o) {
    int bx = blockIdx.x, by = blockIdx.y;
    if (g.per_xcd > 0) {
        const int Lt = (blockIdx.x & 7) * g.per_xcd + (blockIdx.x >> 3);
        if (Lt >= g.nx * g.ny) return false;
        bx = Lt / g.ny;
        by = Lt - bx * g.ny;
    }
    o.tile_t = bx % g.tiles_t;
    const int rg = bx / g.tiles_t;
    o.row0 = rg << g.rows_log2;
    o.t0 = o.tile_t << g.tt_log2;
    o.m0 = by * M_BLK;
    return true;
}

// rowinfo[ROWS][2] = (b, f) of the tile's rows, b = -1 past the last row; ends with the barrier that publishes the table
template <int NTHREADS>
__device__ __forceinline__ void conv_tile_rows(const ConvTileGeo& g, int F, int row0, int* rowinfo) {
    const int ROWS = 1 << g.rows_log2;
    for (int r = threadIdx.x; r < ROWS; r += NTHREADS) {
        const int rid = row0 + r;
        int b = -1, f = 0;
        if (rid < g.nrows) { b = rid / F; f = rid - b * F; }
        rowinfo[2 * r] = b;
        rowinfo[2 * r + 1] = f;
    }
    __syncthreads();
}

// ---- direct-to-LDS piece descriptors of the 5x3 kernels --------------------------------------------------------------------------------
// A piece is 1 KiB = one wave-wide 16-byte direct-to-LDS load.  A descriptor is this lane's source for chunk 0, its element advance per
// chunk and the wave-uniform LDS float offset of the piece.  The caller presets (zero page, 0): whatever is out of range keeps reading
// zeros, so every lane of every load is active and no stale LDS data survives.

// Piece wp_ of the weight tile [tap][ci < KC][WROW] from the pack `w` ([tap][Cin_pad][Cout_pad]: p.wp, or the Winograd pack p.wp_wino).
// Columns M_BLK .. WROW of a padded row and the tail past WSZ_RAW stay zero.
template <int KC, int M_BLK, int WROW, int WSZ_RAW>
__device__ __forceinline__ void conv_tile_wpiece(const float* w, const aid_conv2d_params& p, int m0, int wp_, int lane, const float*& src, int& stride) {
    const int e = wp_ * 256 + 4 * lane;         // float offset inside the weight tile
    const int row = e / WROW, col = e % WROW;   // row = tap*KC + ci
    const int tap = row / KC, ci = row % KC;
    if (col < M_BLK && e < WSZ_RAW) {
        src = w + ((int64_t)tap * p.Cin_pad + ci) * p.Cout_pad + m0 + col;
        stride = KC * p.Cout_pad;
    }
}

// Piece `sub` of the N_BLK plain core samples (position n = rr*TT + tt) of block blk = ci*KH + kh
template <int KH, int KC>
__device__ __forceinline__ void conv_tile_xpiece(const aid_conv2d_params& p, const ConvTileGeo& g, const int* rowinfo, int t0, int blk, int sub, int lane,
                                                 const float*& src, int& stride) {
    const int ci = blk / KH, kh = blk % KH;
    const int n = sub * 256 + 4 * lane;
    const int rr = n >> g.tt_log2, tt = n & ((1 << g.tt_log2) - 1);
    const int b = rowinfo[2 * rr];
    const int fi = rowinfo[2 * rr + 1] + (kh - KH / 2) * p.dilF;
    if (b >= 0 && fi >= 0 && fi < p.F && t0 + tt < p.T) {
        src = p.x.p + (int64_t)b * p.x.sB + (int64_t)ci * p.x.sC + (int64_t)fi * p.x.sF + t0 + tt;
        stride = (int)(KC * p.x.sC);
    }
}

// The staging of conv53_dma_kernel and conv53_wino4_kernel: per (ci, kh) block the N_BLK core samples contiguously, then a halo area
// [rr < RMAX][left, right] (one scalar per thread and slot, through a register); behind the x tile the weight tile of TAPS taps.
template <int TAPS, int KC, int M_BLK, int N_BLK, int RMAX, int NW>
struct ConvTileStage {
    static constexpr int KH = 5;
    static constexpr int NTHREADS = 64 * NW;
    static constexpr int XB = N_BLK + 2 * RMAX;                        // floats per (ci,kh) block
    static constexpr int XSZ = KC * KH * XB;
    static constexpr int WROW = (M_BLK % 64 == 0) ? M_BLK : ((M_BLK + 63) / 64) * 64;   // LDS weight row stride (96 -> 128)
    static constexpr int WSZ_RAW = TAPS * KC * WROW;
    static constexpr int WSZ = ((WSZ_RAW + 255) / 256) * 256;          // whole 1-KiB pieces (tail lanes read the zero page)
    static constexpr int BUFSZ = XSZ + WSZ;
    static constexpr int NXP = KC * KH * (N_BLK / 256);                // 1-KiB pieces of the x tile
    static constexpr int NWP = WSZ / 256;                              // 1-KiB pieces of the weight tile
    static constexpr int NP = NXP + NWP;
    static constexpr int PPW = (NP + NW - 1) / NW;                     // pieces per wave per chunk
    static constexpr int HQ = (2 * KC * KH * RMAX + NTHREADS - 1) / NTHREADS;   // halo scalars per thread (ROWS <= RMAX)
    static_assert(N_BLK % 256 == 0, "x tile must be whole 1-KiB pieces");

    const float* psrc[PPW];
    int pstride[PPW], plds[PPW];     // plds: -1 = no piece (wave-uniform)
    const float* hsrc[HQ];
    int hstride[HQ], hlds[HQ];
    float hv[HQ];

    // `wave` must be the readfirstlane value: it keeps plds, and the branch on it in issue_dma, wave-uniform
    __device__ __forceinline__ void init(const aid_conv2d_params& p, const float* w, const float* zero, const ConvTileGeo& g, const int* rowinfo,
                                         int t0, int m0, int wave) {
        const int tid = threadIdx.x, lane = tid & 63;
        const int TT = 1 << g.tt_log2, ROWS = 1 << g.rows_log2;
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const int pc = wave + i * NW;
            psrc[i] = zero; pstride[i] = 0; plds[i] = -1;
            if (pc < NXP) {
                const int blk = pc / (N_BLK / 256), sub = pc % (N_BLK / 256);
                plds[i] = blk * XB + sub * 256;
                conv_tile_xpiece<KH, KC>(p, g, rowinfo, t0, blk, sub, lane, psrc[i], pstride[i]);
            } else if (pc < NP) {
                plds[i] = XSZ + (pc - NXP) * 256;
                conv_tile_wpiece<KC, M_BLK, WROW, WSZ_RAW>(w, p, m0, pc - NXP, lane, psrc[i], pstride[i]);
            }
        }
        const int nhalo = 2 * KC * KH * ROWS;
#pragma unroll
        for (int i = 0; i < HQ; ++i) {
            const int h = tid + i * NTHREADS;
            hsrc[i] = zero; hstride[i] = 0; hlds[i] = -1;
            if (h < nhalo) {
                const int side = h & 1;
                const int rr = (h >> 1) & (ROWS - 1);
                const int blk = (h >> 1) >> g.rows_log2;    // ci*KH + kh
                const int ci = blk / KH, kh = blk % KH;
                const int b = rowinfo[2 * rr];
                const int fi = rowinfo[2 * rr + 1] + (kh - KH / 2) * p.dilF;
                const int t = side ? (t0 + TT) : (t0 - 1);
                hlds[i] = blk * XB + N_BLK + rr * 2 + side;
                if (b >= 0 && fi >= 0 && fi < p.F && t >= 0 && t < p.T) {
                    hsrc[i] = p.x.p + (int64_t)b * p.x.sB + (int64_t)ci * p.x.sC + (int64_t)fi * p.x.sF + t;
                    hstride[i] = (int)(KC * p.x.sC);
                }
            }
        }
    }
    // chunk ch: the pieces go straight into `buf`, the halo scalars into registers
    __device__ __forceinline__ void issue_dma(int ch, float* buf) {
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            if (plds[i] >= 0) {                          // wave-uniform
                const float* src = psrc[i] + (int64_t)ch * pstride[i];
                AID_GLDS16(src, buf + plds[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < HQ; ++i) hv[i] = hsrc[i][(int64_t)ch * hstride[i]];
    }
    __device__ __forceinline__ void write_halo(float* buf) const {
#pragma unroll
        for (int i = 0; i < HQ; ++i)
            if (hlds[i] >= 0) buf[hlds[i]] = hv[i];
    }
};

// ---- scalar epilogue: y = alpha * (res_scale*res + acc*out_scale[b,co]), or the dGELU form (epi = 1); one sample per lane and row ------
// (conv_mfma_kernel and conv53_dma_kernel; MT x NT tiles of 32 x 32 per wave, WGM x WGN waves)
// `raw(j, b, f, t)`: the kernel's own store of position tile j, true when it took the tile (the split-K partial sums of conv_mfma_kernel).  It is asked
// per tile, inside the loop: with the split-K branch in front of the whole loop the register-staged instances lost a wave per SIMD (128 -> 132 VGPRs).
struct ConvTileNoRaw { __device__ __forceinline__ bool operator()(int, int, int, int) const { return false; } };
template <int MT, int NT, int WGM, int WGN, typename Raw = ConvTileNoRaw>
__device__ __forceinline__ void conv_tile_epilogue(const aid_conv2d_params& p, const ConvTileGeo& g, const ConvTileOrigin& o, const int* rowinfo, int wave,
                                                   const f32x16 (&acc)[MT][NT], Raw raw = Raw()) {
    const int lane = threadIdx.x & 63;
    const int wm = wave / WGN, wn = wave % WGN;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = (wn * NT + j) * 32 + (lane & 31);
        const int rr = n >> g.tt_log2;
        const int tt = n & ((1 << g.tt_log2) - 1);
        const int b = rowinfo[2 * rr];
        const int f = rowinfo[2 * rr + 1];
        const int t = o.t0 + tt;
        if (b < 0 || t >= p.T) continue;
        if (raw(j, b, f, t)) continue;
        const int64_t ybase = (int64_t)b * p.y.sB + (int64_t)f * p.y.sF + t;
        const int64_t rbase = p.res.p ? ((int64_t)b * p.res.sB + (int64_t)f * p.res.sF + t) : 0;
        const int64_t abase = p.aux.p ? ((int64_t)b * p.aux.sB + (int64_t)f * p.aux.sF + t) : 0;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            // gather phase first (res / aux / gate), then compute + store: res may alias y (gradient accumulation),
            // so the compiler would otherwise serialise load -> store element by element (16 dependent round trips)
            float rv[16], uv[16], sv[16];
            const int mbase = o.m0 + (wm * MT + i) * 32 + 4 * (lane >> 5);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mbase + (r & 3) + 8 * (r >> 2);
                const bool ok = m < p.Cout;
                rv[r] = (ok && p.res.p) ? p.res.p[rbase + (int64_t)m * p.res.sC] : 0.f;
                sv[r] = (ok && p.out_scale) ? p.out_scale[(int64_t)b * p.out_scale_ld + m] : 1.f;
                uv[r] = (ok && p.epi == 1) ? p.aux.p[abase + (int64_t)m * p.aux.sC] * p.aux_scale[(int64_t)b * p.aux_scale_ld + m] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mbase + (r & 3) + 8 * (r >> 2);
                if (m >= p.Cout) continue;
                float v = acc[i][j][r] * sv[r];
                if (p.epi == 1) v *= aid_dgelu(uv[r]);
                v += p.res_scale * rv[r];
                p.y.p[ybase + (int64_t)m * p.y.sC] = p.alpha * v;
            }
        }
    }
}

// ---- F(4,3) epilogue: output transform, then gate / dGELU / residual, four samples per lane; optionally <y, aux> partials ----------------
// (conv53_wino4_kernel and conv53_wino4v_kernel; acc[i][j][xi] = M_xi of 32 rows x 32 groups of 4 outputs.)
//   y0 = M0+M1+M2+M3+M4, y1 = (M1-M2)+2(M3-M4), y2 = (M1+M2)+4(M3+M4), y3 = (M1-M2)+8(M3-M4)+M5
// `wave`: the readfirstlane value.  `red`: LDS no wave reads any more (every wave is past the last chunk's barrier), 8 * NW * MT floats for the partials.
template <int MT, int NTT, int WGM, int WGN>
__device__ __forceinline__ void wino4_tile_epilogue(const aid_conv2d_params& p, const ConvTileGeo& g, const ConvTileOrigin& o, const int* rowinfo, float* red,
                                                    int wave, const f32x16 (&acc)[MT][NTT][6]) {
    constexpr int NW = WGM * WGN, M_BLK = 32 * MT * WGM;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wm = wave / WGN, wn = wave % WGN;
    const int half = lane >> 5;
    const int ttau_log2 = g.tt_log2 - 2;                 // groups per row = TT/4
    float dsum[MT][4];                                   // <y, aux> per block of 4 rows (dot_ws)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) dsum[i][q] = 0.f;
#pragma unroll
    for (int j = 0; j < NTT; ++j) {
        const int nt = (wn * NTT + j) * 32 + (lane & 31);
        const int rr = nt >> ttau_log2, tau = nt & ((1 << ttau_log2) - 1);
        const int b = rowinfo[2 * rr];
        const int f = rowinfo[2 * rr + 1];
        const int t = o.t0 + 4 * tau;
        if (b < 0 || t >= p.T) continue;                 // T % 4 == 0: the four samples are in range together
        const int64_t ybase = (int64_t)b * p.y.sB + (int64_t)f * p.y.sF + t;
        const int64_t rbase = p.res.p ? ((int64_t)b * p.res.sB + (int64_t)f * p.res.sF + t) : 0;
        const int64_t abase = p.aux.p ? ((int64_t)b * p.aux.sB + (int64_t)f * p.aux.sF + t) : 0;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int mbase = o.m0 + (wm * MT + i) * 32 + 4 * half;
#pragma unroll
            for (int r0 = 0; r0 < 16; r0 += 4) {         // batches of 4 rows: gather, then compute + store (res may alias y)
                float4 rv[4], ur[4];                      // residual, raw aux (scaled by `as` when the dGELU is evaluated)
                float sv[4], as[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int r = r0 + q;
                    const int m = mbase + (r & 3) + 8 * (r >> 2);
                    const bool ok = m < p.Cout;
                    rv[q] = (ok && p.res.p) ? *reinterpret_cast<const float4*>(p.res.p + rbase + (int64_t)m * p.res.sC) : make_float4(0.f, 0.f, 0.f, 0.f);
                    sv[q] = (ok && p.out_scale) ? p.out_scale[(int64_t)b * p.out_scale_ld + m] : 1.f;
                    if (ok && p.epi == 1) {
                        as[q] = p.aux_scale[(int64_t)b * p.aux_scale_ld + m];
                        ur[q] = *reinterpret_cast<const float4*>(p.aux.p + abase + (int64_t)m * p.aux.sC);
                    } else { as[q] = 0.f; ur[q] = make_float4(0.f, 0.f, 0.f, 0.f); }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int r = r0 + q;
                    const int m = mbase + (r & 3) + 8 * (r >> 2);
                    if (m >= p.Cout) continue;
                    const float M0 = acc[i][j][0][r], M1 = acc[i][j][1][r], M2 = acc[i][j][2][r], M3 = acc[i][j][3][r],
                                M4 = acc[i][j][4][r], M5 = acc[i][j][5][r];
                    const float a12 = M1 + M2, s12 = M1 - M2, a34 = M3 + M4, s34 = M3 - M4;
                    float y0 = (M0 + a12 + a34) * sv[q];
                    float y1 = (s12 + 2.f * s34) * sv[q];
                    float y2 = (a12 + 4.f * a34) * sv[q];
                    float y3 = (s12 + 8.f * s34 + M5) * sv[q];
                    if (p.epi == 1) { y0 *= aid_dgelu(ur[q].x * as[q]); y1 *= aid_dgelu(ur[q].y * as[q]); y2 *= aid_dgelu(ur[q].z * as[q]); y3 *= aid_dgelu(ur[q].w * as[q]); }
                    y0 += p.res_scale * rv[q].x; y1 += p.res_scale * rv[q].y; y2 += p.res_scale * rv[q].z; y3 += p.res_scale * rv[q].w;
                    y0 *= p.alpha; y1 *= p.alpha; y2 *= p.alpha; y3 *= p.alpha;
                    *reinterpret_cast<float4*>(p.y.p + ybase + (int64_t)m * p.y.sC) = make_float4(y0, y1, y2, y3);
                    if (p.dot_ws) dsum[i][r0 >> 2] += (y0 * ur[q].x + y1 * ur[q].y) + (y2 * ur[q].z + y3 * ur[q].w);
                }
            }
        }
    }
    // ---- optional: <y, aux> per (sample, channel group), one partial per tile (replaces the aid_group_dot pass) -----------
    if (p.dot_ws) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float v = dsum[i][q];
#pragma unroll
                for (int off = 16; off >= 1; off >>= 1) v += __shfl_xor(v, off, 32);     // the 32 lanes of a half-wave share their rows
                dsum[i][q] = v;
            }
        if ((lane & 31) == 0) {
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) red[((wave * 2 + half) * MT + i) * 4 + q] = dsum[i][q];
        }
        __syncthreads();
        const int cpg = p.Cout >> 3;                     // channels per group (8 groups); M_BLK % cpg == 0 (host-checked)
        const int grp = o.m0 / cpg + tid;
        if (tid < M_BLK / cpg && grp < 8) {
            float sacc = 0.f;
#pragma unroll 1                                         // (a few lanes, once per tile: unrolled it is 300 instructions in every instance)
            for (int w = 0; w < NW; ++w)                 // fixed order: deterministic
                for (int h = 0; h < 2; ++h)
                    for (int i = 0; i < MT; ++i)
                        for (int q = 0; q < 4; ++q) {
                            const int mrow = o.m0 + ((w / WGN) * MT + i) * 32 + 4 * h + 8 * q;
                            if (mrow / cpg == grp) sacc += red[((w * 2 + h) * MT + i) * 4 + q];
                        }
            const int b = rowinfo[0];
            const int ptile = ((o.row0 - b * p.F) >> g.rows_log2) * g.tiles_t + o.tile_t;
            p.dot_ws[((int64_t)b * 8 + grp) * p.dot_n + ptile] = (double)sacc;
        }
    }
}
