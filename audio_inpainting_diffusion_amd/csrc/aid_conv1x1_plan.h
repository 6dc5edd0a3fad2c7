// Which kernel serves one 1x1 convolution launch, and with what geometry (aid_conv1x1_rs.hip, aid_conv1x1_dma.hip, aid_conv1x1.hip and the 1x1 side of
// aid_conv.hip).  Host only, plain C++17, scalars only -- no aid_conv2d_params, no pointers, no HIP: the launchers, aid_conv2d's dispatch and the host
// queries (aid_conv2d_dot_partials_1x1, aid_conv2d_x2_supported) read ONE C11Plan, so the <y, aux> partial slots a launch writes and the slots the caller
// allocated for it are the same number by construction.  What only a launch knows (view and weight-pack alignment, the 32-bit offset limits,
// dot_n == slots, the alignment of y and res for the split-K reduction) stays with the aid_conv1x1_*_try functions.
//
// aid_conv2d tries the families in the order rs, dma (tiles | skinny GEMM | GEMM with K split), stream, tiled; c11_plan is that chain on scalars.
// Counts that can exceed an int (B * F, B * T, F * T, nx * ny, scratch bytes) are formed in 64 bits; a family whose int fields would not hold them declines.
#pragma once
#include <stdint.h>
#include <stdlib.h>

enum { C11_TILED = 0, C11_RS, C11_DMA, C11_SKINNY, C11_DMA_SPLITK, C11_STREAM };

struct C11Shape {
    int B, Cin, Cin1, Cout, Cout_pad, F, T;      // Cin1: channels served by the first tensor of a two-tensor K axis (read when x2)
    int act, epi;
    bool in_scale, res, x2, dot;                 // dot: <y, aux> partials are asked for
    bool ws;                                     // scratch is offered, of ws_bytes
    int64_t ws_bytes;
};

struct C11Plan {
    int family;
    bool ok;                       // false (family C11_TILED only): refused -- x2 / dot with neither of the first two families, or a count beyond the tiled kernel's ints
    // the instance: rs <MT, KMAX, key = ACT 8 | SCALE 4 | EPI 2 | RES 1>; dma <MT = 2 | 1 | 3: the 128 | 64 | 96-wide tile>; skinny <nt>; stream <MT, nt>;
    // tiled <WGM = rows of the M tile / 32, KC = channels per chunk>
    int MT, KMAX, key, WGM, KC;
    int slots;                     // <y, aux> partial slots per (sample, group) when dot is asked for, else 0
    // dma: positions per tile row, rows per tile, tiles along T, position tiles, Cout tiles, 16-channel chunks (all / of the first tensor)
    int TT, ROWS, tiles_t, nrows, nx, ny, nchunks, nch1;
    int S, kps;                    // dma GEMM, skinny, tiled: K ranges and channels per range (S = 1: single pass)
    int tps, ntiles, gx;           // rs: 64-position tiles per sample, all tiles, workgroups along x (capped); skinny: gx workgroups of four 32-row tiles
    int nsteps1;                   // rs: k-pairs served by the first tensor
    int nt, mchunks;               // stream: positions per lane (2 | 4), Cout slices; skinny: nt column tiles per wave
    int64_t npos, pblocks;         // stream: B * F * T and blocks of 4 waves x 32 nt positions
};

static inline int64_t c11_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Cout tile of the weight pack (aid_conv2d_pack_dims pads Cout to a multiple of it) and of the tiled kernel
static inline int c11_pick_mblk(int Cout) {
    if (Cout <= 32) return 32;
    if (Cout <= 64) return 64;
    if (Cout <= 96 || (Cout % 96 == 0 && Cout % 128 != 0)) return 96;   // 96, 192, 288: no padded rows
    return 128;
}

// The split-K scratch rule, pure half: S partial planes [B][Cout][F][T] of floats fit ws_bytes (a1 ... ak <= n  <=>  a1 <= floor(... floor(n / ak) ...):
// no product is formed).  The launch adds the 16-byte alignment of y and res for the reduction (aid_conv_splitk_scratch_ok).
static inline bool c11_splitk_fits(int S, int B, int Cout, int F, int T, int64_t ws_bytes) {
    if (S < 1 || B < 1 || Cout < 1 || F < 1 || T < 1 || ws_bytes < 0) return false;
    return (int64_t)S <= ws_bytes / 4 / T / F / Cout / B;
}

// K partition of the qk GEMMs: a function of K ALONE -- the skinny kernel (N <= 128) and the tiled kernel (any N) then add the same k-pairs in
// the same order into the same number of partial planes, so a segment's result does not depend on the batch it is evaluated in.
static inline void c11_gemm_k_partition(int Cin, int* S, int* kps) {
    int s = 8;
    if (s > Cin / 64) s = Cin / 64;
    if (s < 1) s = 1;
    int cps = (int)c11_cdiv(c11_cdiv(Cin, 16), s);     // 16-channel chunks per range, even (two LDS buffers alternate from the first chunk)
    cps += cps & 1;
    *kps = cps * 16;
    *S = (int)c11_cdiv(Cin, *kps);
}

// The AID_C11_RS switch of -DAID_EXPERIMENT builds (tools/c11_probe.py, tools/r03_c11_ab.sh): 0 takes the register-streamed kernel out of the chain.
static inline bool c11_rs_enabled() {
#ifdef AID_EXPERIMENT
    static const int enabled = getenv("AID_C11_RS") ? atoi(getenv("AID_C11_RS")) : 1;
    return enabled != 0;
#else
    return true;
#endif
}

static inline C11Plan c11_none() { C11Plan pl = {}; pl.ok = true; return pl; }

// ---- rs: conv11_rs_kernel<MT, KMAX, ACT, SCALE, EPI, RES> -------------------------------------------------------------------------------------------
// Which layers (a function of the per-sample shape only, so that a segment's result does not depend on its batch): measured per shape at batch 8 AND
// batch 1 against the tile kernels (profiles/r03_trace_b8.txt / _b1.txt before and after): 96 output channels (MT = 3) win for every K <= 256
// (batch 8: -12 ... -32 %); 64 output channels (MT = 2) win at K = 64 and lose at K = 128 / 192 (more waves would be needed to cover the longer K
// loop's exposed first block); 128-channel slices (MT = 4: 128 accumulators + the epilogue's gather registers, 64-128 KB of weights per workgroup)
// lose on the small pyramid levels by 2x (32 ... 128 tiles per sample: one wave per tile, most SIMDs idle) and are not instantiated.
// The <y, aux> partials are one per 64-position tile; their group rule (Cout % 8 == 0, 4 | Cout / 8 | tile) holds for both Cout = 64 and 96.
static inline C11Plan c11_rs_plan(const C11Shape& s) {
    C11Plan pl = c11_none();
    if (!c11_rs_enabled() || s.ws || (s.act && !s.in_scale) || s.Cout != s.Cout_pad) return pl;
    if (s.F <= 1 || s.Cin < 32 || (s.Cin % 32) || s.Cin > 256 || s.Cout < 32) return pl;
    if (!(s.Cout_pad == 96 || (s.Cout_pad == 64 && s.Cin <= 64))) return pl;
    const int64_t ft = (int64_t)s.F * s.T;
    if ((s.T % 2) || (ft % 64)) return pl;
    if (ft / 64 > INT32_MAX) return pl;
    const int64_t ntiles = s.B * (ft / 64);
    if (ntiles + 8 * 256 > INT32_MAX) return pl;        // (the kernel's tile loop steps an int by at most 8 waves x 256 workgroups)
    if (s.x2 && ((s.Cin1 % 2) || s.Cin1 <= 0 || s.Cin1 >= s.Cin || s.in_scale || s.act)) return pl;
    const int key = (s.act ? 8 : 0) | (s.in_scale ? 4 : 0) | (s.epi == 1 ? 2 : 0) | (s.res ? 1 : 0);
    if (!(key <= 6 || key == 12 || key == 13)) return pl;      // (the combinations the network emits; anything else goes to the tile kernels)
    if (s.dot && s.epi != 1) return pl;
    const int MT = s.Cout_pad / 32;
    pl.MT = MT; pl.KMAX = (MT == 3 && s.Cin > 128) ? 256 : 128; pl.key = key;
    pl.tps = (int)(ft / 64);
    pl.ntiles = (int)ntiles;
    pl.nsteps1 = (s.x2 ? s.Cin1 : s.Cin) / 2;
    pl.ny = s.Cout_pad / (32 * MT);
    const int cap = pl.ny > 1 ? 256 / pl.ny + (256 % pl.ny ? 1 : 0) : 256;      // one workgroup per CU over all Cout slices
    pl.gx = (int)c11_cdiv(ntiles, 8);
    if (pl.gx > cap) pl.gx = cap;
    pl.slots = s.dot ? pl.tps : 0;
    pl.family = C11_RS;
    return pl;
}

// ---- dma: conv11_dma_kernel<MT, WGM, WGN = 4, RMAX = 16, KC = 16, MINW> and, for the qk GEMMs (F = 1), gemm_skinny_kernel<NT> ----------------------
// Tiles of 256 positions = ROWS rows x TT samples; K is walked in whole 16-channel chunks (no ragged tail).  Cout tile: 128 x 256 (8 waves, 2 workgroups
// / CU), else 64 x 256, else 96 x 256 (4 waves).  The qk projections (F = 1) are a plain GEMM with N = B * T columns on the 128-wide tile: grid-starved,
// so K is split over several workgroups per tile when the scratch is there (deterministic fixed-order reduction); with N <= 128 columns the skinny
// kernel takes them: a wave per 32 rows and K range.
static inline C11Plan c11_dma_plan(const C11Shape& s) {
    C11Plan pl = c11_none();
    if (s.act != 0 || s.Cin < 32 || (s.Cin % 16) || s.Cout < 32) return pl;
    const bool gemm = s.F == 1;
    if (gemm && (s.epi != 0 || s.in_scale || s.x2 || (s.Cout_pad % 128) || s.Cin < 256)) return pl;
    if ((s.T % 4) || s.T < 8) return pl;                                       // (T % 4 == 0 and pow2ceil(T) >= 8)
    if (s.x2 && ((s.Cin1 % 16) || s.Cin1 <= 0 || s.Cin1 >= s.Cin || s.in_scale)) return pl;
    int TT = 8;
    while (TT < 256 && TT < s.T) TT *= 2;                                      // min(pow2ceil(T), 256)
    const int ROWS = 256 / TT;
    // a tile (256 positions) must stay inside one sample when a per-(b,ci) scale is applied to the weights
    if (ROWS > 16 || (s.in_scale && (s.F % ROWS))) return pl;
    const int mblk = (s.Cout_pad % 128 == 0) ? 128 : ((s.Cout_pad % 64 == 0) ? 64 : ((s.Cout_pad % 96 == 0) ? 96 : 0));
    if (!mblk) return pl;
    const int tiles_t = (int)c11_cdiv(s.T, TT);
    if (s.dot) {                                                               // one partial per position tile of a sample, per group of Cout / 8 channels
        const int cpg = s.Cout / 8;
        if (s.epi != 1 || s.x2 || gemm || (s.Cout % 8) || (cpg % 4) || (mblk % cpg) || (s.F % ROWS)) return pl;
        if ((int64_t)(s.F / ROWS) * tiles_t > INT32_MAX) return pl;
        pl.slots = (s.F / ROWS) * tiles_t;
    }
    const int64_t nrows = (int64_t)s.B * s.F;
    const int64_t nx = nrows > INT32_MAX ? INT32_MAX : c11_cdiv(nrows, ROWS) * tiles_t;
    if (nx > (INT32_MAX - 7) / (s.Cout_pad / mblk)) { pl.slots = 0; return pl; }      // (the kernel walks 8 * ceil(nx ny / 8) tiles in an int)
    pl.TT = TT; pl.ROWS = ROWS; pl.tiles_t = tiles_t;
    pl.nrows = (int)nrows; pl.nx = (int)nx; pl.ny = s.Cout_pad / mblk;
    pl.nchunks = s.Cin / 16;
    pl.nch1 = s.x2 ? s.Cin1 / 16 : pl.nchunks;
    pl.S = 1; pl.kps = s.Cin;
    pl.MT = mblk == 128 ? 2 : (mblk == 64 ? 1 : 3);                            // <2, 2, 4, 16, 16, 4> | <1, 2, 4, 16, 16, 4> | <3, 1, 4, 16, 16, 2>
    pl.family = C11_DMA;
    if (gemm) {
        int S, kps;
        c11_gemm_k_partition(s.Cin, &S, &kps);
        if (S > 1 && s.ws && c11_splitk_fits(S, s.B, s.Cout, s.F, s.T, s.ws_bytes)) {
            pl.S = S; pl.kps = kps;
            pl.family = C11_DMA_SPLITK;
            if ((int64_t)s.B * s.T <= 128) {                                   // skinny GEMM: enough K ranges for ~2000 waves, as the scratch allows
                pl.family = C11_SKINNY;
                pl.nt = (int)c11_cdiv((int64_t)s.B * s.T, 32);
                pl.gx = (int)c11_cdiv(s.Cout_pad / 32, 4);
            }
        }
    }
    return pl;
}

// ---- stream: conv1x1_stream_kernel<MT, NT, PF = 4, MINW = 2> ----------------------------------------------------------------------------------------
// measured (profiles/r01_conv1x1_probe.txt): ahead of the register-staged tiled kernel for the short-K / write-dominated
// projections (Cin <= 96: 8-35 %), behind it (10-18 %) once K >= 256 makes the layer MFMA-bound; the direct-to-LDS kernel
// (aid_conv1x1_dma.hip, tried first) is 17-20 % ahead of this one wherever it is eligible, so this kernel serves the shapes
// that one refuses (K % 16 != 0, Cout tiles of 32).  128 positions per wave (float4 traffic) when the geometry allows, else 64.
static inline C11Plan c11_stream_plan(const C11Shape& s) {
    C11Plan pl = c11_none();
    if (s.act != 0 || s.Cin < 16 || (s.Cin & 1) || s.Cout < 32) return pl;
    const int64_t ft = (int64_t)s.F * s.T;
    if (s.F == 1 || s.B > INT64_MAX / ft || s.B * ft < 2048) return pl;       // few positions (qk GEMMs, F = 1): the tiled kernel's job
    if (!(s.Cin <= 96 || s.Cout_pad <= 32)) return pl;
    int nt = 4;
    if ((ft % 128) || (s.T % 4)) nt = 2;
    if ((ft % (32 * nt)) || (s.T % nt)) return pl;                             // a wave's positions stay inside one sample b, vectors inside one row
    const int mt32 = s.Cout_pad / 32;
    // nt = 2: 128-wide slices, 2 waves / SIMD; 96-wide (Cout 96, 192), 3 waves / SIMD
    const int MT = nt == 4 ? (mt32 % 2 == 0 ? 2 : 1) : (mt32 % 4 == 0 ? 4 : (mt32 % 3 == 0 ? 3 : (mt32 % 2 == 0 ? 2 : 1)));
    pl.npos = s.B * ft;
    pl.mchunks = mt32 / MT;
    pl.pblocks = c11_cdiv(pl.npos, 4 * 32 * nt);
    if (pl.pblocks > INT32_MAX / pl.mchunks) return pl;                        // (the grid: pblocks * mchunks workgroups)
    pl.nt = nt;
    pl.MT = MT;
    pl.family = C11_STREAM;
    return pl;
}

// ---- tiled: conv_mfma_kernel<1, 1, 1, 2, WGM, 4, KC>, M tile 32 WGM x 256 positions -----------------------------------------------------------------
static inline C11Plan c11_tiled_plan(const C11Shape& s) {
    C11Plan pl = c11_none();
    const int KC = s.Cin <= 8 ? 8 : 16;
    int mb = c11_pick_mblk(s.Cout);
    pl.S = 1;
    const int64_t nrows = (int64_t)s.B * s.F;
    int TT = 4;
    while (TT < 256 && TT < s.T) TT *= 2;
    pl.ok = nrows <= INT32_MAX && c11_cdiv(nrows, 256 / TT) * c11_cdiv(s.T, TT) <= INT32_MAX;
    if (pl.ok && mb == 128) {
        // grid-starved GEMMs (qk projections: N = B*T columns only)
        int64_t ntiles = c11_cdiv(nrows * s.T, 256);
        if (ntiles > 384) ntiles = 384;                                        // (only compared with 192 and 384: keeps the products below small)
        const int64_t wg64 = ntiles * (s.Cout_pad / 64);
        if (s.ws && s.epi == 0 && wg64 < 384 && s.Cin >= 16 * KC && s.Cout_pad % 64 == 0 && (s.T % 4) == 0) {
            // split K over several workgroups per 64 x 256 tile (deterministic two-pass reduction through ws)
            int S = (int)((768 + wg64 - 1) / wg64);
            if (S > 8) S = 8;
            if (S > 1 && c11_splitk_fits(S, s.B, s.Cout, s.F, s.T, s.ws_bytes)) { pl.S = S; mb = 64; }
        }
        // single pass: trade tile height for more workgroups
        if (pl.S == 1 && ntiles * (s.Cout_pad / 128) < 192) mb = (ntiles * (s.Cout_pad / 64) < 192) ? 32 : 64;
    }
    pl.WGM = mb / 32; pl.KC = KC;                                              // more waves per CU for the short-K (memory-bound) channel projections
    return pl;
}

static inline C11Plan c11_plan(const C11Shape& s) {
    C11Plan pl = c11_rs_plan(s);
    if (!pl.family) pl = c11_dma_plan(s);
    if (!pl.family && (s.x2 || s.dot)) pl.ok = false;                         // (x2 and dot are options of the first two families only)
    else if (!pl.family) pl = c11_stream_plan(s);
    if (!pl.family && pl.ok) pl = c11_tiled_plan(s);
    return pl;
}

// the scalars of a launch (P: aid_conv2d_params; a template so that this header needs no other)
template <class P> static inline C11Shape c11_shape_of(const P& p) {
    C11Shape s = {p.B, p.Cin, p.Cin1, p.Cout, p.Cout_pad, p.F, p.T, p.act, p.epi, p.in_scale != nullptr, p.res.p != nullptr, p.x2.p != nullptr, p.dot_ws != nullptr,
                  p.ws != nullptr, p.ws_bytes};
    return s;
}
