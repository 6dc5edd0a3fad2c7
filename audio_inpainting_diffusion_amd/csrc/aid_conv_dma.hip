// conv53_dma_kernel: the 5x3 dilated dense convolution (plain-copy prologue) with DIRECT-TO-LDS staging.
//
// Same GEMM decomposition and epilogue as conv_mfma_kernel (aid_conv.hip), but for the shapes that carry the
// FLOPs (KH=5, KW=3, Cin % 4 == 0, no in-kernel prologue because aid_scale_act ran first):
//   * both operands travel HBM/L2 -> LDS with `global_load_lds_dwordx4` (1 KiB per wave-instruction, no VGPR
//     round trip, no ds_write, no VALU besides one 64-bit pointer bump per piece per chunk).  The LDS image
//     is therefore lane-linear: the x tile stores, per (ci, kh), the N_BLK core samples of the tile
//     CONTIGUOUSLY (position n = rr*TT + tt) followed by a small halo area [rr][left,right]; out-of-range
//     rows / columns / channels are sourced from a device zero page instead of being masked, so every lane of
//     every DMA is active and no stale LDS data survives;
//   * with the core region a compile-time constant per (ci,kh), every operand ds_read is `vaddr + immediate`:
//     the per-lane addresses (incl. the halo redirection of the tile-edge lanes for kw = 0/2) are computed once,
//     so the steady-state loop is [ds_read_b32, v_mfma] plus 3-5 DMA issues per wave per chunk;
//   * double-buffered LDS, DMA of chunk c+1 issued right after the barrier that closes chunk c-1, one
//     `__syncthreads()` (vmcnt(0) + barrier) per chunk, priority-based progress balancing between the waves
//     of a SIMD (see aid_conv.hip).
// Tile origin, row table, the piece / halo descriptors with issue_dma / write_halo (ConvTileStage) and the epilogue are the
// shared frame of aid_conv_tile.h; this file keeps the operand addresses, the K loop and the launcher.
#include "aid_conv_tile.h"
#include <type_traits>
#include <stdlib.h>

struct ConvDmaDev {
    aid_conv2d_params p;
    const float* zero;   // >= 64 B of zeros in global memory
    ConvTileGeo g;
};

template <int MT, int NT, int WGM, int WGN, int RMAX, int KC, int MINW>
__global__ __launch_bounds__(64 * WGM * WGN, MINW) void conv53_dma_kernel(const ConvDmaDev a) {
    constexpr int KH = 5, KW = 3, TAPS = 15;
    constexpr int NW = WGM * WGN;
    constexpr int M_BLK = 32 * MT * WGM;
    constexpr int N_BLK = 32 * NT * WGN;
    using Stage = ConvTileStage<TAPS, KC, M_BLK, N_BLK, RMAX, NW>;     // the LDS image of a buffer and its DMA pieces (aid_conv_tile.h)
    constexpr int XB = Stage::XB, XSZ = Stage::XSZ, WROW = Stage::WROW, BUFSZ = Stage::BUFSZ;

    const aid_conv2d_params& p = a.p;
    const int TT = 1 << a.g.tt_log2;

    extern __shared__ __attribute__((aligned(16))) float smem[];
    int* rowinfo = (int*)(smem + 2 * BUFSZ);            // [ROWS][2] = (b, f) or b = -1

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WGN;
    const int wn = wave % WGN;

    ConvTileOrigin o;
    if (!conv_tile_origin<M_BLK>(a.g, o)) return;
    conv_tile_rows<64 * NW>(a.g, p.F, o.row0, rowinfo);

    Stage st;                                            // piece and halo descriptors (per lane, constant over the K loop)
    st.init(p, p.wp, a.zero, a.g, rowinfo, o.t0, o.m0, wave);
    // ---- operand addresses (LDS float offsets inside a buffer; ci / kh / tap terms are immediates) -----------
    const int half = lane >> 5;                          // which of the two ci of a k-step this lane feeds
    int vB[NT][KW];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = (wn * NT + j) * 32 + (lane & 31);
        const int rr = n >> a.g.tt_log2, tt = n & (TT - 1);
#pragma unroll
        for (int kw = 0; kw < KW; ++kw) {
            const int tc = tt + kw - 1;
            int off = n + kw - 1;
            if (tc < 0) off = N_BLK + rr * 2;
            else if (tc >= TT) off = N_BLK + rr * 2 + 1;
            vB[j][kw] = half * KH * XB + off;
        }
    }
    int vA[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) vA[i] = XSZ + half * WROW + (wm * MT + i) * 32 + (lane & 31);

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    st.issue_dma(0, smem);
    st.write_halo(smem);
    __syncthreads();

    auto chunk = [&](auto curc, int ch) {
        constexpr int cur = decltype(curc)::value;
        const float* Bf = smem + cur * BUFSZ;
        float* Nx = smem + (cur ^ 1) * BUFSZ;
        const bool more = (ch + 1) < a.g.nchunks;
        if (more) st.issue_dma(ch + 1, Nx);
        float av[2][MT], bv[2][NT];
        auto load_frags = [&](int ks, int buf) {
            const int tap = ks / (KC / 2), cp = ks % (KC / 2);
            const int kh = tap / KW, kw = tap % KW;
#pragma unroll
            for (int i = 0; i < MT; ++i) av[buf][i] = Bf[vA[i] + (tap * KC + 2 * cp) * WROW];
#pragma unroll
            for (int j = 0; j < NT; ++j) bv[buf][j] = Bf[vB[j][kw] + (2 * cp * KH + kh) * XB];
        };
        load_frags(0, 0);
#pragma unroll
        for (int ks = 0; ks < TAPS * (KC / 2); ++ks) {
            if (ks == 0) __builtin_amdgcn_s_setprio(3);
            else if (ks == 3 * (KC / 2)) __builtin_amdgcn_s_setprio(2);
            else if (ks == 6 * (KC / 2)) __builtin_amdgcn_s_setprio(1);
            else if (ks == 9 * (KC / 2)) __builtin_amdgcn_s_setprio(0);
            if (ks + 1 < TAPS * (KC / 2)) load_frags(ks + 1, (ks + 1) & 1);
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ks & 1][i], bv[ks & 1][j], acc[i][j], 0, 0, 0);
        }
        if (more) st.write_halo(Nx);
        __syncthreads();
    };
    for (int ch = 0; ch < a.g.nchunks; ch += 2) {
        chunk(std::integral_constant<int, 0>{}, ch);
        if (ch + 1 < a.g.nchunks) chunk(std::integral_constant<int, 1>{}, ch + 1);
    }
    __builtin_amdgcn_s_setprio(0);

    conv_tile_epilogue<MT, NT, WGM, WGN>(p, a.g, o, rowinfo, wave, acc);
}

template <int MT, int NT, int WGM, int WGN, int RMAX, int KC = 4, int MINW = 1>
static int launch_dma(const aid_conv2d_params* p, hipStream_t st) {
    constexpr int M_BLK = 32 * MT * WGM;
    constexpr int N_BLK = 32 * NT * WGN;
    ConvDmaDev a;
    a.p = *p;
    a.zero = aid_zero_page();
    if (!a.zero) return AID_E_LAUNCH;
    dim3 grid;
    if (conv_tile_geo(&a.g, &grid, p, N_BLK, M_BLK, KC, RMAX, 1, false) == 1000) return 1000;      // halo area holds RMAX rows: caller falls back
    const size_t lds = sizeof(float) * 2 * (size_t)ConvTileStage<15, KC, M_BLK, N_BLK, RMAX, WGM * WGN>::BUFSZ + sizeof(int) * 2 * ((size_t)1 << a.g.rows_log2);
    auto kern = conv53_dma_kernel<MT, NT, WGM, WGN, RMAX, KC, MINW>;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set = true;
    }
    hipLaunchKernelGGL(kern, grid, dim3(64 * WGM * WGN), lds, st, a);
    AID_CHECK_LAUNCH();
    aid_note_kernel("conv53_dma_kernel");
    return AID_OK;
}

// returns 1 if the DMA kernel took the launch, 0 if the shape is not eligible, <0 on error
int aid_conv53_dma_try(const aid_conv2d_params* p, hipStream_t st) {
    if (!(p->KH == 5 && p->KW == 3) || p->in_scale || p->act != 0) return 0;
    if ((p->Cin % 4) != 0 || p->Cout < 64 || (p->T % 4) != 0) return 0;
    const int TT = aid_pow2ceil(p->T);
    if (TT < 8) return 0;                                  // ROWS <= 32 (halo area)
    if (!aid_view_aligned(p->x, 4)) return 0;
    if ((int64_t)4 * p->x.sC >= (1LL << 31)) return 0;
    int rc;
    // (round-1 experiments with 4/16-wave tiles, KC = 2 and 3-4 workgroups per CU are recorded in DESIGN.md section 3.1)
    if (p->Cout_pad % 64 == 0)       rc = launch_dma<1, 2, 2, 4, 16>(p, st);     //  64 x 256, 8 waves, 2 workgroups per CU
    else if (p->Cout_pad % 96 == 0)  rc = launch_dma<1, 2, 3, 4, 32>(p, st);     //  96 x 256, 12 waves
    else return 0;
    if (rc == 1000) return 0;
    return rc == AID_OK ? 1 : rc;
}
