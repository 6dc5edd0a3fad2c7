// Tile geometry of one launch of the row-shared Winograd kernels (aid_conv_wino.hip: conv53_wino4r_kernel / conv53_wino8r_kernel and their
// split-K, K-group and pair instances).  Host only, plain C++17: the launcher, the form choice and every host query read ONE WinoRPlan, so the
// partial slots a launch writes and the slots the caller allocated for it are the same number by construction.
//
// A tile is 64 output channels x `npos` positions = RA rows of each of NC adjacent residue classes of the dilation (f, f + d, f + 2 d, ...) x TT
// samples.  96-channel layers take two tile families in one grid: 64-channel tiles (family 0) and 32-channel remainder tiles of twice the
// positions (family 1).  The plan picks the fewest classes per tile (least staging) whose rows per class waste no more than the form's padding
// ratio of a tile on padding rows.
#pragma once
#include <stdint.h>

struct WinoRFamily {
    int TT, NC, quads, ttiles;     // samples per tile row, residue classes per tile, tiles along the rows of a class, tiles along T
    int rgroups, ny;               // groups of NC residue classes, Cout tiles
    int m_base, m_stride;          // Cout tile `by` starts at m_base + by * m_stride
    int dot_base;                  // first per-sample partial slot of this family
    int64_t ntiles;                // B * rgroups * quads * ttiles * ny
};
struct WinoRPlan {
    int form;                      // 4: F(4,3), 8: F(8,3)
    int nl;                        // tile families: 0 (the shape is declined), 1, or 2 (the 64 + 32 pair of a 96-channel layer)
    WinoRFamily f[2];
    int64_t tiles;                 // all families, whole batch
    int slots;                     // partial slots per sample (one per tile of one Cout tile); a shape whose slots do not fit an int is declined
};

// What tells the two forms apart.  F(4,3): 256 | 512 positions, up to 10 % padding rows; F(8,3): 512 | 1024 positions (64 | 128 groups of 8), up to 15 %
// (7, 14, 28 rows per class -> 8, 16, 32; the form choice weighs them).  NC * TT <= nc_tt keeps the instantiated shapes: more classes per tile would
// not leave room for two workgroups per CU (NC (RA + 4) staged rows per transform plane).
struct WinoRForm {
    int ntt, tt[3];                // the TT ladder, longest first
    bool tt_divides;               // true: the longest rung that divides T; false: the longest rung not above T (the shortest for a shorter T), which must divide T
    struct { int npos, max_nc, nc_tt; } fam[2];
    int pad_num, pad_den;          // a tile is declined when quads * RA * pad_den > nrow * pad_num
};
static constexpr WinoRForm kWinoR4 = {3, {64, 32, 16}, false, {{256, 8, 256}, {512, 2, 256}}, 11, 10};      // (T = 16: the deepest level of the 8-octave 44.1 kHz network at L = 184184)
static constexpr WinoRForm kWinoR8 = {2, {64, 32}, true, {{512, 4, 128}, {1024, 4, 256}}, 115, 100};

static inline WinoRPlan wino_r_plan(int form, int B, int Cout_pad, int F, int T, int dilF) {
    const WinoRForm& k = form == 8 ? kWinoR8 : kWinoR4;
    WinoRPlan none = {};
    none.form = form;
    WinoRPlan pl = none;
    const int nl = (Cout_pad % 64 == 0) ? 1 : ((Cout_pad % 96 == 0) ? 2 : 0);
    if (!nl || dilF < 1 || (F % dilF)) return none;
    int TT = 0;
    for (int i = 0; i < k.ntt && !TT; ++i)
        if (k.tt_divides ? T % k.tt[i] == 0 : (T >= k.tt[i] || i == k.ntt - 1)) TT = k.tt[i];
    if (!TT || (T % TT)) return none;
    if (nl == 2 && TT != 64) return none;    // F(4,3): the remainder family is instantiated for TT = 64 only; F(8,3): so are family 0 of a pair and the 128-group tile
    const int nrow = F / dilF;               // rows of one residue class
    int64_t slots = 0;
    for (int l = 0; l < nl; ++l) {
        WinoRFamily& f = pl.f[l];
        for (int NC = 1; NC * TT <= k.fam[l].nc_tt && NC <= k.fam[l].max_nc && !(dilF % NC); NC *= 2) {
            const int RA = k.fam[l].npos / (TT * NC);
            const int qd = (nrow + RA - 1) / RA;
            if ((int64_t)qd * RA * k.pad_den > (int64_t)nrow * k.pad_num) continue;
            f.NC = NC; f.quads = qd;
            break;
        }
        if (!f.NC) return none;
        f.TT = TT; f.ttiles = T / TT;
        f.rgroups = dilF / f.NC;
        f.ny = Cout_pad / (nl == 2 ? 96 : 64);
        f.m_base = l == 0 ? 0 : 64;
        f.m_stride = nl == 2 ? 96 : 64;
        f.dot_base = (int)slots;
        const int64_t per_sample = (int64_t)f.rgroups * f.quads * f.ttiles;
        slots += per_sample;
        f.ntiles = (int64_t)B * per_sample * f.ny;
        pl.tiles += f.ntiles;
        if (slots > INT32_MAX) return none;
    }
    pl.slots = (int)slots;
    pl.nl = nl;
    return pl;
}
