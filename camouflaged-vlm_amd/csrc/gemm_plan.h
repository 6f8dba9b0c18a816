// The planner of cvlm_gemm (gemm.hip): which gemm_nt_kernel instantiation a call gets, on which grid, with how much LDS and which
// GemmParams -- a function of the argument struct, the CVLM_GEMM_* knobs, whether a workspace was given and the CU count.  Plain host
// C++: no HIP header, no HIP call, no allocation; cvlm_debug_gemm_plan (include/cvlm.h) runs it without a device.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "../../include/cvlm.h"

namespace cvlm_gemm_p {
namespace {   // everything here is internal to the translation unit that includes it

constexpr int BK_MIN = 32;
constexpr int SK_MAX_TILES = 1024 - (4 * 128 + 2);   // split-K arrival counters behind the tail and error words of the flag page (gemm_kernel.h)

// ---- tail-split workspace (caller-owned, include/cvlm.h): [4 KiB hand-off words][128 tiles x 3 parts of 256 x 256 f32]
constexpr size_t TAIL_FLAG_BYTES = 4096;
constexpr size_t TAIL_WS_BYTES = (size_t)128 * 3 * 256 * 256 * sizeof(float);
static_assert((4 * 128 + 2) * sizeof(unsigned) <= TAIL_FLAG_BYTES, "hand-off words fit the flag page");

// ---- tuning knobs, read once per process.  A process started with CVLM_GEMM_VARIANT_LIVE=1 (tests/conftest.py,
// tools/ab_gemm.py) re-reads them on every call so that variants can be A/B-ed and raced inside one process.
struct GemmKnobs {
    int tail;       // CVLM_GEMM_TAIL: K-parts for a partial last round of 256^2 tiles
    int variant;    // CVLM_GEMM_VARIANT 0: auto (big tile for big problems); 1: 128x128 2-stage; 2: 256x128 3-stage; 3: 128x128 3-stage(4 waves)
    int persist;    // CVLM_GEMM_PERSIST: persistent form of the 256^2 kernel
    int colsplit;   // CVLM_GEMM_COLSPLIT: two launches for a grid a little over one round
    int ring;       // CVLM_GEMM_RING: slots of the deep LDS ring of the 128^2 launches of a small grid
    // CVLM_GEMM_W8: 0 four waves of 64 x 64; 1 (default) eight waves, 64 x 128 tiles when those fit one round of workgroups, else
    // 128^2; 2 / 3 force the 64-row / 128-row form (A/B tools)
    int w8;
    int sk;         // CVLM_GEMM_SK 0: no split-K over all tiles; 1: by the model; 2..8: forced parts (A/B tools, tests)
    int t192;       // CVLM_GEMM_T192: 192-row tiles under one round of 256-row ones
    int group_m;    // CVLM_GEMM_GROUP_M > 0 (live processes only, tools): tile rows per L2 super-tile of the mx kernels
#ifdef CVLM_PROBES
    bool trace;     // a trace buffer is set (cvlm_debug_set_gemm_trace): CVLM_GEMM_VARIANT=47 runs
#endif
};
inline int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
inline GemmKnobs gemm_knobs_from_env(bool live) {
    GemmKnobs k = {};
    k.tail = env_int("CVLM_GEMM_TAIL", 1); k.variant = env_int("CVLM_GEMM_VARIANT", 0); k.persist = env_int("CVLM_GEMM_PERSIST", 1);
    k.colsplit = env_int("CVLM_GEMM_COLSPLIT", 1); k.ring = env_int("CVLM_GEMM_RING", 4); k.w8 = env_int("CVLM_GEMM_W8", 1);
    k.sk = env_int("CVLM_GEMM_SK", 1); k.t192 = env_int("CVLM_GEMM_T192", 1);
    k.group_m = live ? env_int("CVLM_GEMM_GROUP_M", 0) : 0;
    return k;
}
inline GemmKnobs gemm_knobs() {
    static const bool live = env_int("CVLM_GEMM_VARIANT_LIVE", 0) != 0;
    static const GemmKnobs latched = gemm_knobs_from_env(false);
    return live ? gemm_knobs_from_env(true) : latched;
}

// ---- one instantiation of gemm_nt_kernel: its template parameters, same order, same defaults
struct GemmKernel {
    int split, wm, wn, nstage, bk, dbg = 0, mt = 4;
    bool persist = false;
    int epi = -1;
    bool conv = false, sk = false, wil = false, ail = false, mx = false;
};
constexpr uint64_t gemm_kernel_key(const GemmKernel& k) {
    return (uint64_t)k.split | (uint64_t)k.wm << 4 | (uint64_t)k.wn << 8 | (uint64_t)k.nstage << 12 | (uint64_t)k.bk << 16 | (uint64_t)k.dbg << 24 |
           (uint64_t)k.mt << 32 | (uint64_t)(k.epi + 1) << 36 | (uint64_t)k.persist << 40 | (uint64_t)k.conv << 41 | (uint64_t)k.sk << 42 |
           (uint64_t)k.wil << 43 | (uint64_t)k.ail << 44 | (uint64_t)k.mx << 45;
}
// Dynamic LDS of an instantiation: the ring -- slots x planes x (tile rows + tile columns) x BK halves -- plus, PERSIST, one
// 16 x 64 f32 slab per wave (160 KB in all); MX: five half-slots of 32 KiB (gemm_kernel.h, MX branch).  The convolution kernels are
// given two planes' worth whatever their split (the size their launches have always passed).
constexpr int gemm_lds_bytes(const GemmKernel& k) {
    const int slots = k.nstage >= 13 ? k.nstage - 10 : k.nstage == 6 ? 1 : k.nstage >= 4 ? 2 : k.nstage;
    const int planes = k.split == 3 || k.conv ? 2 : 1;
    return k.mx ? 5 * 32768 : slots * planes * (k.wm * k.mt * 16 + k.wn * 64) * k.bk * 2 + (k.persist ? k.wm * k.wn * 16 * 64 * 4 : 0);
}

// The instantiations cvlm_gemm launches, X(template arguments): gemm.hip switches over this list (the ones with WIL are instantiated
// in gemm_il.hip, CVLM_GEMM_IL_KERNELS) ...
#define CVLM_GEMM_KERNELS(X)                                                                                                           \
    X(1, 2, 2, 2, 32) X(1, 4, 2, 3, 32) X(1, 2, 4, 3, 32, 0, 8) X(1, 4, 1, 2, 32, 0, 4, false, -1, true)                               \
    X(3, 4, 1, 2, 32, 0, 4, false, -1, true)                                                                                           \
    X(3, 2, 2, 2, 32) X(3, 2, 2, 13, 32) X(3, 2, 2, 14, 32) X(3, 2, 2, 15, 32) X(3, 4, 2, 3, 32)                                       \
    X(3, 4, 2, 14, 32, 0, 1) X(3, 4, 2, 14, 32, 0, 2)                                                                                  \
    X(3, 2, 2, 2, 32, 0, 4, false, -1, false, true) X(3, 2, 2, 13, 32, 0, 4, false, -1, false, true)                                   \
    X(3, 2, 2, 14, 32, 0, 4, false, -1, false, true) X(3, 4, 2, 14, 32, 0, 2, false, -1, false, true)                                  \
    X(3, 2, 4, 5, 32, 0, 8) X(3, 2, 4, 5, 32, 0, 8, false, 0) X(3, 2, 4, 5, 32, 0, 8, false, 1) X(3, 2, 4, 5, 32, 0, 8, false, 2)      \
    X(3, 2, 4, 5, 32, 0, 8, true, 0) X(3, 2, 4, 5, 32, 0, 8, true, 1) X(3, 2, 4, 5, 32, 0, 8, true, 2)                                 \
    X(3, 2, 4, 5, 32, 0, 6, false, 2)                                                                                                  \
    CVLM_X_IL(X, 3, 2, 4, 5, 32, 0, 8, false, 0, false, false) CVLM_X_IL(X, 3, 2, 4, 5, 32, 0, 8, false, 1, false, false)              \
    CVLM_X_IL(X, 3, 2, 4, 5, 32, 0, 8, false, 2, false, false) CVLM_X_IL(X, 3, 2, 4, 5, 32, 0, 8, true, 0, false, false)               \
    CVLM_X_IL(X, 3, 2, 4, 5, 32, 0, 8, true, 1, false, false) CVLM_X_IL(X, 3, 2, 4, 5, 32, 0, 8, true, 2, false, false)                \
    CVLM_X_IL(X, 3, 2, 4, 5, 32, 0, 6, false, 2, false, false) CVLM_X_IL(X, 3, 4, 2, 3, 32, 0, 4, false, -1, false, false)             \
    CVLM_X_IL(X, 3, 4, 2, 14, 32, 0, 1, false, -1, false, false) CVLM_X_IL(X, 3, 4, 2, 14, 32, 0, 2, false, -1, false, false)          \
    CVLM_X_IL(X, 3, 4, 2, 14, 32, 0, 2, false, -1, false, true)
#define CVLM_X_IL(X, ...) X(__VA_ARGS__, true, false) X(__VA_ARGS__, true, true)   /* weight image; weight and activation image */
// ... the probe variants (make EXTRA=-DCVLM_PROBES: the variants behind profiles/r01_gemm_probes.md and tools/{ab,trace}_gemm.py) ...
#define CVLM_GEMM_PROBE_KERNELS(X)                                                                                                     \
    X(1, 2, 2, 3, 32) X(1, 2, 2, 3, 64) X(3, 2, 2, 3, 32) X(3, 2, 2, 2, 64) X(3, 2, 2, 2, 64, 2) X(3, 2, 2, 2, 32, 2)                  \
    X(3, 2, 4, 2, 32, 0, 8) X(3, 2, 4, 2, 32, 1, 8) X(3, 2, 4, 2, 32, 2, 8)                                                            \
    X(3, 2, 4, 4, 32, 0, 8) X(3, 2, 4, 4, 32, 1, 8) X(3, 2, 4, 4, 32, 2, 8)                                                            \
    X(3, 2, 2, 6, 32, 0, 8) X(3, 2, 2, 6, 32, 1, 8) X(3, 2, 2, 6, 32, 2, 8)                                                            \
    X(3, 2, 4, 5, 32, 1, 8) X(3, 2, 4, 5, 32, 2, 8) X(3, 2, 4, 5, 32, 3, 8) X(3, 2, 4, 5, 32, 4, 8) X(3, 2, 4, 5, 32, 5, 8)            \
    X(3, 2, 4, 5, 32, 6, 8) X(3, 2, 4, 5, 32, 7, 8) X(3, 2, 4, 5, 32, 8, 8)
// ... and the mx kernels (ABI 10), instantiated and launched in gemm_mx.hip: 256-row tiles with the LayerNorm-fold or the h2-residual
// epilogue, 192-row tiles with the latter; X(MT, EPI, DBG)
#define CVLM_GEMM_MX_KERNELS(X) X(8, 1, 0) X(8, 2, 0) X(6, 2, 0)
/* CVLM_GEMM_VARIANT = 100 + DBG: the probe forms of the fold-epilogue kernel (gemm_kernel.h, MX branch; tools/probe_gemm_mx.py), and a
   few of the same for the h2-residual form (lin2) */
#define CVLM_GEMM_MX_PROBE_KERNELS(X)                                                                                                  \
    X(8, 1, 1) X(8, 1, 2) X(8, 1, 3) X(8, 1, 5) X(8, 1, 6) X(8, 1, 7) X(8, 1, 9) X(8, 1, 10) X(8, 1, 11) X(8, 1, 12) X(8, 1, 13)       \
    X(8, 1, 14) X(8, 1, 15) X(8, 1, 16) X(8, 1, 17) X(8, 1, 18) X(8, 1, 19) X(8, 1, 20) X(8, 1, 21) X(8, 1, 22)                        \
    X(8, 2, 1) X(8, 2, 2) X(8, 2, 3) X(8, 2, 6) X(8, 2, 16) X(8, 2, 17) X(8, 2, 18) X(8, 2, 19) X(8, 2, 20) X(8, 2, 21) X(8, 2, 22)
constexpr GemmKernel gemm_mx_kernel(int mt, int epi, int dbg) { return GemmKernel{3, 2, 4, 5, 32, dbg, mt, false, epi, false, false, true, true, true}; }
constexpr bool gemm_mx_kernel_exists(int mt, int epi, int dbg) {
#define CVLM_X(MT, EPI, DBG) if (mt == MT && epi == EPI && dbg == DBG) return true;
    CVLM_GEMM_MX_KERNELS(CVLM_X)
#ifdef CVLM_PROBES
    CVLM_GEMM_MX_PROBE_KERNELS(CVLM_X)
#endif
#undef CVLM_X
    return false;
}

// ---- everything one launch needs
struct GemmPlan {
    GemmKernel k;
    int n0, N;                       // the columns [n0, n0 + N) of the problem (a column split is two plans)
    int nbx, nby;                    // tiles along N / M
    int grid_x, grid_y, block, lds_bytes;
    int group_m;                     // tile rows per L2 super-tile
    int tail_rem, tail_split;        // 256^2 staggered kernels: the last tail_rem tiles run as tail_split chained K-parts
    int total_blocks;                // PERSIST: length of the tile list
    int sk_parts;                    // SK kernels: K-parts per tile
    bool use_ws;                     // the launch is given the workspace (slabs and hand-off words of K-parts)
};

inline int gemm_validate(const cvlm_gemm_args& g) {
    if (!g.a_hi || !g.w_hi) return CVLM_E_BADARG;
    if (g.M <= 0 || g.N <= 0 || g.K <= 0 || (g.K % BK_MIN) != 0) return CVLM_E_BADARG;
    if ((g.lda & 7) || (g.ldw & 7) || (g.stride_a & 7) || (g.stride_w & 7)) return CVLM_E_BADARG;
    if (g.split != 1 && g.split != 3) return CVLM_E_BADARG;
    if (g.split == 3 && ((!g.a_lo && !g.a_il && !g.a_mx) || !g.w_lo)) return CVLM_E_BADARG;
    if (!g.out_f32 && !g.out_hi) return CVLM_E_BADARG;
    if (g.ps_c2 > 0 && ((g.ps_c2 & 3) || g.ps_h <= 0 || g.ps_w <= 0)) return CVLM_E_BADARG;
    if (g.hm_S > 0 && ((g.hm_hd & 3) || g.hm_H <= 0 || (g.M % g.hm_S) || g.N != 3 * g.hm_H * g.hm_hd || !g.out_hi)) return CVLM_E_BADARG;
    const bool conv = g.conv_c > 0;
    if (conv) {
        // implicit 3x3 convolution: channels a power of two >= 32 (a K-tile never straddles a tap), rows = whole images
        if (g.conv_h <= 0 || g.conv_w <= 0 || g.conv_c < 32 || (g.conv_c & (g.conv_c - 1)) || g.K != 9 * g.conv_c ||
            g.lda != g.conv_c || (g.M % (g.conv_h * g.conv_w)) || g.batch > 1)
            return CVLM_E_UNSUPPORTED;
    }
    const bool fold = g.ln_stats != nullptr, h2res = g.res_hi != nullptr || g.row_stats != nullptr;
    if (fold || h2res) {
        // these two epilogue forms exist on the LDS-staged path only: h2 output, 8-column row pieces, one problem per launch
        if (fold && h2res) return CVLM_E_BADARG;
        if (!g.out_hi || g.out_f32 || g.residual || g.ps_c2 > 0 || g.batch > 1) return CVLM_E_BADARG;
        if ((g.N & 7) || (g.ldoh & 7) || (g.hm_S > 0 && ((g.hm_hd & 7) || g.hm_S < 128))) return CVLM_E_UNSUPPORTED;
        if (fold && (!g.ln_colsum || (g.act != CVLM_ACT_NONE && g.act != CVLM_ACT_GELU && g.act != CVLM_ACT_QUICKGELU))) return CVLM_E_BADARG;
        if (h2res && (g.act != CVLM_ACT_NONE || (g.res_hi && ((!g.res_lo && !g.res_il) || (g.ldrh & 7))))) return CVLM_E_BADARG;
    }
    const bool il_any = g.a_il || g.out_il || g.res_il;
    if (il_any) {
        // 128-byte-row images of activations (ABI 6): split-3, one problem, the LDS-staged epilogues, no head-major / pixel-shuffle store
        if (g.split != 3 || conv || g.batch > 1 || (g.out_il && g.hm_S > 0) || (g.hm_S > 0 && ((g.hm_hd & 7) || g.hm_S < 256)) || g.ps_c2 > 0 ||
            (g.N & 7) || (g.ldoh & 7) || (g.stride_oh & 7) ||
            (g.out_f32 && ((g.ldo & 3) || (g.stride_o & 3))) || (g.residual && ((g.ldr & 3) || (g.stride_r & 3))))
            return CVLM_E_UNSUPPORTED;
        if (g.a_il && (!g.w_il || (g.lda & 7) || g.lda < 2 * (int64_t)g.K)) return CVLM_E_UNSUPPORTED;
        if (g.res_il && !g.res_hi) return CVLM_E_BADARG;
    }
    if (g.a_mx || g.out_mx || g.res_mx) {
        // mx images (ABI 10): split-3, one problem, the LDS-staged epilogues; whole 64-column groups
        if (g.split != 3 || conv || g.batch > 1 || g.ps_c2 > 0 || (g.a_mx && g.a_il) || (g.out_mx && g.out_il) || (g.res_mx && g.res_il) ||
            (g.N & 7) || (g.ldoh & 7) || (g.stride_oh & 7) || (g.hm_S > 0 && ((g.hm_hd & 7) || g.hm_S < 256)) ||
            (g.out_f32 && ((g.ldo & 3) || (g.stride_o & 3))) || (g.residual && ((g.ldr & 3) || (g.stride_r & 3))))
            return CVLM_E_UNSUPPORTED;
        if (g.a_mx && (!g.a_mxs || !g.w_mx || !g.w_mxs || (g.K & 63) || (g.lda & 7) || g.lda < 2 * (int64_t)g.K || (g.ldw_mx & 7) ||
                       g.ldw_mx < 2 * (int64_t)g.K || (g.lda_s & 3) || (g.ldw_s & 3) || g.lda_s * 64 < g.K || g.ldw_s * 64 < g.K))
            return CVLM_E_BADARG;
        if (g.out_mx && (!g.out_hi || !g.out_mxs || g.hm_S > 0 || (g.N & 63) || (g.ldo_s & 3) || (g.out_lo && (g.ldol & 7))))
            return CVLM_E_BADARG;
        if (g.res_mx && (!g.res_hi || !g.res_lo || (g.ldrl & 7) || (g.ldrh & 7))) return CVLM_E_BADARG;
    }
    return 0;
}

// The argument struct as the kernel gets it (GemmParams.a) and as the planner reads it.
inline cvlm_gemm_args gemm_sanitised(const cvlm_gemm_args& g) {
    cvlm_gemm_args a = g;
    if (g.ln_stats || g.res_hi || g.row_stats) {
        // these launches have no f32 output, no f32 residual and one problem: whatever the caller left in the fields that describe
        // them must not send the kernel to the scalar epilogue, which knows neither form (it would return rc 0 and wrong numbers)
        a.ldo = a.stride_o = a.ldr = a.stride_r = a.stride_oh = 0;
        a.stride_a = a.stride_w = 0;
    }
    if (a.batch <= 0) a.batch = 1;
    if (a.out_scale == 0.f) a.out_scale = 1.f;
    return a;
}

// ---- the cost models.  Tiles of tm x tn over all problems of the launch:
inline long tiles(const cvlm_gemm_args& a, int tm, int tn) { return (long)((a.M + tm - 1) / tm) * ((a.N + tn - 1) / tn) * a.batch; }
inline long rounds(long t, long slots) { return (t + slots - 1) / slots; }
// 256^2 staggered: 0.0685 us per K + 14 us per tile (S: the tile cut into S K-parts)
inline double tile256_us(double K, int S = 1) { return 0.0685 * K / S + 14.0; }
// Modelled time of a tail round cut into S chained K-parts: one part's main loop + epilogue, first slab
// publish (~16 us), last read-back (~8 us), ~20 us per middle hop (read + publish), and the slabs of all `rem` tiles
// moving at once (qkv at K = 1280 with 128 tail tiles measured no gain).
inline double tail_us(int S, int K, int rem) {
    return tile256_us(K, S) + 16.0 + 8.0 + 20.0 * (S - 2) + 0.15 * rem;   // + concurrent hand-offs (rem slabs at once)
}
// Number of K-parts for a last round of `rem` tiles (1 = leave it whole).
inline int tail_parts(int rem, int K) {
    if (rem <= 0 || rem > 128) return 1;
    const int smax = 256 / rem < 4 ? 256 / rem : 4;
    int best = 1;
    double t = tile256_us(K);
    // a split has to win by a margin: at K = 1280 / 128 tail tiles the model calls it even and the measurement does not
    // (proj 32768 x 1280 x 1280: 312-355 us split, 303-338 us whole, tools/ab_tail.py)
    double need = 0.92 * t;
    for (int S = 2; S <= smax; ++S)
        if (K / 32 >= 4 * S && tail_us(S, K, rem) < need) { t = need = tail_us(S, K, rem); best = S; }
    return best;
}

// variant 0 on grids that fill the chip several times: 1 (128^2 tiles), 2 (256 x 128) or 5 (256^2)
inline int big_grid_variant(const cvlm_gemm_args& a, const GemmKnobs& kn, bool have_ws) {
    // 256x256 tiles (1 workgroup/CU, half the L2->LDS bytes per FLOP) when they fill the 256 CUs well,
    // otherwise 128x128 tiles (2 workgroups/CU -> 512 slots) for small / skinny problems.
    const long t5 = tiles(a, 256, 256), t1 = tiles(a, 128, 128), t2 = tiles(a, 256, 128);
    if (a.split == 3) {
        // microsecond model fitted to tools/ab_gemm.py (B = 8 cascade shapes): rounds x time per tile,
        //   128^2 (2 workgroups/CU): 0.0544 us per K;  256x128: 0.0469 us per K;
        //   256^2 staggered: 0.0685 us per K + 14 us per tile, last partial round cut into S K-parts (tail_us).
        const double K = (double)a.K;
        const double m1 = (double)rounds(t1, 512) * 0.0544 * K;
        const double m2 = (double)rounds(t2, 256) * 0.0469 * K;
        const int rem = (int)(t5 % 256);
        double tail = rem > 0 ? tile256_us(K) : 0.0;
        if (kn.tail && have_ws && a.batch == 1) {
            const int S = tail_parts(rem, a.K);
            if (S >= 2) tail = tail_us(S, a.K, rem);
        }
        const double m7 = (double)(t5 / 256) * tile256_us(K) + tail;
        // a near tie goes to the 256^2 tile: it moves a third fewer L2->LDS bytes per flop, and at the power cap the
        // joules count (proj 32768 x 1280 x 1280 is modelled 305 vs 300 us; with 256^2 tiles the cascade gains 0.85 %)
        if (a.a_il) return m7 <= 1.04 * m2 ? 5 : 2;                    // kernels that stage the activation image: 256^2 family, 256 x 128
        return (m7 <= 1.04 * m1 && m7 <= 1.04 * m2) ? 5 : (m2 <= m1 ? 2 : 1);
    }
    if (t5 >= 200 && t5 <= 256) return 5;                              // one full wave of 256^2 tiles
    // padded work / relative throughput (measured, profiles/r01_gemm_probes.md)
    const double c1 = (double)(rounds(t1, 512) * 512) * 1.0;
    if (t5 >= 1536) {
        const double c2 = (double)(rounds(t2, 256) * 256) * 2.0 / 1.08;
        const double c5 = (double)(rounds(t5, 256) * 256) * 4.0 / 1.20;
        return (c5 <= c2 && c5 <= c1) ? 5 : (c2 <= c1 ? 2 : 1);
    }
    const double c2 = (double)(rounds(t2, 256) * 256) * 2.0 / (a.M >= 16384 ? 1.08 : 1.05);
    return (c2 < c1) ? 2 : 1;
}

inline int pick_ring(const GemmKnobs& kn, long wgs) { return (wgs <= 256 && kn.ring >= 3 && kn.ring <= 5) ? kn.ring : 0; }

// ---- small grids: one image (M = 4096 in the ViT-H blocks, 581 in the CLIP towers -- the reference's own call pattern,
// demo.py / DataLoader batch_size = 1) and everything below.  The constants of the model above were fitted on grids that fill
// the chip several times; here a workgroup often has a CU (or the L2) to itself and runs up to twice as fast, hand-offs are
// cheap (every K-part is resident at once) and a fourth form exists: split-K over ALL tiles of a 128^2 grid (SK kernel).
// Per-workgroup cost = t0 + K * c(fill), c rising linearly with the fill of the workgroup slots; fitted on the eight shapes of
// tools/ab_gemm.py SHAPES=b1 (profiles/r03_ab_gemm_b1.log: the model picks the measured winner for each).
struct SmallGridChoice {
    int variant;     // 1, 2 or 5 (the knob's value when that is not 0)
    int tail_S;      // variant 5: K-parts of the last round's tiles, 1 = whole (0: not chosen here)
    int sk_parts;    // > 1: split-K over every 128^2 tile
};
inline SmallGridChoice small_grid_choice(const cvlm_gemm_args& a, const GemmKnobs& kn, bool have_ws) {
    SmallGridChoice c = {kn.variant, 0, 1};
    const double K = (double)a.K;
    const long t1 = tiles(a, 128, 128), t2 = tiles(a, 256, 128), t5 = tiles(a, 256, 256);
    auto fillc = [](double lo, double hi, double wgs, double slots) { const double f = wgs / slots; return lo + (hi - lo) * (f < 1.0 ? f : 1.0); };
    auto over = [](double wgs, double slots) { const double r = wgs / slots; return r > 1.0 ? r : 1.0; };
    // 128^2 family: under one round of workgroups the deep-ring / eight-wave kernels run (0.78 of the fitted two-slot cost per K;
    // 0.62 with 64 x 128 tiles when those still fit one round), tools/ab_gemm.py SHAPES=b1 COLD=1
    const bool ring_on = kn.ring == 4 && kn.w8 != 0;
    const double k1 = !ring_on || t1 > 256 ? 1.0 : (tiles(a, 64, 128) <= 256 && kn.w8 != 3 ? 0.62 : 0.78);
    const double m1 = 4.0 + k1 * K * fillc(0.021, 0.054, (double)t1, 512.0) * over((double)t1, 512.0);
    const double m2 = 4.0 + K * fillc(0.028, 0.047, (double)t2, 256.0) * over((double)t2, 256.0);
    // 256^2 tiles: full rounds at the fitted tile time, the last round whole or cut into S chained K-parts
    const long rem5 = t5 % 256;
    double m7 = (double)(t5 / 256) * tile256_us(K);
    int tailS = 0;
    if (rem5 > 0) {
        double last = tile256_us(K) * (0.75 + 0.25 * (double)rem5 / 256.0);
        if (kn.tail && have_ws && rem5 <= 128) {
            const int smax = 256 / rem5 < 4 ? (int)(256 / rem5) : 4;
            for (int S = 2; S <= smax; ++S) {
                if (a.K / 32 < 4 * S) break;
                const double f = (double)(rem5 * S) / 256.0;
                const double t = tile256_us(K, S) * (0.75 + 0.25 * (f < 1.0 ? f : 1.0)) + 6.0 + 4.0 * S;
                if (t < 0.95 * last) { last = t; tailS = S; }
            }
        }
        m7 += last;
    }
    // split-K over every 128^2 tile: S x (slab write + read) of the whole output is what it costs
    auto sk_fits = [&](int S) { return a.K / 32 >= 4 * S && (size_t)t1 * S * 128 * 128 * sizeof(float) <= TAIL_WS_BYTES; };
    int skS = 1;
    double msk = 1e30;
    if (have_ws && kn.sk != 0 && t1 <= SK_MAX_TILES) {
        for (int S = 2; S <= 8 && sk_fits(S); ++S) {
            const double wg = (double)(t1 * S);
            const double t = 4.0 + (ring_on && wg <= 256.0 ? 0.78 : 1.0) * (K / S) * fillc(0.021, 0.054, wg, 512.0) * over(wg, 512.0) + 6.0 + 2.0 * S + 0.052 * wg;
            if (t < msk) { msk = t; skS = S; }
        }
    }
    if (kn.sk > 1) {                                                 // forced (A/B tools, tests): the same limits
        const bool okS = have_ws && kn.sk <= 8 && t1 <= SK_MAX_TILES && sk_fits(kn.sk);
        skS = okS ? kn.sk : 1;
        msk = okS ? 0.0 : 1e30;
    }
    // activation image: of the 128^2 family only the eight-wave ring kernels stage it (one round of workgroups)
    const bool ail1_ok = !a.a_il || (ring_on && t1 <= 256);
    if (a.a_il && skS > 1 && !(ring_on && t1 * skS <= 256)) { skS = 1; msk = 1e30; }
    if (kn.variant == 0) {
        double best = ail1_ok ? m1 : 1e30;
        c.variant = 1;
        if (m2 < best) { best = m2; c.variant = 2; }
        if (m7 < best) { best = m7; c.variant = 5; c.tail_S = tailS > 0 ? tailS : 1; }
        if (skS > 1 && msk < 0.9 * best) { c.variant = 1; c.sk_parts = skS; }
    } else if (skS > 1) {
        c.sk_parts = skS;
    }
    return c;
}

// Grid, block and LDS of kernel pl.k over the columns pl.N of `a`, from the K-parts and the tile list chosen before.
inline int gemm_plan_finish(const cvlm_gemm_args& a, GemmPlan& pl) {
    const GemmKernel& k = pl.k;
    pl.nbx = (pl.N + k.wn * 64 - 1) / (k.wn * 64);
    pl.nby = (a.M + k.wm * k.mt * 16 - 1) / (k.wm * k.mt * 16);
    if (!k.persist) pl.grid_x = k.sk ? pl.nbx * pl.nby * pl.sk_parts : pl.nbx * pl.nby + pl.tail_rem * (pl.tail_split - 1);   // persistent: the CUs
    pl.grid_y = a.batch;
    pl.block = k.wm * k.wn * 64;
    pl.lds_bytes = gemm_lds_bytes(k);
    return 1;
}

// One launch for the sanitised arguments `a` (columns [pl.n0, pl.n0 + a.N)).  cus(): the CU count, asked for only where a persistent
// grid is in question (the device query behind it is not free).
template <class Cus>
inline int gemm_plan_one(const cvlm_gemm_args& a, const GemmKnobs& kn, bool have_ws, Cus&& cus, GemmPlan& pl) {
    const bool conv = a.conv_c > 0, fold = a.ln_stats != nullptr, h2res = a.res_hi != nullptr || a.row_stats != nullptr;
    const bool one3 = a.split == 3 && !conv && a.batch == 1;            // one split-3 problem, no convolution
    // interleaved weight image (ABI 6): used by the big-tile kernels when the caller provides it
    const bool wil = a.w_il && one3 && a.ldw_il >= 2 * (int64_t)a.K && (a.ldw_il & 7) == 0;
    const bool ail = a.a_il != 0;
    if (ail && (!wil || (kn.variant != 0 && kn.variant != 2 && kn.variant != 7))) return CVLM_E_UNSUPPORTED;
    pl.N = a.N;
    pl.group_m = 8;
    pl.tail_rem = 0; pl.tail_split = 1; pl.total_blocks = 0; pl.sk_parts = 1; pl.use_ws = false;
    int variant = kn.variant == 0 ? big_grid_variant(a, kn, have_ws) : kn.variant;
    int tail_S = 0;                                                      // K-parts of a partial last round of 256^2 tiles, 0: by tail_parts
    if (one3 && a.M <= 4096 && !a.a_mx && (kn.variant == 0 || (kn.variant == 1 && kn.sk > 1))) {
        const SmallGridChoice c = small_grid_choice(a, kn, have_ws);
        variant = c.variant; tail_S = c.tail_S; pl.sk_parts = c.sk_parts;
    }
    const long t1 = tiles(a, 128, 128), t5 = tiles(a, 256, 256), t6 = tiles(a, 192, 256), t64 = tiles(a, 64, 128);
    if (pl.sk_parts > 1) {
        // 128^2 launches of a small grid (whole or in K-parts) run the deep ring: see the R-slot loop of the kernel
        // ... with eight waves of 32 x 64 instead of four of 64 x 64 (CVLM_GEMM_W8): a wave issues one KiB of DMA per ~100 cycles, and
        // with the chip mostly idle it is the issue of a K-tile's 32 DMA instructions by four waves (800 cycles against 768 of MFMAs),
        // not the matrix pipe, that a workgroup waits for
        int ring = pick_ring(kn, t1 * pl.sk_parts);
        if (ring > 4) ring = 4;                                          // five slots are the whole LDS; this kernel has a static word beside them
        const bool w8 = ring == 4 && kn.w8;
        if (ail && !(w8 && wil)) return CVLM_E_UNSUPPORTED;
        if (w8) pl.k = GemmKernel{3, 4, 2, 14, 32, 0, 2, false, -1, false, true, wil, ail};   /* wil: operands from the 128-byte-row images */
        else pl.k = GemmKernel{3, 2, 2, ring == 3 ? 13 : ring == 4 ? 14 : 2, 32, 0, 4, false, -1, false, true};
        pl.use_ws = true;
        return gemm_plan_finish(a, pl);
    }
    if (conv) {
        // 256 x 64 tiles (4 waves, 2 workgroups per CU): the edge head's N is 32 / 64, the neck's 256
        pl.k = GemmKernel{a.split, 4, 1, 2, 32, 0, 4, false, -1, true};
        return gemm_plan_finish(a, pl);
    }
    if (a.split != 3) {
        if (variant == 2) pl.k = GemmKernel{1, 4, 2, 3, 32};
        else if (variant == 5) pl.k = GemmKernel{1, 2, 4, 3, 32, 0, 8};
#ifdef CVLM_PROBES
        else if (variant == 4 && (a.K % 64) == 0) pl.k = GemmKernel{1, 2, 2, 3, 64};
        else if (variant == 3) pl.k = GemmKernel{1, 2, 2, 3, 32};
#endif
        else pl.k = GemmKernel{1, 2, 2, 2, 32};
        return gemm_plan_finish(a, pl);
    }
    if (variant == 5 && kn.variant == 0) variant = 7;      // auto: staggered wave groups (3-5 % over the plain 256^2 loop)
    // tile rows per L2 super-tile: 8 for the small tiles; the 256^2 kernel is 2-3 % faster with 4 (2 at long K),
    // i.e. ~20 (10) of an XCD's 32 co-resident tiles sharing their activation panels (tools/ab_gemm.py sweep)
    if (variant == 7 || a.a_mx) pl.group_m = a.K >= 4096 ? 2 : 4;
    if (variant == 7 && kn.tail && have_ws && a.batch == 1) {
        const int rem = (int)(t5 % 256);
        const int S = tail_S > 0 ? tail_S : tail_parts(rem, a.K);        // small grids: chosen by their own model
        if (S >= 2) { pl.tail_rem = rem; pl.tail_split = S; pl.use_ws = true; }
    }
    const bool lds_staged = a.ps_c2 == 0 && (a.N & 7) == 0 && (a.hm_S == 0 || ((a.hm_hd & 7) == 0 && a.hm_S >= 128)) &&
                            (a.ldo & 3) == 0 && (a.stride_o & 3) == 0 && (a.ldr & 3) == 0 && (a.stride_r & 3) == 0 &&
                            (a.ldoh & 7) == 0 && (a.stride_oh & 7) == 0;
    // 192 x 256 tiles (MT = 6, same staggered loop) for grids UNDER one round of 256^2 tiles: the CLIP out_proj / c_proj of the
    // fused 16-image forward are 37 x 4 = 148 tiles on 256 CUs; 49 x 4 = 196 tiles of 192 rows put 48 more CUs to work and
    // every workgroup finishes a quarter earlier.  Only the h2-residual form is instantiated (what those launches use).
    const bool fits192 = kn.t192 && h2res && t5 <= 256 && t6 <= 256 && t6 > t5 && a.M > 4096;
    const int epi = fold ? 1 : (h2res ? 2 : 0);
    if (a.a_mx) {
        // both operands mx: the staggered 256-column kernel in its unit form (gemm_kernel.h, MX), one instantiation per epilogue form;
        // 192-row tiles under one round of 256-row ones (the h2-residual form, as above); K-parts of a partial last round are whole
        // groups of 8 units
        // 32-bit quantities of the kernel: the offset of a row inside its 8-row DMA block (the block's base is a 64-bit scalar) and the
        // byte offset of a row's scale words -- not the size of the images (batches above 4 GiB of operand are fine)
        if (!lds_staged || a.batch != 1 || (a.M & 7) || (a.N & 7) || (int64_t)8 * a.lda * 2 >= ((int64_t)1 << 32) ||
            (int64_t)8 * a.ldw_mx * 2 >= ((int64_t)1 << 32) || (int64_t)a.M * 4 * a.lda_s >= ((int64_t)1 << 32) ||
            (int64_t)a.N * 4 * a.ldw_s >= ((int64_t)1 << 32))
            return CVLM_E_UNSUPPORTED;
        if (epi == 0) return CVLM_E_UNSUPPORTED;                          /* the plain epilogue has no mx instantiation (no caller) */
        pl.tail_rem = 0; pl.tail_split = 1;     // the K-parts are chosen again here; the workspace pointers stay if the choice above set them
        if (!fits192 && kn.tail && have_ws) {
            int S = tail_parts((int)(t5 % 256), a.K);
            while (S > 1 && (a.K / 32 + 7) / 8 < 2 * S) --S;
            if (S >= 2) { pl.tail_rem = (int)(t5 % 256); pl.tail_split = S; pl.use_ws = true; }
        }
        if (kn.group_m > 0) pl.group_m = kn.group_m;   /* tools only */
        const int probe = kn.variant >= 100 ? kn.variant - 100 : 0;          /* probe builds: tools/probe_gemm_mx.py */
        pl.k = gemm_mx_kernel(fits192 ? 6 : 8, epi, gemm_mx_kernel_exists(fits192 ? 6 : 8, epi, probe) ? probe : 0);
        return gemm_plan_finish(a, pl);
    }
    const bool staggered = variant == 7 && lds_staged && a.batch == 1;    // 256x256, 8 waves, wave groups staggered; one epilogue form
    // slots of the deep ring for a plain (whole-tile) 128^2-family launch of a small grid, 0: the two-slot loop
    const int ring = (one3 && a.M <= 4096 && variant == 1) ? pick_ring(kn, t1) : 0;
    if (staggered && kn.variant == 0 && fits192 && pl.tail_rem == 0)
        pl.k = GemmKernel{3, 2, 4, 5, 32, 0, 6, false, 2, false, false, wil, ail};
    // Persistent form of the 256^2 kernel: one workgroup per CU walks the tile list.  Not for launches with tail parts:
    // their hand-off chain relies on in-order dispatch (every producer is resident or done before its consumer
    // starts), which a persistent grid sharing the chip with another stream cannot promise.
    else if (staggered && kn.persist && (kn.variant == 0 || kn.variant == 7) && pl.tail_rem == 0 && t5 > cus()) {
        pl.k = GemmKernel{3, 2, 4, 5, 32, 0, 8, true, epi, false, false, wil, ail};
        pl.total_blocks = (int)t5;
        pl.grid_x = cus();
    }
    else if (variant == 2) pl.k = GemmKernel{3, 4, 2, 3, 32, 0, 4, false, -1, false, false, wil, ail};   /* 256 x 128 tiles */
    else if (staggered) pl.k = GemmKernel{3, 2, 4, 5, 32, 0, 8, false, epi, false, false, wil, ail};
    else if (ring == 4 && (kn.w8 == 2 || (kn.w8 == 1 && t64 <= 256)))
        pl.k = GemmKernel{3, 4, 2, 14, 32, 0, 1, false, -1, false, false, wil, ail};                     /* 64 x 128 tiles, eight waves of 16 x 64 */
    else if (ring == 4 && kn.w8) pl.k = GemmKernel{3, 4, 2, 14, 32, 0, 2, false, -1, false, false, wil, ail};   /* 128^2 tiles, eight waves of 32 x 64 */
    else if (ail) return CVLM_E_UNSUPPORTED;                             /* no other kernel stages the activation image */
    else if (variant == 7) pl.k = GemmKernel{3, 2, 4, 5, 32, 0, 8};      /* same, every epilogue form (pixel shuffle, odd N, batched) */
#ifdef CVLM_PROBES
    else if (variant == 77) pl.k = GemmKernel{3, 2, 4, 5, 32, 7, 8};     /* probe: s_setprio around MFMA groups */
    else if (variant == 87) pl.k = GemmKernel{3, 2, 4, 5, 32, 8, 8};     /* probe: static priority for waves 4..7 */
    else if (variant == 4 && (a.K % 64) == 0) pl.k = GemmKernel{3, 2, 2, 2, 64};
    else if (variant == 24 && (a.K % 64) == 0) pl.k = GemmKernel{3, 2, 2, 2, 64, 2};   /* probe: DMA only, 128-byte rows (full L2 lines) */
    else if (variant == 21) pl.k = GemmKernel{3, 2, 2, 2, 32, 2};                      /* probe: DMA only, 64-byte rows, same tile */
    else if (variant == 5) pl.k = GemmKernel{3, 2, 4, 2, 32, 0, 8};      /* 256x256, 8 waves of 128x64 */
    else if (variant == 6) pl.k = GemmKernel{3, 2, 4, 4, 32, 0, 8};      /* same tile, mid-tile slot recycling */
    else if (variant == 8) pl.k = GemmKernel{3, 2, 2, 6, 32, 0, 8};      /* 256x128, 4 waves, one recycled slot, 2 WG/CU */
    else if (variant == 18 || variant == 28) pl.k = GemmKernel{3, 2, 2, 6, 32, variant / 10, 8};
    else if (variant == 17 || variant == 27) pl.k = GemmKernel{3, 2, 4, 5, 32, variant / 10, 8};
    else if (variant == 37) pl.k = GemmKernel{3, 2, 4, 5, 32, 3, 8};     /* probe: no epilogue stores */
    else if (variant == 57) pl.k = GemmKernel{3, 2, 4, 5, 32, 5, 8};     /* probe: epilogue staging only */
    else if (variant == 67) pl.k = GemmKernel{3, 2, 4, 5, 32, 6, 8};     /* probe: main loop only */
    else if (variant == 47 && kn.trace) pl.k = GemmKernel{3, 2, 4, 5, 32, 4, 8};   /* probe: per-workgroup timeline */
    else if (variant == 16 || variant == 26) pl.k = GemmKernel{3, 2, 4, 4, 32, variant / 10, 8};
    else if (variant == 15 || variant == 25) pl.k = GemmKernel{3, 2, 4, 2, 32, variant / 10, 8};
    else if (variant == 3) pl.k = GemmKernel{3, 2, 2, 3, 32};
#endif
    else pl.k = GemmKernel{3, 2, 2, ring >= 3 ? 10 + ring : 2, 32};
    return gemm_plan_finish(a, pl);
}

// The launches of one call: `out[0]`, or out[0] and out[1] for a column split.  Returns their number or a negative CVLM_E_* code.
template <class Cus>
inline int gemm_plan(const cvlm_gemm_args& g, const GemmKnobs& kn, bool have_ws, Cus&& cus, GemmPlan out[2]) {
    cvlm_gemm_args a = gemm_sanitised(g);
    out[0].n0 = 0;
    // ---- column split (one image): a grid of 256^2 tiles a little over one round -- lin1 of a ViT-H block at M = 4096 is 16 x 20 =
    // 320 tiles on 256 CUs -- spends a second round (or a chain of K-parts with its slab traffic and hand-offs, 58 us) on a
    // quarter round of work.  Two launches instead: the columns that make exactly one round of 256^2 tiles, then the rest as
    // 128^2 tiles on the deep-ring kernel, one round of those (30-40 us).  Whole tiles both times: no slabs, no flags, and the bits
    // of every output are those of an unsplit launch.  Plain and LayerNorm-folded epilogues only (their per-column operands just
    // move with the column offset).
    // (For grids of several rounds whose last round is partial -- proj / lin2 of a batch of 8 -- the same split measured slower,
    // profiles/r03_colsplit_ab.log; that form is gone.)
    if (kn.colsplit && a.split == 3 && a.conv_c <= 0 && a.batch == 1 && a.hm_S == 0 && a.ps_c2 == 0 && kn.variant == 0 && a.M <= 4096 &&
        !a.res_hi && !a.row_stats && !a.a_mx && !a.out_mx) {   // (an mx image's groups and scale bytes do not move with a plain column offset: ADVICE r5)
        const int nby = (a.M + 255) / 256, nbx = (a.N + 255) / 256;
        const int c0 = 256 / nby;                                        // column tiles of the first launch: one round of tiles
        const int n0 = c0 * 256, rest = a.N - n0;
        if (nbx > c0 && c0 * nby >= 232 && nbx * nby < 2 * 256 && rest >= 128 && (rest & 7) == 0 &&
            (long)((a.M + 127) / 128) * ((rest + 127) / 128) <= 256) {
            a.N = n0;
            int rc = gemm_plan_one(a, kn, have_ws, cus, out[0]);
            if (rc < 0) return rc;
            a.N = rest;
            out[1].n0 = n0;
            rc = gemm_plan_one(a, kn, have_ws, cus, out[1]);
            return rc < 0 ? rc : 2;
        }
    }
    return gemm_plan_one(a, kn, have_ws, cus, out[0]);
}

// "gemm_nt_kernel<3, 2, 4, 5, 32, 0, 8, false, 1, false, false, true, false, false>": the instantiation as a demangler prints it
inline void gemm_kernel_name(const GemmKernel& k, char* out, size_t cap) {
    auto b = [](bool v) { return v ? "true" : "false"; };
    snprintf(out, cap, "gemm_nt_kernel<%d, %d, %d, %d, %d, %d, %d, %s, %d, %s, %s, %s, %s, %s>", k.split, k.wm, k.wn, k.nstage, k.bk, k.dbg,
             k.mt, b(k.persist), k.epi, b(k.conv), b(k.sk), b(k.wil), b(k.ail), b(k.mx));
}

}  // namespace
}  // namespace cvlm_gemm_p
