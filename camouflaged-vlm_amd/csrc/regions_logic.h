// Instances of sized planes: the per-thread logic of cvlm_mask_regions_sized and cvlm_region_alpha, written once for the
// device kernels (regions.hip) and for the sequential host entries cvlm_debug_mask_regions_sized_host and cvlm_debug_region_alpha_host,
// which run these same functions word by word and pixel by pixel on the CPU.  No HIP call, no allocation.
//
// A sized plane of h x w pixels is labelled as h rows of ws = ceil(w / 32) words: the labelling is components_logic.h's -- runs of a
// word, the neighbour rule, find and union -- on the plane with its pad bits cleared, whose run starts are PADDED indices
// i = (y * ws + c) * 32 + bit.  Padded indices order as raster indices do, so the forest's root is still the region's lowest pixel;
// rg_seed_of turns it into the interface's seed y * w + x.
//   - rg_workspace: the four arrays of components.hip's workspace for one plane of `words` words: 448 bytes per word.
//   - rg_clean_word: a stored word of column c without the pad bits of a row of w pixels.
//   - rg_counts: whether a root of `area` pixels is a region of the call (at least max(min_area, 1) pixels).
//   - rg_write_row: one row of the table, or the filler.
//   - rg_ranks / rg_rank_word: behind the selection the area slot of every root holds its rank in the table (0 .. M - 1) or -1.  A
//     word has at most 16 runs; rg_ranks reads the rank of each once into 16 bytes of registers and the set of ranks that occur,
//     rg_rank_word builds the word of one rank from them without another read.
//   - rg_out_plane: where plane (p, m) of out_bits lies.
//   - rg_gate: the plane's bits as 0 / 1 resized to R x R at one output pixel, cvlm_bilinear's arithmetic on four bit reads.
#pragma once
#include <stdint.h>

#include "components_logic.h"
#include "sized_logic.h"
#include "thin_logic.h"

#define RG_HD CC_HD

constexpr int RG_MAXM = 64;                                           // rows of the table, and planes a plane is split into
constexpr int64_t RG_WS_PER_WORD = 448;                               // bytes of workspace per word of a plane: 14 per padded pixel

struct rg_ws { int* parent; int* list; int* area; cc_box* box; };
// base: 16-byte aligned; words >= 1.  Every array starts on a multiple of 64 bytes of base.
RG_HD rg_ws rg_workspace(void* base, int64_t words) {
    char* b = (char*)base;
    return rg_ws{(int*)b, (int*)(b + 64 * words), (int*)(b + 128 * words), (cc_box*)(b + 192 * words)};
}

RG_HD uint32_t rg_clean_word(uint32_t stored, int c, int w) { return cc_pack(cc_unpack(stored) & th_col_mask(c, w)); }

RG_HD bool rg_counts(int area, int min_area) { return area >= (min_area > 1 ? min_area : 1); }

// padded run start -> y * w + x
RG_HD int rg_seed_of(int padded, int ws, int w) {
    const int y = padded / (32 * ws);
    return y * w + (padded - y * 32 * ws);
}

// row: int32 [6]; key = cc_rank_key(area, padded seed) of the winner, 0 for none
RG_HD void rg_write_row(int32_t* row, uint64_t key, const cc_box* box, int ws, int w) {
    if (key) {
        const int seed = cc_key_seed(key);
        const cc_box b = box[seed >> 1];
        row[0] = (int)(key >> 32); row[1] = b.x0; row[2] = b.y0; row[3] = b.x1; row[4] = b.y1; row[5] = rg_seed_of(seed, ws, w);
    } else {
        row[0] = 0; row[1] = row[2] = row[3] = row[4] = row[5] = -1;
    }
}

// The ranks of the runs of the unpacked word w != 0 whose first pixel has the padded index base: byte j of lo (runs 0 .. 7) and hi
// (runs 8 .. 15) = the rank of run j, 0xff for a region outside the table; -> the set of ranks that occur, bit m = rank m.
// parent is flat: a run start's parent is its root; rank = the area array behind the selection.
RG_HD uint64_t rg_ranks(uint32_t w, int base, const int* parent, const int* rank, uint64_t& lo, uint64_t& hi) {
    uint64_t present = 0;
    lo = hi = 0;
    int j = 0;
    for (uint32_t rest = w; rest; ++j) {
        int s, e;
        cc_next_run(w, rest, s, e);
        const int r = rank[parent[(base + s) >> 1] >> 1];
        const uint64_t byte = (uint64_t)(r < 0 ? 0xff : r) << (8 * (j & 7));
        if (j < 8) lo |= byte; else hi |= byte;
        if (r >= 0) present |= (uint64_t)1 << r;
    }
    return present;
}

// the runs of w whose rank is m
RG_HD uint32_t rg_rank_word(uint32_t w, uint64_t lo, uint64_t hi, int m) {
    uint32_t out = 0u;
    int j = 0;
    for (uint32_t rest = w; rest; ++j) {
        int s, e;
        cc_next_run(w, rest, s, e);
        const int r = (int)(((j < 8 ? lo : hi) >> (8 * (j & 7))) & 0xff);
        if (r == m) out |= cc_span(s, e);
    }
    return out;
}

// plane (p, m) of out_bits, for the input plane at [off, end): sized_tables' layout of every size repeated M times
RG_HD int64_t rg_out_plane(int64_t off, int64_t end, int M, int m) { return (int64_t)M * off + (int64_t)m * (end - off); }

// ---- cvlm_region_alpha ----------------------------------------------------------------------------------------------------------------
// pixel (y, x) of a plane of ws stored words per row, as 0.0f or 1.0f; y < h and x < w: never a pad bit
RG_HD float rg_bit(const uint32_t* plane, int ws, int y, int x) {
    return (float)((cc_unpack(plane[sz_word_of(y, x, ws)]) >> (x & 31)) & 1u);
}

// the source coordinate of output o: cvlm_bilinear's (rowops.hip: bilinear_src), float32, clamped below
RG_HD float rg_src(float scale, int o) {
#pragma clang fp contract(off)
    const float f = scale * ((float)o + 0.5f) - 0.5f;
    return f < 0.f ? 0.f : f;
}

// the gate at output pixel (oy, ox) of R x R over a plane of h x w
RG_HD float rg_gate(const uint32_t* plane, int h, int w, int R, int oy, int ox) {
#pragma clang fp contract(off)
    const int ws = sz_words_per_row(w);
    const float fy = rg_src((float)h / (float)R, oy), fx = rg_src((float)w / (float)R, ox);
    // fy <= h - 0.5 - 0.5 h / R before rounding, so the clamps never bind: they are the bound check of the four reads
    const int y0 = (int)fy < h - 1 ? (int)fy : h - 1, x0 = (int)fx < w - 1 ? (int)fx : w - 1;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    const float v00 = rg_bit(plane, ws, y0, x0), v01 = rg_bit(plane, ws, y0, x1);
    const float v10 = rg_bit(plane, ws, y1, x0), v11 = rg_bit(plane, ws, y1, x1);
    return (1.0f - ly) * ((1.0f - lx) * v00 + lx * v01) + ly * ((1.0f - lx) * v10 + lx * v11);
}
