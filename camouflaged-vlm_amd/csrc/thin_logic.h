// Thinning of sized planes: the per-thread logic of cvlm_mask_thin_sized, written once for the device kernels (thin.hip)
// and for the sequential host entry cvlm_debug_mask_thin_sized_host, which runs these same functions word by word on the CPU.  No HIP
// call, no allocation.
//
// The rule is Guo & Hall's two-subiteration thinning as Lam, Lee & Suen state it -- what MATLAB's bwmorph(X, 'thin') and scikit-image's
// thin run.  With the neighbours of p = (y, x) counter-clockwise from east, rows growing downwards,
//   x1 = (y, x+1)  x2 = (y-1, x+1)  x3 = (y-1, x)  x4 = (y-1, x-1)  x5 = (y, x-1)  x6 = (y+1, x-1)  x7 = (y+1, x)  x8 = (y+1, x+1)  x9 = x1,
//   G1   X_H = 1,  X_H = sum over i = 1 .. 4 of  !x(2i-1) & (x(2i) | x(2i+1));
//   G2   2 <= min(n1, n2) <= 3,  n1 = sum over k of x(2k-1) | x(2k),  n2 = sum over k of x(2k) | x(2k+1);
//   G3   (x2 | x3 | !x8) & x1 = 0  in the first subiteration,   G3'  (x6 | x7 | !x4) & x5 = 0  in the second,
// a subiteration clears at once every set pixel with G1 & G2 & G3 (G3').  Everything outside the plane, pad bits included, reads clear.
//   - th_word: the rule on 32 pixels at a time.  The eight neighbour planes of a word are its row neighbours as they are and the east /
//     west neighbours shifted by one with the carried bit of the neighbouring word; the three sums of four bits are bit-sliced adders
//     (th_add4: s0, s1, s2); G1 = s0 & !s1 & !s2, "n >= 2" = s1 | s2, "n = 4" = s2.
//   - th_col_mask: the pixels of word column c that lie below w.
//   - th_iter_ok, th_slice_ok: what a plane is refused for besides sized_logic.h's sz_plane_ok.
//   - th_resident, th_lds_bytes: whether a plane with a clear border of one row and one word column all round fits the resident
//     kernel's LDS budget.
#pragma once
#include <stdint.h>

#include "sized_logic.h"

#define TH_HD CC_HD

constexpr int TH_MAX_ITER = 1 << 30;                                  // max_iter of a plane: 0 (no limit) .. TH_MAX_ITER
constexpr int TH_MAX_STEPS = 1024;                                    // iterations the stepping path launches in one call
constexpr int TH_SHARE = 38;                                          // words of the bordered plane a thread of the resident kernel keeps
constexpr int TH_THREADS = 1024;                                      // threads of the resident kernel's workgroup at most
// The resident kernel's LDS budget: TH_SHARE words for each of 1024 threads = 155 648 bytes of the CU's 163 840, the rest left to the
// kernel's static LDS.  1024 x 1024 needs (1024 + 2)(32 + 2) * 4 = 139 536.
constexpr int64_t TH_LDS_BUDGET = (int64_t)4 * TH_SHARE * TH_THREADS;

TH_HD bool th_iter_ok(int max_iter) { return max_iter >= 0 && max_iter <= TH_MAX_ITER; }

// A refused plane's slice [off, end) can still be zeroed: whole words inside out_bits[0, nbytes)
TH_HD bool th_slice_ok(int64_t off, int64_t end, int64_t nbytes) {
    return off >= 0 && (off & 3) == 0 && end >= off && (end & 3) == 0 && end <= nbytes;
}

TH_HD int64_t th_lds_bytes(int h, int w) { return (int64_t)4 * (h + 2) * (sz_words_per_row(w) + 2); }
TH_HD bool th_resident(int h, int w) {
    return h >= 1 && w >= 1 && h <= SZ_MAX_SIDE && w <= SZ_MAX_SIDE && th_lds_bytes(h, w) <= TH_LDS_BUDGET;
}
// ... and within what ONE launch offers: `lds` bytes of dynamic LDS and `cells` = threads * TH_SHARE words to sweep.  The resident
// kernel and the stepping kernels of a call take the same two numbers, so that they agree on every plane.
TH_HD bool th_resident_in(int h, int w, int64_t lds, int64_t cells) {
    return th_resident(h, w) && th_lds_bytes(h, w) <= lds && (int64_t)h * (sz_words_per_row(w) + 2) <= cells;
}

// the pixels of word column c of a row of w pixels, as a mask of the unpacked word
TH_HD uint32_t th_col_mask(int c, int w) {
    const int valid = w - 32 * c;
    return valid >= 32 ? 0xffffffffu : valid <= 0 ? 0u : (1u << valid) - 1u;
}

// a + b + c + d of four bit planes -> the planes of the sum's bits 0, 1 and 2 (the sum is 4 only if all are set)
TH_HD void th_add4(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t& s0, uint32_t& s1, uint32_t& s2) {
    const uint32_t t1 = a ^ b, c1 = a & b, t2 = c ^ d, c2 = c & d, c3 = t1 & t2;
    s0 = t1 ^ t2;
    s1 = c1 ^ c2 ^ c3;
    s2 = c1 & c2;
}

// One word of one subiteration.  nl nc nr / cl cc cr / sl sc sr: the UNPACKED words of the rows y - 1, y, y + 1 at the word columns
// c - 1, c, c + 1, zero where the plane has none; mask = th_col_mask(c, w): the centre column's pad bits are cleared here, so the
// stored input may hold anything there (column c + 1 only gives its bit 0, which is a pixel whenever the column exists).
// -> the new word of (y, c): a subset of cc & mask.
TH_HD uint32_t th_word(bool second, uint32_t nl, uint32_t nc, uint32_t nr, uint32_t cl, uint32_t cc, uint32_t cr, uint32_t sl, uint32_t sc,
                       uint32_t sr, uint32_t mask) {
    nc &= mask;
    cc &= mask;
    sc &= mask;
    const uint32_t x1 = (cc >> 1) | (cr << 31), x5 = (cc << 1) | (cl >> 31);
    const uint32_t x2 = (nc >> 1) | (nr << 31), x4 = (nc << 1) | (nl >> 31), x3 = nc;
    const uint32_t x8 = (sc >> 1) | (sr << 31), x6 = (sc << 1) | (sl >> 31), x7 = sc;
    uint32_t s0, s1, s2;
    th_add4(~x1 & (x2 | x3), ~x3 & (x4 | x5), ~x5 & (x6 | x7), ~x7 & (x8 | x1), s0, s1, s2);
    const uint32_t g1 = s0 & ~s1 & ~s2;
    uint32_t a0, a1, a2, b0, b1, b2;
    th_add4(x1 | x2, x3 | x4, x5 | x6, x7 | x8, a0, a1, a2);
    th_add4(x2 | x3, x4 | x5, x6 | x7, x8 | x1, b0, b1, b2);
    const uint32_t g2 = (a1 | a2) & (b1 | b2) & (~a2 | ~b2);
    const uint32_t g3 = second ? ~((x6 | x7 | ~x4) & x5) : ~((x2 | x3 | ~x8) & x1);
    return cc & ~(g1 & g2 & g3);
}

// The same from a plane in memory, h rows of ws STORED words: word (y, c) of one subiteration, its neighbours read with the plane's
// bounds.  old = the word's own pixels before it; a clear word reads no neighbour.
TH_HD uint32_t th_step_word(bool second, const uint32_t* src, int h, int w, int ws, int y, int c, uint32_t& old) {
    const uint32_t mask = th_col_mask(c, w);
    old = cc_unpack(src[(int64_t)y * ws + c]) & mask;
    if (!old) return 0u;
    const bool up = y > 0, down = y + 1 < h, left = c > 0, right = c + 1 < ws;
    const int64_t m = (int64_t)y * ws + c, n = m - ws, s = m + ws;    // read only where the row and the column exist
    return th_word(second, up && left ? cc_unpack(src[n - 1]) : 0u, up ? cc_unpack(src[n]) : 0u, up && right ? cc_unpack(src[n + 1]) : 0u,
                   left ? cc_unpack(src[m - 1]) : 0u, old, right ? cc_unpack(src[m + 1]) : 0u, down && left ? cc_unpack(src[s - 1]) : 0u,
                   down ? cc_unpack(src[s]) : 0u, down && right ? cc_unpack(src[s + 1]) : 0u, mask);
}
