// Run-length encoding of packed masks: the per-thread logic of cvlm_mask_rle_count / cvlm_mask_rle_emit, written once
// for the device kernels (rle.hip) and for the sequential host entry cvlm_debug_mask_rle_host, which runs these same functions word by
// word on the CPU.  No HIP call, no allocation.  Everything is integers.
//
// A plane is H rows of wpr = W / 32 words in numpy.packbits' order, of which the columns below the true width Wt <= W are the image
// (Wt = W for the planes of cvlm_mask_pack; the sized planes of cvlm_mask_pack_sized end inside their last word: DESIGN.md §19);
// cc_unpack (maskbits.h) turns a stored word into bit i = pixel i of the word.  COCO's order is column-major: position j = x * H + y.  A TRANSITION is a position whose pixel differs from
// the pixel of position j - 1 (from 0 at j = 0); the counts of the encoding are the differences of consecutive transition positions.
//   - rl_transition: the transition bits of one word of the row-major plane -- one XOR with the word of the row above; row 0 takes
//     the last row of the previous column, which is the last row's word shifted up by one pixel with the word before it carrying in.
//   - rl_gather: 32 consecutive rows of one pixel column of those words as one word -- the transposition.
//   - rl_place: where that word lies in the STREAM, the H * Wt transition bits in position order, word k = positions 32 k .. 32 k + 31.
//   - rl_last: the scan's two quantities of a stream word; rl_emit_word: the counts of a stream word's transitions.
#pragma once
#include <stdint.h>

#include "maskbits.h"

#define RL_HD CC_HD

// The columns of word c that exist in a plane of true width Wt (32 (wpr - 1) < Wt <= 32 wpr): all of them but in the last word of a
// row, whose pad columns are the tail of the column-major order and no part of the image.
RL_HD uint32_t rl_columns(int c, int Wt) {
    const int n = Wt - 32 * c;
    return n >= 32 ? 0xffffffffu : (n <= 0 ? 0u : (1u << n) - 1u);
}

// Transition bits of word c of row y (unpacked form: bit i = pixel 32 c + i), of the columns below Wt only: bit i of the result is a
// function of the pixels of the columns i and i - 1, so whatever the pad bits hold does not reach it.  plane: the stored words of ONE
// plane -- nothing of a neighbouring plane is read, so the last pixel of plane p never reaches plane p + 1.
RL_HD uint32_t rl_transition(const uint32_t* plane, int y, int c, int H, int wpr, int Wt) {
    const uint32_t m = cc_unpack(plane[(int64_t)y * wpr + c]), cols = rl_columns(c, Wt);
    if (y > 0) return (m ^ cc_unpack(plane[(int64_t)(y - 1) * wpr + c])) & cols;
    const uint32_t* last = plane + (int64_t)(H - 1) * wpr;            // pixel (0, x) follows pixel (H - 1, x - 1); (0, 0) follows a 0
    const uint32_t carry = c > 0 ? cc_unpack(last[c - 1]) >> 31 : 0u;
    return (m ^ ((cc_unpack(last[c]) << 1) | carry)) & cols;
}

// Bit `bit` of t[0], t[stride], ..., t[(n - 1) * stride] as bits 0 .. n - 1 of one word, 1 <= n <= 32: rows become bits.
RL_HD uint32_t rl_gather(const uint32_t* t, int stride, int n, int bit) {
    uint32_t v = 0u;
#pragma unroll
    for (int i = 0; i < 32; ++i)
        if (i < n) v |= ((t[i * stride] >> bit) & 1u) << i;
    return v;
}

// The n <= 32 transition bits v of rows y .. y + n - 1 of pixel column x start at stream bit x * H + y: they lie in stream word `word`
// as `lo` and, where they pass its end, in word + 1 as `hi` (0 otherwise: then word + 1 may not exist).  H * W < 2^31.
RL_HD void rl_place(uint32_t v, int x, int y, int H, int& word, uint32_t& lo, uint32_t& hi) {
    const int at = x * H + y, s = at & 31;
    word = at >> 5;
    lo = v << s;
    hi = s ? v >> (32 - s) : 0u;
}

// The position of the last transition of stream word k, 0 for a word without one (positions only grow, and 0 is t_{-1})
RL_HD int rl_last(uint32_t w, int k) { return w ? 32 * k + 31 - __builtin_clz(w) : 0; }

// The counts of stream word k's transitions.  rank: the transitions before word k; prev: the position of the last of them, 0 without
// one; the plane's slice is counts[off, off + cap) and `ok` says that it lies inside counts[0, total).  A store that would leave the
// slice is dropped; returns 1 if one was, 0 otherwise.
RL_HD int rl_emit_word(uint32_t w, int k, int rank, int prev, int32_t* counts, int64_t off, int64_t cap, bool ok) {
    int dropped = 0;
    while (w) {
        const int pos = 32 * k + __builtin_ctz(w);
        if (ok && rank < cap) counts[off + rank] = pos - prev;
        else dropped = 1;
        prev = pos;
        ++rank;
        w &= w - 1u;
    }
    return dropped;
}

// The tail run: count number `rank` = all transitions of the plane, from the last of them (0 without one) to the plane's end
RL_HD int rl_emit_tail(int HW, int rank, int prev, int32_t* counts, int64_t off, int64_t cap, bool ok) {
    if (ok && rank < cap) { counts[off + rank] = HW - prev; return 0; }
    return 1;
}
