// COCO annotations on the device: the per-thread logic of cvlm_mask_rle_decode and cvlm_mask_inter_sized, written once
// for the device kernels (gt.hip) and for the sequential host entries cvlm_debug_mask_rle_decode_host / cvlm_debug_mask_inter_sized_host,
// which run these same functions on the CPU.  No HIP call, no allocation.  Everything is integers.
//
// Decoding is the encoder's stream (rle_logic.h) run backwards.  The counts c_0 .. c_{n-1} of a plane of h x w pixels have the prefix
// sums e_k = c_0 + ... + c_k; BOUNDARY k <= n - 2 toggles bit e_k of the plane's STREAM of h * w bits (position j = x * h + y,
// column-major), two boundaries at one position cancel, and the inclusive prefix XOR of the stream is the pixels: j is set iff an odd
// number of boundaries lie at or before it.
//   - gd_shape_ok, gd_slice_ok: what is checked before anything of a plane is read or stored;
//   - gd_toggle: the stream word and bit of a boundary position;
//   - gd_prefix_word: the prefix XOR inside one stream word; the words before it enter as the parity of their popcounts;
//   - gd_fetch: 32 consecutive stream bits from any position -- 32 rows of one pixel column;
//   - rl_gather (rle_logic.h) turns 32 such words, one per pixel column, into one word of a row: the transposition;
//   - gi_pair_ok, gi_word: the check of a pair of sized planes and the intersection of one word of them.
#pragma once
#include <stdint.h>

#include "rle_logic.h"
#include "sized_logic.h"

#define GT_HD CC_HD

constexpr int64_t GT_MAX_PIXELS = (int64_t)SZ_MAX_SIDE * SZ_MAX_SIDE;  // 2^28: h * w of a sized plane fits an int
constexpr int GT_WS_HEAD = 4;                                          // words of a plane's workspace before its stream: word 0 is the verdict

GT_HD int64_t gd_stream_words(int64_t pixels) { return (pixels + 31) >> 5; }
// Workspace of one plane of at most `pixels` pixels: the head, then the stream; a multiple of 16 bytes
GT_HD int64_t gd_plane_ws_bytes(int64_t pixels) { return ((GT_WS_HEAD + gd_stream_words(pixels)) * 4 + 15) / 16 * 16; }

// The size is a size and its stream fits the workspace slot of max_pixels pixels
GT_HD bool gd_shape_ok(int h, int w, int64_t max_pixels) {
    if (h < 1 || w < 1 || h > SZ_MAX_SIDE || w > SZ_MAX_SIDE) return false;
    return (int64_t)h * w <= max_pixels;
}

// The plane's counts are counts[off, end): not empty, forwards, inside counts[0, total)
GT_HD bool gd_slice_ok(int64_t off, int64_t end, int64_t total) { return off >= 0 && off < end && end <= total; }

// Boundary position e of a plane of hw pixels -> the stream word and bit it toggles; false: the position is no pixel's (a trailing zero
// count puts a boundary at hw; a sum that has left [0, hw) belongs to a plane that is refused anyway) and nothing may be toggled.
GT_HD bool gd_toggle(int64_t e, int hw, int& word, uint32_t& bit) {
    if (e < 0 || e >= hw) return false;
    word = (int)(e >> 5);
    bit = 1u << (e & 31);
    return true;
}

// Inclusive prefix XOR of the 32 bits of a stream word: bit i = XOR of the bits 0 .. i.  `before`: the parity of all set bits of the
// words before it.
GT_HD uint32_t gd_prefix_word(uint32_t w, uint32_t before) {
    w ^= w << 1;
    w ^= w << 2;
    w ^= w << 4;
    w ^= w << 8;
    w ^= w << 16;
    return before & 1u ? ~w : w;
}

// Stream bits at .. at + 31 as one word (bit i = position at + i); the stream has `words` words and bits at or beyond its end read as
// whatever the last word holds or as 0 -- the caller keeps only the rows that exist.  0 <= at < 32 * words.
GT_HD uint32_t gd_fetch(const uint32_t* stream, int64_t words, int at) {
    const int k = at >> 5, s = at & 31;
    const uint32_t lo = stream[k] >> s;
    return s && k + 1 < words ? lo | (stream[k + 1] << (32 - s)) : lo;
}

// Word c of row y of a sized plane of width w from the 32 fetched words v[0 .. 31] of its pixel columns 32 c .. 32 c + 31 (v[i] bit r =
// pixel (y0 + r, 32 c + i)): the unpacked word, pad columns clear.  stride: the distance of two columns' words.
GT_HD uint32_t gd_row_word(const uint32_t* v, int stride, int c, int w, int r) {
    const int n = w - 32 * c;
    return rl_gather(v, stride, n < 32 ? n : 32, r);
}

// ---- intersections of pairs of sized planes --------------------------------------------------------------------------------------------
// Pair (a, b) of planes of two tables: both indices in range, both planes pass §19's check against their own tensors, equal sizes.
GT_HD bool gi_pair_ok(int a, int b, int Pa, int Pb, const int* a_dims, const int64_t* a_off, int64_t a_bytes, const int* b_dims,
                      const int64_t* b_off, int64_t b_bytes) {
    if (a < 0 || a >= Pa || b < 0 || b >= Pb) return false;
    const int h = a_dims[2 * a], w = a_dims[2 * a + 1];
    if (h != b_dims[2 * b] || w != b_dims[2 * b + 1]) return false;
    return sz_plane_ok(h, w, a_off[a], a_off[a + 1], a_bytes) && sz_plane_ok(h, w, b_off[b], b_off[b + 1], b_bytes);
}

// Set pixels of stored words x AND y of word column c of a plane of width w: the columns at or beyond w do not count
GT_HD int gi_word(uint32_t x, uint32_t y, int c, int w) { return __builtin_popcount(x & y & cc_pack(rl_columns(c, w))); }
