// Morphology of packed masks: the per-thread logic of cvlm_mask_morph, written once for the device kernel (morph.hip)
// and for the sequential host entry cvlm_debug_mask_morph_host, which runs these same functions word by word on the CPU.  No HIP call,
// no allocation.
//
// A plane is H rows of W / 32 words in numpy.packbits' order; cc_unpack (maskbits.h) turns a stored word into bit i = pixel i
// of the word, so that "x + 1" is "bit << 1" and the word to the LEFT of a word holds the pixels BELOW its bit 0.  The structuring
// element is the (2r + 1)^2 square, 1 <= r <= 16, and it is separable: a horizontal pass inside each row (mo_hdilate / mo_herode, one
// neighbour word each side always suffices) and a vertical pass over the rows max(0, y - r) .. min(H - 1, y + r) (mo_column).  Pixels
// outside the plane influence neither operator: dilation sees them clear, erosion sees them set -- max_pool2d's -inf padding.
#pragma once
#include <stdint.h>

#include "maskbits.h"

#define MO_HD CC_HD

constexpr int MO_MAXR = 16;

// `acc` ORed with itself shifted up (UP) or down by 1 .. r bits, by doubling: after a step that has covered c shifts the next one
// adds min(c + 1, r - c) more -- 5 steps for r = 16, not 16.
template <bool UP>
MO_HD uint64_t mo_smear(uint64_t acc, int r) {
    for (int covered = 0; covered < r;) {
        const int step = covered + 1 < r - covered ? covered + 1 : r - covered;
        acc |= UP ? acc << step : acc >> step;
        covered += step;
    }
    return acc;
}

// The centre word with every pixel set that has a set pixel within r columns in the 96-pixel window left | centre | right (unpacked
// words; 0 for a word beyond the row's end).  Pixels left of and inside the centre reach upwards through (centre : left), pixels
// right of and inside it reach downwards through (right : centre).
MO_HD uint32_t mo_hdilate(uint32_t left, uint32_t centre, uint32_t right, int r) {
    const uint64_t up = mo_smear<true>((uint64_t)centre << 32 | left, r);
    const uint64_t down = mo_smear<false>((uint64_t)right << 32 | centre, r);
    return (uint32_t)(up >> 32) | (uint32_t)down;
}

// Erosion is dilation of the complement, and a word beyond the row's end is 0 in the complement as well: there it means "outside is
// set".  has_left / has_right: the neighbour word lies inside the row.
MO_HD uint32_t mo_herode(uint32_t left, uint32_t centre, uint32_t right, bool has_left, bool has_right, int r) {
    return ~mo_hdilate(has_left ? ~left : 0u, ~centre, has_right ? ~right : 0u, r);
}

// Word c of row y of a plane of wpr words per row, unpacked; 0 beyond either end of the row
MO_HD uint32_t mo_fetch(const uint32_t* row, int c, int wpr) { return c >= 0 && c < wpr ? cc_unpack(row[c]) : 0u; }

// The vertical pass of one word column: hd / he point at the horizontally dilated / eroded word of the FIRST row of the window, rows
// are `stride` words apart, n = the rows of the window that lie inside the plane (the caller clips; nothing is read outside).
MO_HD void mo_column(const uint32_t* hd, const uint32_t* he, int stride, int n, uint32_t& dil, uint32_t& ero) {
    uint32_t d = 0u, e = 0xffffffffu;
    for (int k = 0; k < n; ++k) {
        d |= hd[(int64_t)k * stride];
        e &= he[(int64_t)k * stride];
    }
    dil = d;
    ero = e;
}
