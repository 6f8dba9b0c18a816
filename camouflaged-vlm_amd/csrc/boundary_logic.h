// Boundaries of sized planes: the per-thread logic of cvlm_mask_boundary_sized, written once for the device kernels
// (boundary.hip) and for the sequential host entry cvlm_debug_mask_boundary_sized_host, which runs these same functions chunk by chunk
// and pixel by pixel on the CPU.  No HIP call, no allocation.
//
// The boundary of a plane X (h x w) at radius d is X & ~ero, ero(y, x) = AND of X over |y' - y| <= d, |x' - x| <= d with every pixel
// outside the plane read as CLEAR -- boundary_iou_api's mask_to_boundary: copyMakeBorder(1, constant 0), d erosions by ones((3, 3)),
// the crop.  The window is a product, so the erosion is a row pass and a column pass, and neither costs more for a larger d:
//   - rows:    hero(y, x) = the run of set pixels ending at x and the run starting at x, each counted with x itself, both reach d + 1.
//              A CHUNK is 64 consecutive pixels of a row as a 64-bit mask, bit i = pixel i (bd_chunk: pixels >= w are clear, whatever
//              the pad bits hold); the run lengths come from a count of leading / trailing zeros of the complement plus one integer
//              carried from the neighbouring chunk (bd_run_end, bd_run_start); outside the row the carry is 0.
//   - columns: count(y, x) = the consecutive rows up to y with hero set (bd_count); ero(y - d, x) = count(y, x) >= 2 d + 1; a row with
//              y + d > h - 1 is never eroded.  The rows are cut into SEGMENTS of bd_seg_rows(d) rows; a segment's counts start 2 d
//              rows early (d rows before its first row, the d rows its first output looks ahead): a count that started later can only
//              be too small by rows that lie more than 2 d back, which `>= 2 d + 1` cannot tell.
#pragma once
#include <stdint.h>

#include "sized_logic.h"

#define BD_HD CC_HD

constexpr int BD_MAX_RADIUS = 16384;                                  // the radius of a plane: 1 .. BD_MAX_RADIUS

BD_HD bool bd_radius_ok(int d) { return d >= 1 && d <= BD_MAX_RADIUS; }

// A refused plane's slice [off, end) can still be zeroed: whole words inside out_bits[0, nbytes)
BD_HD bool bd_slice_ok(int64_t off, int64_t end, int64_t nbytes) {
    return off >= 0 && (off & 3) == 0 && end >= off && (end & 3) == 0 && end <= nbytes;
}

// The chunk that starts at pixel x0 < w of a row of w pixels, from its two UNPACKED words (hi = 0 where the row has no second one)
BD_HD uint64_t bd_chunk(uint32_t lo, uint32_t hi, int x0, int w) {
    const uint64_t m = (uint64_t)lo | ((uint64_t)hi << 32);
    const int valid = w - x0;
    return valid >= 64 ? m : m & (((uint64_t)1 << valid) - 1);
}

// Length of the run of set pixels that ends at pixel i of chunk m, counted with i (0: pixel i is clear); carry = the run that ends at
// the pixel before the chunk
BD_HD int bd_run_end(uint64_t m, int i, int carry) {
    const uint64_t z = ~m & (((uint64_t)2 << i) - 1);                 // the clear pixels at or before i; i = 63: 2 << 63 wraps to 0
    return z ? i - (63 - __builtin_clzll(z)) : i + 1 + carry;
}
// Length of the run of set pixels that starts at pixel i of chunk m, counted with i; carry = the run that starts behind the chunk
BD_HD int bd_run_start(uint64_t m, int i, int carry) {
    const uint64_t z = ~m >> i;                                       // the clear pixels at or behind i
    return z ? __builtin_ctzll(z) : 64 - i + carry;
}
// A run, counted with its pixel, covers the d pixels on its side of it; a pixel survives the row pass iff both of its runs do
BD_HD bool bd_run_reaches(int run, int d) { return run >= d + 1; }

// Consecutive rows with the row pass's bit set, up to and with this one
BD_HD int bd_count(int count, bool on) { return on ? count + 1 : 0; }
BD_HD bool bd_col_erodes(int count, int d) { return count >= 2 * d + 1; }

// Rows of a segment of the column pass: at least 4 d, so that the 2 d rows of warm-up stay under half of a segment's work, at least
// 128, a multiple of the 32 rows a wave loads at once
BD_HD int bd_seg_rows(int d) {
    const int s = 4 * d < 128 ? 128 : 4 * d;
    return (s + 31) & ~31;
}
