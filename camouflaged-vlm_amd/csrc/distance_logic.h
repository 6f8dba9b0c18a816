// Distance maps of sized planes and directed surface totals: the per-thread logic of cvlm_mask_distance_sized and
// cvlm_mask_surface_totals, written once for the device kernels (distance.hip) and for the sequential host entries
// cvlm_debug_mask_distance_sized_host / cvlm_debug_mask_surface_totals_host, which run these same functions pixel by pixel on the CPU.
// No HIP call, no allocation.  All integers but the one square root of dt_pixel.
//
// D2(y, x) = min over the set pixels (y', x') of a plane of (y - y')^2 + (x - x')^2, an int32 (at most 2 * 16383^2 < 2^31), 0 on a set
// pixel; DT_FAR where no set pixel is within reach.  The minimum separates:
//   - rows:    f(y, x) = the horizontal distance to the nearest set pixel of row y, a uint16, DT_ROW_FAR where the row has none within
//              reach.  A CHUNK is 64 consecutive pixels of a row as a 64-bit mask, bit i = pixel i (dt_chunk: pixels >= w are clear,
//              whatever the pad bits hold); the GAP of pixel i towards the row's start (dt_gap_back) and towards its end
//              (dt_gap_fwd) comes from a count of leading / trailing zeros plus one integer carried from the neighbouring chunk,
//              DT_NONE (or more) where no set pixel lies that way; f is the smaller of the two (dt_row_value).
//   - columns: D2(y, x) = min over y' of (y - y')^2 + f(y', x)^2 (dt_column): rows y - k and y + k for k = 0, 1, ... until k^2 >= the
//              best so far, k > reach, or both rows have left the plane.  O(min(D, reach)) reads per pixel.
// A reach R >= 1 keeps D2 <= R^2 and turns everything else into DT_FAR: a minimiser within R has |dy| <= R and f <= |dx| <= R, so
// neither cut loses it.  R = 0: unlimited.
#pragma once
#include <math.h>
#include <stdint.h>

#include "sized_logic.h"

#define DT_HD CC_HD

constexpr int32_t DT_FAR = 0x7fffffff;                               // D2 of a pixel with no set pixel within reach
constexpr int DT_MAX_REACH = 23170;                                   // reach and tolerance radii: 0 .. 23170, 23170^2 < 2^31
constexpr int DT_ROW_FAR = 0xFFFF;                                    // f of a pixel with no set pixel of its row within reach
constexpr int DT_NONE = 1 << 24;                                      // a gap >= DT_NONE: no set pixel that way (a real gap is < 2^14)
constexpr int64_t DT_NONE64 = (int64_t)1 << 62;
constexpr int DT_MAX_T = 8;                                           // tolerance radii of a pair

DT_HD bool dt_reach_ok(int R) { return R >= 0 && R <= DT_MAX_REACH; }

// The pixel slice [off, end) of a plane of h x w: exactly h * w entries inside [0, n_pix)
DT_HD bool dt_slice_ok(int h, int w, int64_t off, int64_t end, int64_t n_pix) {
    return off >= 0 && end <= n_pix && end - off == (int64_t)h * w;
}
// A refused plane's slice can still be filled: forwards and inside [0, n_pix)
DT_HD bool dt_slice_sound(int64_t off, int64_t end, int64_t n_pix) { return off >= 0 && end >= off && end <= n_pix; }

// The chunk that starts at pixel x0 < w of a row of w pixels, from its two UNPACKED words (hi = 0 where the row has no second one)
DT_HD uint64_t dt_chunk(uint32_t lo, uint32_t hi, int x0, int w) {
    const uint64_t m = (uint64_t)lo | ((uint64_t)hi << 32);
    const int valid = w - x0;
    return valid >= 64 ? m : m & (((uint64_t)1 << valid) - 1);
}

// Distance from pixel i of chunk m to the nearest set pixel at or before it; carry = that of the pixel before the chunk (DT_NONE
// before the row).  At most 64 is added per chunk and a row has 256 chunks: a gap that started at DT_NONE stays >= DT_NONE, no overflow.
DT_HD int dt_gap_back(uint64_t m, int i, int carry) {
    const uint64_t z = m & (((uint64_t)2 << i) - 1);                  // the set pixels at or before i; i = 63: 2 << 63 wraps to 0
    return z ? i - (63 - __builtin_clzll(z)) : i + 1 + carry;
}
// Distance from pixel i of chunk m to the nearest set pixel at or behind it; carry = that of the pixel behind the chunk
DT_HD int dt_gap_fwd(uint64_t m, int i, int carry) {
    const uint64_t z = m >> i;
    return z ? __builtin_ctzll(z) : 64 - i + carry;
}
// What the first walk parks in f: the gap itself, DT_ROW_FAR for none
DT_HD uint16_t dt_row_park(int gap) { return (uint16_t)(gap >= DT_NONE ? DT_ROW_FAR : gap); }
// f of a pixel from its parked gap and its other gap, at reach R
DT_HD uint16_t dt_row_value(int parked, int gap, int R) {
    const int f = parked < gap ? parked : gap;                        // DT_ROW_FAR > every real gap
    const int limit = R >= 1 && R < SZ_MAX_SIDE ? R : SZ_MAX_SIDE - 1;
    return (uint16_t)(f > limit ? DT_ROW_FAR : f);
}

// D2 of pixel (y, x) from the plane's f (row pitch w), at reach R.  The best is kept in 64 bits until it is stored.
DT_HD int32_t dt_column(const uint16_t* f, int h, int w, int y, int x, int R) {
    int64_t best = DT_NONE64;
    for (int k = 0;; ++k) {
        const int64_t kk = (int64_t)k * k;
        if (kk >= best || (R >= 1 && k > R)) break;
        const bool up = y - k >= 0, down = y + k < h;
        if (!up && !down) break;
        if (up) {
            const int64_t v = f[(int64_t)(y - k) * w + x];
            if (v != DT_ROW_FAR && kk + v * v < best) best = kk + v * v;
        }
        if (down && k) {
            const int64_t v = f[(int64_t)(y + k) * w + x];
            if (v != DT_ROW_FAR && kk + v * v < best) best = kk + v * v;
        }
    }
    if (best == DT_NONE64 || (R >= 1 && best > (int64_t)R * R)) return DT_FAR;
    return (int32_t)best;
}

// ---- directed surface totals: the set pixels of plane A against the distance map of plane B ---------------------------------------------
// One thread's, or one host loop's, share of a pair
struct dt_totals {
    int n = 0, far = 0, max_d2 = -1;
    int within[DT_MAX_T] = {};
    int64_t sum_d2 = 0;
    double sum_d = 0.0;
};

// One set pixel of A whose entry of B's map is d2; r2[k] = the squares of the pair's radii, formed in 64 bits, -1 for k >= T (the loop
// has a fixed length, so that the counts stay in registers)
DT_HD void dt_pixel(dt_totals& t, int32_t d2, const int64_t (&r2)[DT_MAX_T]) {
    ++t.n;
    if (d2 == DT_FAR || d2 < 0) {                                     // a map holds no negative entry; one is far, not a distance
        ++t.far;
        return;
    }
#pragma unroll
    for (int k = 0; k < DT_MAX_T; ++k) t.within[k] += (int64_t)d2 <= r2[k];
    t.max_d2 = d2 > t.max_d2 ? d2 : t.max_d2;
    t.sum_d2 += d2;
#if defined(__HIP_DEVICE_COMPILE__)
    t.sum_d += __dsqrt_rn((double)d2);                               // correctly rounded, like the host's sqrt
#else
    t.sum_d += sqrt((double)d2);
#endif
}

// What makes pair (ia, ib) sound: both indices in range, A's plane a sized plane, B's map the same size in a slice of its own, every
// radius in range.  The same for every thread of a pair; nothing of a refused pair is read.
DT_HD bool dt_pair_ok(int ia, int ib, int Pa, int Pb, const int32_t* a_dims, const int64_t* a_offsets, int64_t a_bytes,
                      const int32_t* b_dims, const int64_t* b_pix_offsets, int64_t b_n_pix, const int32_t* radii, int T) {
    if (ia < 0 || ia >= Pa || ib < 0 || ib >= Pb) return false;
    const int h = a_dims[2 * ia], w = a_dims[2 * ia + 1];
    if (!sz_plane_ok(h, w, a_offsets[ia], a_offsets[ia + 1], a_bytes)) return false;
    if (b_dims[2 * ib] != h || b_dims[2 * ib + 1] != w) return false;
    if (!dt_slice_ok(h, w, b_pix_offsets[ib], b_pix_offsets[ib + 1], b_n_pix)) return false;
    for (int k = 0; k < T; ++k)
        if (!dt_reach_ok(radii[k])) return false;
    return true;
}

// The valid pixels of word column c of a row of w pixels, as a mask of the unpacked word
DT_HD uint32_t dt_word_mask(int c, int w) {
    const int valid = w - 32 * c;
    return valid >= 32 ? 0xffffffffu : (1u << valid) - 1u;
}
