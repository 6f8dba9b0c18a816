// Label maps: the per-thread logic of the cvlm_label_* kernels (labels.hip), written once for the device and for the
// sequential host entries cvlm_debug_label_*_host, which run these same functions pixel by pixel on the CPU.  No HIP call, no
// allocation.
//
//   - lb_image_ok: what is checked of an image's table entries before anything of it is read or stored;
//   - lb_value: the value v_p(y, x) of §19 -- sz_sigmoid and sz_blend of sized_logic.h on the taps of sz_axis_of, called, not copied;
//   - lb_score: s = w * v, one fp32 product, never contracted;
//   - lb_offer: one hypothesis offered to a pixel's running best (strict `>` in increasing k; a NaN weight or value takes no part);
//   - lb_kept: Mask2Former's per-query test on the three areas;
//   - lb_reduce_gt / lb_class: mmseg's reduce_zero_label and the class range of the histogram.
#pragma once
#include <math.h>
#include <stdint.h>

#include "sized_logic.h"

#define LB_HD SZ_HD

constexpr int LB_MAX_K = 16384;                                       // hypotheses per image: a winner is an int16
constexpr int LB_MAX_B = 65535;                                       // images of a call: a grid's y index
constexpr int LB_MAX_C = 65536;                                       // classes of the histogram
constexpr int LB_TILE = 1024;                                         // planes whose set bits a workgroup counts in LDS at a time
constexpr int LB_LDS_C = 4096;                                        // classes up to which 3 C counters are kept in a workgroup's LDS

// Image b of a call with n_pix pixels of maps: its size is a size and its slice [off, end) is its h * w pixels inside [0, n_pix)
LB_HD bool lb_image_ok(int h, int w, int64_t off, int64_t end, int64_t n_pix) {
    if (h < 1 || w < 1 || h > SZ_MAX_SIDE || w > SZ_MAX_SIDE) return false;
    return off >= 0 && end <= n_pix && end - off == (int64_t)h * w;
}

// units of 64 consecutive pixels of one row: per row, per image (h, w <= 16384: fewer than 2^23)
LB_HD int lb_units_per_row(int w) { return (w + 63) >> 6; }

// v_p(y, x): plane = one source plane of Hs x Ws
LB_HD float lb_value(const float* plane, int Ws, const sz_axis& ax, const sz_axis& ay) {
    const float* r0 = plane + (int64_t)ay.i0 * Ws;
    const float* r1 = plane + (int64_t)ay.i1 * Ws;
    return sz_blend(sz_sigmoid(r0[ax.i0]), sz_sigmoid(r0[ax.i1]), sz_sigmoid(r1[ax.i0]), sz_sigmoid(r1[ax.i1]), ax, ay);
}

LB_HD float lb_score(float w, float v) {
#pragma clang fp contract(off)
    return w * v;
}

// A pixel's state between calls: winner < 0 is "none" (best is then not read); bit is the winner's own sized bit
struct lb_best { float s; int k; bool bit; };

// Hypothesis k with weight w, value v and sized bit `bit` offered to the pixel.  It takes part iff neither w nor v is NaN; the first to
// take part is taken, a later one only if its score is larger: on equal scores the smaller k stays, +0 and -0 are equal.
LB_HD void lb_offer(lb_best& b, int k, float w, float v, bool bit) {
    if (w != w || v != v) return;
    const float s = lb_score(w, v);
    if (b.k < 0 || s > b.s) { b.s = s; b.k = k; b.bit = bit; }
}

// Mask2Former's panoptic_inference: `mask_area > 0 and original_area > 0 and mask.sum() > 0`, then `mask_area / original_area <
// overlap_threshold: continue`
LB_HD bool lb_kept(int won, int orig, int kept, double overlap_threshold) {
    if (won <= 0 || orig <= 0 || kept <= 0) return false;
    return !((double)won / (double)orig < overlap_threshold);
}

// mmseg's intersect_and_union with reduce_zero_label: 0 -> 255, then - 1, then 254 -> 255
LB_HD int lb_reduce_gt(int g) {
    if (g == 0) return 255;
    return g - 1 == 254 ? 255 : g - 1;
}
LB_HD bool lb_class(int v, int C) { return v >= 0 && v < C; }
