// Packed masks at each image's own size: the per-thread logic of cvlm_mask_pack_sized, written once for the device
// kernel (sized.hip) and for the sequential host entry cvlm_debug_mask_pack_sized_host, which runs these same functions pixel by pixel
// on the CPU.  No HIP call, no allocation.
//
// A sized plane is h rows of ws = ceil(w / 32) words in numpy.packbits' order (maskbits.h: cc_pack); the pad bits of a row,
// columns w .. 32 ws - 1, are 0.  bit(y, x) = (v(y, x) * 255.0f >= (float)level) with v the value of cvlm_mask_to_u8's resize -- cv::resize
// (INTER_LINEAR) on the fp32 sigmoid of the logits:
//   - sz_axis_of: the two taps and weights of one output coordinate -- the source coordinate formed in double and rounded to float;
//     columns zero the weight where the window leaves the row, rows clamp the indices and keep the weight;
//   - sz_sigmoid, sz_blend: the four probabilities, blended horizontally and then vertically, each blend two fp32 products and one fp32
//     sum (no contraction into an fma: the pragma holds on the host and on the device);
//   - sz_bit: the compare -- a NaN compares false;
//   - sz_word_of / sz_bit_of: the place of a pixel in its row's words (bit i of the unpacked word = pixel 32 c + i).
#pragma once
#include <math.h>
#include <stdint.h>

#include "maskbits.h"

#define SZ_HD CC_HD

constexpr int SZ_MAX_SIDE = 16384;                                    // h and w of a sized plane: 1 .. SZ_MAX_SIDE

struct sz_axis { int i0, i1; float w0, w1; };                        // value = src[i0] * w0 + src[i1] * w1

// Output coordinate d of n_dst along an axis of n_src samples, scale = (double)n_src / (double)n_dst.  Whatever d, n_dst and scale
// are, 0 <= i0, i1 <= n_src - 1: the float is compared before it becomes an int.
SZ_HD sz_axis sz_axis_of(int d, int n_src, double scale, bool column) {
#pragma clang fp contract(off)
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    const float fl = floorf(f);
    sz_axis a;
    if (!(fl >= 0.0f)) {                                              // left of the first sample (or no number at all)
        a.i0 = 0;
        a.i1 = column && n_src > 1 ? 1 : 0;                           // rows: floor + 1 <= 0 clamps to 0 as well
        f = column ? 0.0f : f - fl;
    } else if (fl >= (float)(n_src - 1)) {                            // on or right of the last sample
        a.i0 = a.i1 = n_src - 1;
        f = column ? 0.0f : f - fl;
    } else {
        a.i0 = (int)fl;
        a.i1 = a.i0 + 1;
        f -= fl;
    }
    if (!(f >= 0.0f && f <= 1.0f)) f = 0.0f;                          // only for coordinates that are no number
    a.w0 = 1.0f - f;
    a.w1 = f;
    return a;
}

SZ_HD float sz_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// p00 p01 / p10 p11: the probabilities at (y0, x0) (y0, x1) / (y1, x0) (y1, x1)
SZ_HD float sz_blend(float p00, float p01, float p10, float p11, const sz_axis& ax, const sz_axis& ay) {
#pragma clang fp contract(off)
    const float t0 = p00 * ax.w0 + p01 * ax.w1;
    const float t1 = p10 * ax.w0 + p11 * ax.w1;
    return t0 * ay.w0 + t1 * ay.w1;
}

SZ_HD bool sz_bit(float v, int level) { return v * 255.0f >= (float)level; }

// The whole pixel: plane = one source plane of Hs x Ws, ay the row's table
SZ_HD bool sz_pixel(const float* plane, int Ws, const sz_axis& ax, const sz_axis& ay, int level) {
    const float* r0 = plane + (int64_t)ay.i0 * Ws;
    const float* r1 = plane + (int64_t)ay.i1 * Ws;
    return sz_bit(sz_blend(sz_sigmoid(r0[ax.i0]), sz_sigmoid(r0[ax.i1]), sz_sigmoid(r1[ax.i0]), sz_sigmoid(r1[ax.i1]), ax, ay), level);
}

SZ_HD int sz_words_per_row(int w) { return (w + 31) >> 5; }
SZ_HD int64_t sz_word_of(int y, int x, int ws) { return (int64_t)y * ws + (x >> 5); }
SZ_HD uint32_t sz_bit_of(int x) { return 1u << (x & 31); }          // in the unpacked word; cc_pack turns it into the stored one

// What is checked before every store of plane p: its size is a size, its slice [off, end) is the plane's 4 h ws bytes, 4-byte aligned
// and inside bits[0, nbytes)
SZ_HD bool sz_plane_ok(int h, int w, int64_t off, int64_t end, int64_t nbytes) {
    if (h < 1 || w < 1 || h > SZ_MAX_SIDE || w > SZ_MAX_SIDE) return false;
    return off >= 0 && (off & 3) == 0 && end <= nbytes && end - off == (int64_t)4 * h * sz_words_per_row(w);
}
