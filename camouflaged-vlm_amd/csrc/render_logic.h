// Rendering on the device: the per-thread logic of cvlm_render, written once for the device kernel (render.hip) and for
// the sequential host entry cvlm_debug_render_host, which runs these same functions pixel by pixel on the CPU.  No HIP call, no
// allocation.  One float32 rule, never contracted into an fma; everything else is integers.
//
//   - rd_blend:       the only arithmetic -- c (1 - a) + col a in float32, two products and a sum each rounded on its own, then round half
//                     to even and saturate: cv2.addWeighted's documented result on uint8 where both products are exact (a = 0.5); its
//                     steps rd_rest, rd_weigh and rd_mix are what the kernel calls, with 1 - a and col a formed once per table row;
//   - rd_alpha_ok:    an opacity that paints -- a number in [0, 1];
//   - rd_image_ok:    what is checked of an image's table entries before a byte of it is read or stored;
//   - rd_layer_of:    a layer's descriptor row taken apart and checked against the image's size and the call's buffers;
//   - rd_bit:         one pixel of a sized plane (pad bits are never asked for: x < w);
//   - rd_edge:        a pixel of a label map with a 4-neighbour inside the image of another raw id.
#pragma once
#include <math.h>
#include <stdint.h>

#include "sized_logic.h"

#define RD_HD SZ_HD

constexpr int RD_MAX_B = 1 << 16;                                     // images of a call
constexpr int RD_MAX_L = 1 << 20;                                     // layers of a call
constexpr int RD_MAX_T = 1 << 24;                                     // rows of the colour table

enum { RD_BITS = 0, RD_LEVELS = 1, RD_LABELS = 2 };                   // kind
enum { RD_EDGES = 1, RD_INVERT = 2 };                                 // flags
enum { RD_IMAGE_REFUSED = 1, RD_LAYER_SKIPPED = 2, RD_ROW_REFUSED = 4 };   // status bits

// c b + q rounded to an integer, q = col a formed beforehand: the two products and the sum each rounded on their own
RD_HD float rd_mix(uint8_t c, float b, float q) {
#pragma clang fp contract(off)
    const float p = (float)c * b;
    return rintf(p + q);                                              // half to even in the default rounding mode, host and device
}
RD_HD float rd_weigh(uint8_t col, float a) {
#pragma clang fp contract(off)
    return (float)col * a;
}
RD_HD float rd_rest(float a) {
#pragma clang fp contract(off)
    return 1.0f - a;
}
RD_HD uint8_t rd_blend(uint8_t c, uint8_t col, float a) {
    const float v = rd_mix(c, rd_rest(a), rd_weigh(col, a));
    return (uint8_t)(v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v));
}

RD_HD bool rd_alpha_ok(float a) { return a >= 0.0f && a <= 1.0f; }    // a NaN fails both

RD_HD int64_t rd_image_bytes(int h, int w) { return (int64_t)3 * h * w; }

// Image b of the tables: a size that is a size, a slice [off, end) on 4-byte boundaries inside [0, img_bytes) that is its 3 h w bytes and
// the 0 .. 3 pad bytes behind them, and a layer range [l0, l1) that runs forwards inside [0, L]
RD_HD bool rd_image_ok(int h, int w, int64_t off, int64_t end, int64_t img_bytes, int l0, int l1, int L) {
    if (h < 1 || w < 1 || h > SZ_MAX_SIDE || w > SZ_MAX_SIDE) return false;
    if (off < 0 || (off & 3) != 0 || end > img_bytes || end - off != ((rd_image_bytes(h, w) + 3) & ~(int64_t)3)) return false;
    return l0 >= 0 && l1 >= l0 && l1 <= L;
}

struct rd_layer {
    int kind, flags, first, rows;
    int64_t src;                                                      // BITS: in 32-bit words; LEVELS: bytes; LABELS: elements
};

// The call's source buffers and table size, as every layer check needs them
struct rd_sources {
    const uint8_t* bits; int64_t bits_bytes;
    const uint8_t* levels; int64_t levels_bytes;
    const int32_t* labels; int64_t labels_n;
    int T;
};

// Row (kind | flags << 8, src, first, rows) of an image of (h, w) -> the layer, or false: skipped as if absent
RD_HD bool rd_layer_of(const int64_t* row, int h, int w, const rd_sources& s, rd_layer& q) {
    const int64_t kf = row[0], src = row[1], first = row[2], rows = row[3];
    if (kf < 0 || kf > 0xffff) return false;
    const int kind = (int)(kf & 0xff), flags = (int)(kf >> 8);
    if (src < 0 || first < 0 || rows < 0 || first > s.T || rows > s.T || first + rows > s.T) return false;
    const int64_t pixels = (int64_t)h * w;
    if (kind == RD_BITS) {
        if ((flags & ~RD_INVERT) != 0 || !s.bits || rows != 1 || (src & 3) != 0) return false;
        if (src > s.bits_bytes || (int64_t)4 * h * sz_words_per_row(w) > s.bits_bytes - src) return false;
        q.src = src >> 2;
    } else if (kind == RD_LEVELS) {
        if (flags != 0 || !s.levels || rows != 256) return false;
        if (src > s.levels_bytes || pixels > s.levels_bytes - src) return false;
        q.src = src;
    } else if (kind == RD_LABELS) {
        if ((flags & ~RD_EDGES) != 0 || !s.labels) return false;
        if (src > s.labels_n || pixels > s.labels_n - src) return false;
        q.src = src;
    } else {
        return false;
    }
    q.kind = kind; q.flags = flags; q.first = (int)first; q.rows = (int)rows;
    return true;
}

// Pixel (y, x), x < w, of the sized plane of ws words per row
RD_HD bool rd_bit(const uint32_t* plane, int ws, int y, int x) {
    return ((cc_unpack(plane[sz_word_of(y, x, ws)]) >> (x & 31)) & 1u) != 0;
}

// Pixel p = y w + x of the (h, w) map: some 4-neighbour inside the image holds another raw id
RD_HD bool rd_edge(const int32_t* map, int h, int w, int y, int x, int64_t p) {
    const int32_t id = map[p];
    if (x > 0 && map[p - 1] != id) return true;
    if (x < w - 1 && map[p + 1] != id) return true;
    if (y > 0 && map[p - w] != id) return true;
    return y < h - 1 && map[p + w] != id;
}
