// Rendering on the device (include/cvlm.h: cvlm_render): overlays, outlines and label colour maps painted over interleaved
// 3-channel uint8 images of any mix of sizes -- demo.py's save_array_as_image without its text, and the visualizer's draw_binary_mask /
// draw_soft_mask / draw_sem_seg / draw_panoptic_seg without matplotlib's anti-aliasing.  One streaming pass of two launches.
//
// rd_init_kernel    status = 0.
// rd_render_kernel  workgroups (x, b) walk image b.  A RUN is 16 consecutive pixels of the FLAT image, 48 bytes = 3 x 16, and belongs to one
//                   lane: it loads them as three 16-byte vectors once, keeps them in twelve registers across every layer of the image and
//                   stores them once -- 48 bytes in flight per lane is what hides the memory latency (DESIGN.md §31 measured 12).  w is
//                   free, so a run may straddle a row end: (y, x) comes from the flat pixel index, one division per run.  A BITS layer
//                   costs one word per lane where the run sits in one row and one word, two where it crosses a word end inside its row,
//                   a word per pixel across a row end; its table row is read once per run and layer.  Pixels are blended four at a time:
//                   twelve bytes branch-free (byte -> float, a product, a sum, round, a saturating pack), merged under the byte mask of the
//                   selected ones; a wave without a selected pixel in a group of four skips it.  Layer descriptors depend on blockIdx and
//                   the layer counter alone: scalar loads and scalar checks.  The last run of an image whose pixel count is no multiple
//                   of 16 is loaded and stored byte by byte, so the pad bytes behind an image are never written.  The grid is sized by the
//                   largest image of the call; a workgroup whose first run lies beyond its image leaves at once.
// A lane reads and writes the bytes of its own run alone and no thread waits for another: out == img is the same pass.  The per-pixel
// logic is render_logic.h, shared with the sequential host entry at the end of this file.
#include <string.h>

#include <algorithm>

#include "../../include/cvlm.h"
#include "common.h"
#include "render_logic.h"

namespace {

constexpr int RD_THREADS = 256;
constexpr int RD_QUAD = 4;                                            // pixels blended together: 12 bytes, 3 dwords
constexpr int RD_QUADS = 4;                                           // of a run
constexpr int RD_RUN = RD_QUAD * RD_QUADS;                            // pixels of a run: 48 bytes
constexpr int RD_GRID_Y = 65535;                                      // images of one launch

typedef uint32_t rd_u32x4 __attribute__((ext_vector_type(4), aligned(4)));    // an image starts on a 4-byte boundary, no more
typedef int32_t rd_i32x4 __attribute__((ext_vector_type(4), aligned(4)));     // four ids of a label map
typedef uint32_t rd_u32x4_any __attribute__((ext_vector_type(4), aligned(1))); // sixteen levels: a levels map starts at any byte

__global__ void rd_init_kernel(int* __restrict__ status) {
    if (threadIdx.x == 0) status[0] = 0;
}

// byte i (0 .. 11) of a quad blended with (b, q) into `to`
__device__ __forceinline__ void rd_mix_byte(const uint32_t (&px)[3], uint32_t (&to)[3], int i, float b, float q) {
    const uint8_t c = (uint8_t)(px[i >> 2] >> (8 * (i & 3)));
    to[i >> 2] = __builtin_amdgcn_cvt_pk_u8_f32(rd_mix(c, b, q), i & 3, to[i >> 2]);      // saturates as rd_blend's clamp does
}
// pixel k of the quad blended with table row `row`: false if the row's alpha paints nothing
__device__ __forceinline__ bool rd_paint(uint32_t (&px)[3], int k, const uint8_t* __restrict__ rgb, const float* __restrict__ alpha, int64_t row) {
    const float a = alpha[row];
    if (!rd_alpha_ok(a)) return false;
    const float b = rd_rest(a);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) rd_mix_byte(px, px, 3 * k + ch, b, rd_weigh(rgb[3 * row + ch], a));
    return true;
}
// the bytes of a quad that belong to the pixels of `sel` (bit k = pixel k)
__device__ __forceinline__ void rd_byte_masks(unsigned sel, uint32_t (&m)[3]) {
    m[0] = ((sel & 1u) ? 0x00ffffffu : 0u) | ((sel & 2u) ? 0xff000000u : 0u);
    m[1] = ((sel & 2u) ? 0x0000ffffu : 0u) | ((sel & 4u) ? 0xffff0000u : 0u);
    m[2] = ((sel & 4u) ? 0x000000ffu : 0u) | ((sel & 8u) ? 0xffffff00u : 0u);
}

// img and out may be the same buffer: neither is __restrict__
__global__ __launch_bounds__(RD_THREADS) void rd_render_kernel(const uint8_t* img, int64_t img_bytes, const int64_t* __restrict__ img_off,
                                                               const int* __restrict__ dims, int b0, const int* __restrict__ layer_off,
                                                               const int64_t* __restrict__ layers, int L, rd_sources s,
                                                               const uint8_t* __restrict__ rgb, const float* __restrict__ alpha, uint8_t* out,
                                                               int* __restrict__ status) {
    const int b = b0 + blockIdx.y;
    const int h = dims[2 * b], w = dims[2 * b + 1];
    const int64_t off = img_off[b], end = img_off[b + 1];
    const int l0 = layer_off[b], l1 = layer_off[b + 1];
    const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
    if (!rd_image_ok(h, w, off, end, img_bytes, l0, l1, L)) {         // the same for every thread of the image: nothing is read or stored
        if (lead) atomicOr(status, RD_IMAGE_REFUSED);
        return;
    }
    const int n = h * w;                                              // <= 2^28
    const int runs = (n + RD_RUN - 1) / RD_RUN;
    if (blockIdx.x * RD_THREADS >= runs) return;
    if (lead) {
        bool skipped = false;
        for (int l = l0; l < l1; ++l) {
            rd_layer q;
            skipped |= !rd_layer_of(layers + 4 * (int64_t)l, h, w, s, q);
        }
        if (skipped) atomicOr(status, RD_LAYER_SKIPPED);
    }
    if (img == out && l0 == l1) return;                               // in place and no layer: the bytes are there
    const int ws = sz_words_per_row(w);
    bool bad_row = false;
    for (int r = blockIdx.x * RD_THREADS + threadIdx.x; r < runs; r += gridDim.x * RD_THREADS) {
        const int p0 = RD_RUN * r;
        const int np = n - p0 < RD_RUN ? n - p0 : RD_RUN;             // pixels of this run: 16 but for an image's last
        const int64_t at = off + 3 * (int64_t)p0;                     // a multiple of 4
        uint32_t px[RD_QUADS][3];
        uint32_t* flat = &px[0][0];
        if (np == RD_RUN) {
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const rd_u32x4 t = *(const rd_u32x4*)(img + at + 16 * v);
#pragma unroll
                for (int i = 0; i < 4; ++i) flat[4 * v + i] = t[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 3 * RD_QUADS; ++i) flat[i] = 0u;
            for (int i = 0; i < 3 * np; ++i) {
                const uint32_t byte = (uint32_t)img[at + i] << (8 * (i & 3));
#pragma unroll
                for (int d = 0; d < 3 * RD_QUADS; ++d) flat[d] |= (i >> 2) == d ? byte : 0u;       // no dynamic index: the run stays in registers
            }
        }
        const int y0 = p0 / w, x0 = p0 - y0 * w;
        for (int l = l0; l < l1; ++l) {
            rd_layer q;
            if (!rd_layer_of(layers + 4 * (int64_t)l, h, w, s, q)) continue;       // the same for every thread of the image
            if (q.kind == RD_BITS) {
                const uint32_t* plane = (const uint32_t*)s.bits + q.src;
                unsigned sel = 0;
                if (np == RD_RUN && x0 + RD_RUN - 1 < w) {            // one row: one word, or two across a word end
                    const int sh = x0 & 31;
                    const int64_t word = sz_word_of(y0, x0, ws);
                    sel = cc_unpack(plane[word]) >> sh;
                    if (sh > 32 - RD_RUN) sel |= cc_unpack(plane[word + 1]) << (32 - sh);      // x0 + 15 lies in the next word of the row
                    sel &= 0xffffu;
                } else {
                    int y = y0, x = x0;
                    for (int k = 0; k < np; ++k) {
                        sel |= (rd_bit(plane, ws, y, x) ? 1u : 0u) << k;
                        if (++x == w) { x = 0; ++y; }
                    }
                }
                if (q.flags & RD_INVERT) sel = ~sel & ((1u << np) - 1u);
                if (sel) {
                    const float a = alpha[q.first];
                    if (!rd_alpha_ok(a)) {
                        bad_row = true;
                    } else {
                        const float rest = rd_rest(a);
                        float part[3];
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) part[ch] = rd_weigh(rgb[3 * (int64_t)q.first + ch], a);
#pragma unroll
                        for (int g = 0; g < RD_QUADS; ++g) {
                            const unsigned four = (sel >> (RD_QUAD * g)) & 0xfu;
                            if (!four) continue;
                            uint32_t to[3] = {0u, 0u, 0u}, m[3];
#pragma unroll
                            for (int i = 0; i < 3 * RD_QUAD; ++i) rd_mix_byte(px[g], to, i, rest, part[i % 3]);
                            rd_byte_masks(four, m);
#pragma unroll
                            for (int i = 0; i < 3; ++i) px[g][i] = (px[g][i] & ~m[i]) | (to[i] & m[i]);
                        }
                    }
                }
            } else if (q.kind == RD_LEVELS) {
                const uint8_t* map = s.levels + q.src + p0;
                if (np == RD_RUN) {                                   // the sixteen levels as one vector, whatever the map's alignment
                    const rd_u32x4_any lv = *(const rd_u32x4_any*)map;
#pragma unroll
                    for (int g = 0; g < RD_QUADS; ++g)
#pragma unroll
                        for (int k = 0; k < RD_QUAD; ++k) bad_row |= !rd_paint(px[g], k, rgb, alpha, (int64_t)q.first + ((lv[g] >> (8 * k)) & 0xffu));
                } else {
#pragma unroll
                    for (int g = 0; g < RD_QUADS; ++g)
#pragma unroll
                        for (int k = 0; k < RD_QUAD; ++k)
                            if (RD_QUAD * g + k < np) bad_row |= !rd_paint(px[g], k, rgb, alpha, (int64_t)q.first + map[RD_QUAD * g + k]);
                }
            } else {
                const int32_t* map = s.labels + q.src;
                const bool edges = (q.flags & RD_EDGES) != 0;
                if (np == RD_RUN && x0 + RD_RUN - 1 < w) {
                    // One row: a quad's ids, and for EDGES the four above and the four below, as 16-byte vectors; the id left of the
                    // quad and the one right of it as single loads.  A neighbour outside the image is not read: it counts as equal.
                    const bool up = edges && y0 > 0, down = edges && y0 < h - 1;
#pragma unroll
                    for (int g = 0; g < RD_QUADS; ++g) {
                        const int p = p0 + RD_QUAD * g, x = x0 + RD_QUAD * g;
                        const rd_i32x4 id = *(const rd_i32x4*)(map + p);
                        rd_i32x4 above = id, below = id;
                        int32_t left = id[0], right = id[RD_QUAD - 1];
                        if (up) above = *(const rd_i32x4*)(map + p - w);
                        if (down) below = *(const rd_i32x4*)(map + p + w);
                        if (edges && x > 0) left = map[p - 1];
                        if (edges && x + RD_QUAD < w) right = map[p + RD_QUAD];
#pragma unroll
                        for (int k = 0; k < RD_QUAD; ++k) {
                            const int32_t me = id[k];
                            const int32_t lf = k == 0 ? left : id[k > 0 ? k - 1 : 0], rt = k == RD_QUAD - 1 ? right : id[k < RD_QUAD - 1 ? k + 1 : k];
                            const bool edge = lf != me || rt != me || above[k] != me || below[k] != me;
                            if (me >= 0 && me < q.rows && (!edges || edge)) bad_row |= !rd_paint(px[g], k, rgb, alpha, (int64_t)q.first + me);
                        }
                    }
                } else {
                    int y = y0, x = x0;
                    for (int k = 0; k < np; ++k) {
                        const int p = p0 + k;
                        const int32_t id = map[p];
                        if (id >= 0 && id < q.rows && (!edges || rd_edge(map, h, w, y, x, p))) {
#pragma unroll
                            for (int g = 0; g < RD_QUADS; ++g)        // no dynamic index: the run stays in registers
                                if (k / RD_QUAD == g) {
#pragma unroll
                                    for (int kk = 0; kk < RD_QUAD; ++kk)
                                        if (k % RD_QUAD == kk) bad_row |= !rd_paint(px[g], kk, rgb, alpha, (int64_t)q.first + id);
                                }
                        }
                        if (++x == w) { x = 0; ++y; }
                    }
                }
            }
        }
        if (np == RD_RUN) {
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                rd_u32x4 t;
#pragma unroll
                for (int i = 0; i < 4; ++i) t[i] = flat[4 * v + i];
                *(rd_u32x4*)(out + at + 16 * v) = t;
            }
        } else {
            for (int i = 0; i < 3 * np; ++i) {
                uint32_t word = 0u;
#pragma unroll
                for (int d = 0; d < 3 * RD_QUADS; ++d) word |= (i >> 2) == d ? flat[d] : 0u;
                out[at + i] = (uint8_t)(word >> (8 * (i & 3)));
            }
        }
    }
    if (bad_row) atomicOr(status, RD_ROW_REFUSED);
}

// what both entries refuse
bool rd_bad(const uint8_t* img, int64_t img_bytes, const int64_t* img_offsets, const int32_t* dims, int32_t B, int64_t max_pixels,
            const int32_t* layer_offsets, const int64_t* layers, int32_t L, const uint8_t* bits, int64_t bits_bytes, const uint8_t* levels,
            int64_t levels_bytes, const int32_t* labels, int64_t labels_n, const uint8_t* rgb, const float* alpha, int32_t T,
            const uint8_t* out, const int32_t* status) {
    if (!img || !img_offsets || !dims || !layer_offsets || !rgb || !alpha || !out || !status) return true;
    if (B < 1 || B > RD_MAX_B || L < 0 || L > RD_MAX_L || T < 1 || T > RD_MAX_T || (L > 0 && !layers)) return true;
    if (img_bytes < 4 || bits_bytes < 0 || levels_bytes < 0 || labels_n < 0 || labels_n > ((int64_t)1 << 60)) return true;
    if (max_pixels < 1 || max_pixels > (int64_t)SZ_MAX_SIDE * SZ_MAX_SIDE) return true;
    if (mb_misaligned(4, img, out, dims, layer_offsets, bits, labels, alpha, status) || mb_misaligned(8, img_offsets, layers)) return true;
    const uint64_t nb = (uint64_t)B, nt = (uint64_t)T;
    const struct { const void* p; uint64_t bytes; } in[] = {
        {img, (uint64_t)img_bytes}, {img_offsets, 8 * (nb + 1)}, {dims, 8 * nb}, {layer_offsets, 4 * (nb + 1)}, {layers, 32 * (uint64_t)L},
        {bits, (uint64_t)bits_bytes}, {levels, (uint64_t)levels_bytes}, {labels, 4 * (uint64_t)labels_n}, {rgb, 3 * nt}, {alpha, 4 * nt}};
    for (size_t i = 0; i < sizeof(in) / sizeof(in[0]); ++i) {
        if (mb_ranges_meet(status, 4, in[i].p, in[i].bytes)) return true;
        if (i == 0 && out == img) continue;                           // in place: exactly the image buffer
        if (mb_ranges_meet(out, (uint64_t)img_bytes, in[i].p, in[i].bytes)) return true;
    }
    return mb_ranges_meet(status, 4, out, (uint64_t)img_bytes);
}

}  // namespace

extern "C" {

int cvlm_render(const uint8_t* img, int64_t img_bytes, const int64_t* img_offsets, const int32_t* dims, int32_t B, int64_t max_pixels,
                const int32_t* layer_offsets, const int64_t* layers, int32_t L, const uint8_t* bits, int64_t bits_bytes,
                const uint8_t* levels, int64_t levels_bytes, const int32_t* labels, int64_t labels_n, const uint8_t* rgb, const float* alpha,
                int32_t T, uint8_t* out, int32_t* status, void* stream) {
    if (rd_bad(img, img_bytes, img_offsets, dims, B, max_pixels, layer_offsets, layers, L, bits, bits_bytes, levels, levels_bytes, labels,
               labels_n, rgb, alpha, T, out, status))
        return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const rd_sources s = {bits, bits_bytes, levels, levels_bytes, labels, labels_n, (int)T};
    hipLaunchKernelGGL(rd_init_kernel, dim3(1), dim3(64), 0, st, (int*)status);
    CVLM_CHECK_LAUNCH();
    // workgroups per image: one per 256 runs of the largest image, 2^22 in a launch at most; larger images go in strides
    const int64_t by_work = ((max_pixels + RD_RUN - 1) / RD_RUN + RD_THREADS - 1) / RD_THREADS;
    for (int b0 = 0; b0 < B; b0 += RD_GRID_Y) {
        const int nb = std::min<int>(B - b0, RD_GRID_Y);
        const int gx = (int)std::max<int64_t>(1, std::min<int64_t>(by_work, std::max<int64_t>(1, ((int64_t)1 << 22) / nb)));
        hipLaunchKernelGGL(rd_render_kernel, dim3(gx, nb), dim3(RD_THREADS), 0, st, img, img_bytes, img_offsets, (const int*)dims, b0,
                           (const int*)layer_offsets, layers, (int)L, s, rgb, alpha, out, (int*)status);
        CVLM_CHECK_LAUNCH();
    }
    return 0;
}

// The same functions on host memory: image by image, layer by layer and pixel by pixel through render_logic.h
int cvlm_debug_render_host(const uint8_t* img, int64_t img_bytes, const int64_t* img_offsets, const int32_t* dims, int32_t B,
                           int64_t max_pixels, const int32_t* layer_offsets, const int64_t* layers, int32_t L, const uint8_t* bits,
                           int64_t bits_bytes, const uint8_t* levels, int64_t levels_bytes, const int32_t* labels, int64_t labels_n,
                           const uint8_t* rgb, const float* alpha, int32_t T, uint8_t* out, int32_t* status) {
    if (rd_bad(img, img_bytes, img_offsets, dims, B, max_pixels, layer_offsets, layers, L, bits, bits_bytes, levels, levels_bytes, labels,
               labels_n, rgb, alpha, T, out, status))
        return CVLM_E_BADARG;
    const rd_sources s = {bits, bits_bytes, levels, levels_bytes, labels, labels_n, (int)T};
    status[0] = 0;
    for (int b = 0; b < B; ++b) {
        const int h = dims[2 * b], w = dims[2 * b + 1];
        const int64_t off = img_offsets[b];
        const int l0 = layer_offsets[b], l1 = layer_offsets[b + 1];
        if (!rd_image_ok(h, w, off, img_offsets[b + 1], img_bytes, l0, l1, L)) { status[0] |= RD_IMAGE_REFUSED; continue; }
        uint8_t* px = out + off;
        if (out != img) memcpy(px, img + off, (size_t)rd_image_bytes(h, w));
        const int ws = sz_words_per_row(w);
        auto paint = [&](int64_t p, int64_t row) {
            const float a = alpha[row];
            if (!rd_alpha_ok(a)) { status[0] |= RD_ROW_REFUSED; return; }
            for (int ch = 0; ch < 3; ++ch) px[3 * p + ch] = rd_blend(px[3 * p + ch], rgb[3 * row + ch], a);
        };
        for (int l = l0; l < l1; ++l) {
            rd_layer q;
            if (!rd_layer_of(layers + 4 * (int64_t)l, h, w, s, q)) { status[0] |= RD_LAYER_SKIPPED; continue; }
            for (int y = 0; y < h; ++y) {
                for (int x = 0; x < w; ++x) {
                    const int64_t p = (int64_t)y * w + x;
                    if (q.kind == RD_BITS) {
                        const bool on = rd_bit((const uint32_t*)bits + q.src, ws, y, x);
                        if (on != ((q.flags & RD_INVERT) != 0)) paint(p, q.first);
                    } else if (q.kind == RD_LEVELS) {
                        paint(p, (int64_t)q.first + levels[q.src + p]);
                    } else {
                        const int32_t* map = labels + q.src;
                        const int32_t id = map[p];
                        if (id >= 0 && id < q.rows && (!(q.flags & RD_EDGES) || rd_edge(map, h, w, y, x, p))) paint(p, (int64_t)q.first + id);
                    }
                }
            }
        }
    }
    return 0;
}

}  // extern "C"
