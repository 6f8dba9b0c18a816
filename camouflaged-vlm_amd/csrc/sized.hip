// Packed masks at each image's own size (include/cvlm.h: cvlm_mask_pack_sized): full-resolution logit planes -> the bits
// of `cvlm_mask_to_u8(...) >= level` at a size of the plane's own, in one launch over planes of any mix of sizes.  The per-thread logic
// -- the axis table of an output coordinate, the blend, the compare, the place of a pixel in its word -- is sized_logic.h, shared with
// the sequential host entry at the end of this file.  All results but the blend are integers; no thread waits for another workgroup.
#include <algorithm>

#include "../../include/cvlm.h"
#include "common.h"
#include "sized_logic.h"

namespace {

// status = 0; area = 0, box = -1
__global__ __launch_bounds__(256) void sized_init_kernel(int* __restrict__ area, int* __restrict__ box, int P, int* __restrict__ status) {
    mb_init_planes(status, area, box, P);
}

// Plane blockIdx.y.  A UNIT is 64 consecutive pixels of one output row -- two words; a row has ceil(ws / 2) of them.  Wave v of
// workgroup g takes the units 4 g + v, + 4 gridDim.x, ...: each lane forms its pixel (lanes at x >= w read nothing and give 0), one
// ballot holds both words in "bit i = pixel i" form, bit reversal + byte swap turn each half into packbits' order, lanes 0 and 32
// store them.  A workgroup whose first unit lies beyond its plane leaves at once: the grid is sized by the largest plane of the call.
template <bool STATS>
__global__ __launch_bounds__(256) void sized_pack_kernel(const float* __restrict__ logits, int Hs, int Ws, const int* __restrict__ dims,
                                                         const int64_t* __restrict__ offsets, int level, uint8_t* __restrict__ bits,
                                                         int64_t nbytes, int* __restrict__ area, int* __restrict__ box,
                                                         int* __restrict__ status) {
    const int p = blockIdx.y;
    const int h = dims[2 * p], w = dims[2 * p + 1];
    const int64_t off = offsets[p], end = offsets[p + 1];
    if (!sz_plane_ok(h, w, off, end, nbytes)) {                       // the same for every thread of the plane: nothing is read or stored
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, 1);
        return;
    }
    const int ws = sz_words_per_row(w), upr = (ws + 1) >> 1;          // h, w <= 16384: h * upr < 2^23
    const int units = h * upr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x * 4 >= units) return;                              // the whole workgroup: no barrier has been passed
    const float* src = logits + (int64_t)p * Hs * Ws;
    uint32_t* dst = (uint32_t*)(bits + off);
    const double sx = (double)Ws / (double)w, sy = (double)Hs / (double)h;
    mb_stats stats;
    for (int u = blockIdx.x * 4 + wave; u < units; u += gridDim.x * 4) {
        const int y = u / upr, c = 2 * (u - y * upr);                 // c: the first of the unit's two words
        const int x = 32 * c + lane;
        bool on = false;
        if (x < w) on = sz_pixel(src, Ws, sz_axis_of(x, Ws, sx, true), sz_axis_of(y, Hs, sy, false), level);
        const unsigned long long both = __ballot(on);
        const uint32_t mine = lane < 32 ? (uint32_t)both : (uint32_t)(both >> 32);
        if ((lane & 31) == 0 && c + (lane >> 5) < ws) dst[sz_word_of(y, x, ws)] = cc_pack(mine);
        if (STATS && on) mb_pixel(stats, x, y);
    }
    if (STATS) mb_block_commit(stats, area, box, p);
}

// what both entries refuse
bool sized_bad(const float* logits, int32_t P, int32_t Hs, int32_t Ws, const int32_t* dims, const int64_t* offsets, int32_t level,
               const uint8_t* bits, int64_t nbytes, int64_t max_words, const int32_t* area, const int32_t* box, const int32_t* status) {
    if (!logits || !dims || !offsets || !bits || !status || (area == nullptr) != (box == nullptr)) return true;
    if (mb_misaligned(4, logits, bits, dims, area, box, status) || mb_misaligned(8, offsets)) return true;
    if (P < 1 || P > 65535 || Hs <= 0 || Ws <= 0 || (int64_t)Hs * Ws >= ((int64_t)1 << 31) || level < 1 || level > 255) return true;
    return nbytes < 4 || max_words < 1 || max_words > (int64_t)SZ_MAX_SIDE * (SZ_MAX_SIDE / 32);
}

}  // namespace

extern "C" {

int cvlm_mask_pack_sized(const float* logits, int32_t P, int32_t Hs, int32_t Ws, const int32_t* dims, const int64_t* offsets,
                         int32_t level, uint8_t* bits, int64_t bits_bytes, int64_t max_words, int32_t* area, int32_t* box,
                         int32_t* status, void* stream) {
    if (sized_bad(logits, P, Hs, Ws, dims, offsets, level, bits, bits_bytes, max_words, area, box, status)) return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    // workgroups per plane: one per four units of the largest plane, about 4096 in all and at most 256 -- every workgroup that finds a
    // set pixel ends in five atomics on its plane's results; the waves walk what is left in strides
    const int64_t by_work = ((max_words + 1) / 2 + 3) / 4;
    const int64_t want = (4096 + P - 1) / P;
    const int gx = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(by_work, want), 256));
    hipLaunchKernelGGL(sized_init_kernel, dim3((P + 255) / 256), dim3(256), 0, st, (int*)area, (int*)box, (int)P, (int*)status);
    CVLM_CHECK_LAUNCH();
    if (area)
        hipLaunchKernelGGL(sized_pack_kernel<true>, dim3(gx, P), dim3(256), 0, st, logits, (int)Hs, (int)Ws, (const int*)dims, offsets,
                           (int)level, bits, bits_bytes, (int*)area, (int*)box, (int*)status);
    else
        hipLaunchKernelGGL(sized_pack_kernel<false>, dim3(gx, P), dim3(256), 0, st, logits, (int)Hs, (int)Ws, (const int*)dims, offsets,
                           (int)level, bits, bits_bytes, (int*)nullptr, (int*)nullptr, (int*)status);
    CVLM_CHECK_LAUNCH();
    return 0;
}

// The same functions on host memory, plane by plane and pixel by pixel, through sized_logic.h
int cvlm_debug_mask_pack_sized_host(const float* logits, int32_t P, int32_t Hs, int32_t Ws, const int32_t* dims, const int64_t* offsets,
                                    int32_t level, uint8_t* bits, int64_t bits_bytes, int64_t max_words, int32_t* area, int32_t* box,
                                    int32_t* status) {
    if (sized_bad(logits, P, Hs, Ws, dims, offsets, level, bits, bits_bytes, max_words, area, box, status)) return CVLM_E_BADARG;
    status[0] = 0;
    for (int p = 0; p < P; ++p) {
        if (area) mb_init(area, box, p);
        const int h = dims[2 * p], w = dims[2 * p + 1];
        const int64_t off = offsets[p], end = offsets[p + 1];
        if (!sz_plane_ok(h, w, off, end, bits_bytes)) { status[0] |= 1; continue; }
        const int ws = sz_words_per_row(w);
        const float* src = logits + (int64_t)p * Hs * Ws;
        uint32_t* dst = (uint32_t*)(bits + off);
        const double sx = (double)Ws / (double)w, sy = (double)Hs / (double)h;
        mb_stats stats;
        for (int y = 0; y < h; ++y) {
            const sz_axis ay = sz_axis_of(y, Hs, sy, false);
            for (int c = 0; c < ws; ++c) {
                uint32_t word = 0u;
                for (int x = 32 * c; x < std::min(w, 32 * c + 32); ++x) {
                    if (!sz_pixel(src, Ws, sz_axis_of(x, Ws, sx, true), ay, level)) continue;
                    word |= sz_bit_of(x);
                    mb_pixel(stats, x, y);
                }
                dst[sz_word_of(y, 32 * c, ws)] = cc_pack(word);
            }
        }
        if (area) mb_store(stats, area, box, p);
    }
    return 0;
}

}  // extern "C"
