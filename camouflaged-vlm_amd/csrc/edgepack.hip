// Packed edge maps (include/cvlm.h: cvlm_edge_pack): the edge head's low-resolution probability planes resized,
// thresholded and packed in one kernel, with the popcount of each packed plane and of its AND with a second packed plane (the mask's
// edge band).  The full-resolution f32 plane of the reference (models/sam_maskdecoder_edge.py:298-302) is never written.  The
// per-pixel logic -- coordinate, blend, compare -- is edgepack_logic.h, shared with the sequential host entry at the end of this file.
// One launch after the init launch, no workspace.  All results are bits and integer sums.
#include "../../include/cvlm.h"
#include "common.h"
#include "edgepack_logic.h"

namespace {

__global__ __launch_bounds__(256) void ep_init_kernel(int* __restrict__ area, int* __restrict__ with_inter, int P) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    area[p] = 0;
    if (with_inter) with_inter[p] = 0;
}

// The rows oy0 + wave, + 4, .. <= oy_last of a tile, one row per wave and round: lane l holds the pixels ox .. ox + 3 of the row, whose
// taps xa / xb / lx it computed once.  `p` is the plane (stride = win, xs = ys = 0) or the staged footprint (stride = its columns,
// xa / xb already relative to its first column, ys its first row); y0 / y1 / ly are wave-uniform.  Lanes 8g .. 8g + 7 hold the 32
// pixels of one word: each places its nibble at bit 4 * (lane & 7), three xor-shuffles OR the eight nibbles, lane 8g stores the word
// in packbits' order (mask_pack_kernel's step).  Every lane runs every round -- the trip count is wave-uniform, columns beyond the
// row's end compute on the last column's taps -- so the shuffles always see their whole group.
__device__ __forceinline__ void ep_rows(const float* __restrict__ p, int stride, int ys, const int (&xa)[4], const int (&xb)[4],
                                        const float (&lx)[4], float sy, int hin, float threshold, int oy0, int oy_last, bool col_in,
                                        int word_col, int wpr, uint32_t* __restrict__ dst, const uint32_t* __restrict__ with,
                                        int& n_set, int& n_with) {
    const int lane = threadIdx.x & 63;
    for (int oy = oy0 + (threadIdx.x >> 6); oy <= oy_last; oy += 4) {
        const ep_tap ty = ep_coord(sy, oy, hin);
        const float* r0 = p + (ty.i0 - ys) * stride;                 // < hin * win < 2^31
        const float* r1 = p + (ty.i1 - ys) * stride;
        uint32_t nib = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            nib |= ep_above(ep_value(r0[xa[j]], r0[xb[j]], r1[xa[j]], r1[xb[j]], lx[j], ty.l), threshold) << j;
        uint32_t word = nib << (4 * (lane & 7));
        word |= __shfl_xor(word, 1, 64);
        word |= __shfl_xor(word, 2, 64);
        word |= __shfl_xor(word, 4, 64);
        if (col_in && (lane & 7) == 0) {
            const int64_t at = (int64_t)oy * wpr + word_col;
            const uint32_t stored = cc_pack(word);
            dst[at] = stored;
            n_set += __popc(word);
            if (with) n_with += __popc(stored & with[at]);
        }
    }
}

// Tile blockIdx.x = (row tile) * col_tiles + (column tile) of plane blockIdx.y.  STAGE: the tile's source footprint -- the rows and
// columns its taps read, a rectangle because the coordinate is monotone -- is copied to LDS once, row by row with consecutive lanes on
// consecutive floats, and the blend reads it from there; a tile whose footprint is larger than the buffer (ep_fits_lds bounds it, so
// none should be) reads the plane directly, as every tile of the other instance does.
template <bool STAGE>
__global__ __launch_bounds__(256) void ep_pack_kernel(const float* __restrict__ prob, int hin, int win, int hout, int wout, float sy, float sx,
                                                      float threshold, int col_tiles, uint32_t* __restrict__ bits, int* __restrict__ area,
                                                      const uint32_t* __restrict__ with_bits, int* __restrict__ with_inter) {
    __shared__ float s_src[STAGE ? EP_LDS_FLOATS : 1];
    const int tr = blockIdx.x / col_tiles, tc = blockIdx.x - tr * col_tiles;
    const int ox0 = tc * EP_TW, oy0 = tr * EP_TH;
    const int ox_last = min(ox0 + EP_TW, wout) - 1, oy_last = min(oy0 + EP_TH, hout) - 1;
    const int wpr = wout >> 5;
    const float* src = prob + (int64_t)blockIdx.y * hin * win;       // 64-bit: P planes pass 2^31 floats and 2^31 bytes of bits
    const int64_t plane = (int64_t)blockIdx.y * hout * wpr;          // in words
    const int ox = ox0 + 4 * (threadIdx.x & 63);
    const bool col_in = ox <= ox_last;                                // wout % 32 == 0: a word's eight lanes are inside together

    int xa[4], xb[4];
    float lx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const ep_tap t = ep_coord(sx, min(ox + j, ox_last), win);
        xa[j] = t.i0; xb[j] = t.i1; lx[j] = t.l;
    }

    int n_set = 0, n_with = 0;
    bool staged = false;
    if (STAGE) {
        int xs, xe, ys, ye;
        ep_footprint(sx, ox0, ox_last, win, xs, xe);
        ep_footprint(sy, oy0, oy_last, hin, ys, ye);
        const int cols = xe - xs + 1, rows = ye - ys + 1;
        staged = (int64_t)cols * rows <= EP_LDS_FLOATS;               // workgroup-uniform
        if (staged) {
            const int n = cols * rows;
            for (int i = threadIdx.x; i < n; i += 256) {
                const int r = i / cols, c = i - r * cols;
                s_src[i] = src[(ys + r) * win + xs + c];
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j) { xa[j] -= xs; xb[j] -= xs; }
            ep_rows(s_src, cols, ys, xa, xb, lx, sy, hin, threshold, oy0, oy_last, col_in, ox >> 5, wpr, bits + plane,
                    with_bits ? with_bits + plane : nullptr, n_set, n_with);
        }
    }
    if (!staged)
        ep_rows(src, win, 0, xa, xb, lx, sy, hin, threshold, oy0, oy_last, col_in, ox >> 5, wpr, bits + plane,
                with_bits ? with_bits + plane : nullptr, n_set, n_with);

    int n[2] = {n_set, n_with};
    if (mb_block_sum(n)) {
        if (n[0]) atomicAdd(&area[blockIdx.y], n[0]);                 // a workgroup that set nothing leaves the plane's sums alone
        if (with_inter && n[1]) atomicAdd(&with_inter[blockIdx.y], n[1]);
    }
}

// what both entries refuse
bool ep_bad_request(const float* prob, int32_t P, int32_t hin, int32_t win, int32_t hout, int32_t wout, float threshold, const uint8_t* bits,
                    const int32_t* area, const uint8_t* with_bits, const int32_t* with_inter) {
    if (!prob || !bits || !area || mb_misaligned(4, bits, with_bits) || mb_bad_planes(P, hout, wout)) return true;
    if (hin <= 0 || win <= 0 || (int64_t)hin * win >= ((int64_t)1 << 31)) return true;
    if (!(threshold > 0.0f && threshold < 1.0f)) return true;         // NaN and the infinities fail both comparisons
    if ((with_bits != nullptr) != (with_inter != nullptr)) return true;
    const uint64_t in_bytes = (uint64_t)P * ((uint64_t)hin * win * 4), plane_bytes = (uint64_t)P * ((uint64_t)hout * wout / 8);
    const uint64_t sum_bytes = (uint64_t)P * 4;
    const void* outs[3] = {bits, area, with_inter};
    const uint64_t out_bytes[3] = {plane_bytes, sum_bytes, sum_bytes};
    for (int i = 0; i < 3; ++i) {
        if (mb_ranges_meet(outs[i], out_bytes[i], prob, in_bytes) || mb_ranges_meet(outs[i], out_bytes[i], with_bits, plane_bytes)) return true;
        for (int k = i + 1; k < 3; ++k)
            if (mb_ranges_meet(outs[i], out_bytes[i], outs[k], out_bytes[k])) return true;
    }
    return false;
}

}  // namespace

extern "C" {

int cvlm_edge_pack(const float* prob, int32_t P, int32_t hin, int32_t win, int32_t hout, int32_t wout, float threshold, uint8_t* bits,
                   int32_t* area, const uint8_t* with_bits, int32_t* with_inter, void* stream) {
    if (ep_bad_request(prob, P, hin, win, hout, wout, threshold, bits, area, with_bits, with_inter)) return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const float sy = (float)hin / (float)hout, sx = (float)win / (float)wout;   // divided here: the device's division never enters
    const int col_tiles = (wout + EP_TW - 1) / EP_TW, row_tiles = (hout + EP_TH - 1) / EP_TH;   // hout * wout < 2^31: the grid fits
    hipLaunchKernelGGL(ep_init_kernel, dim3((P + 255) / 256), dim3(256), 0, st, (int*)area, (int*)with_inter, (int)P);
    CVLM_CHECK_LAUNCH();
    if (ep_fits_lds(hin, win, hout, wout))
        hipLaunchKernelGGL(ep_pack_kernel<true>, dim3(col_tiles * row_tiles, P), dim3(256), 0, st, prob, (int)hin, (int)win, (int)hout, (int)wout,
                           sy, sx, threshold, col_tiles, (uint32_t*)bits, (int*)area, (const uint32_t*)with_bits, (int*)with_inter);
    else
        hipLaunchKernelGGL(ep_pack_kernel<false>, dim3(col_tiles * row_tiles, P), dim3(256), 0, st, prob, (int)hin, (int)win, (int)hout, (int)wout,
                           sy, sx, threshold, col_tiles, (uint32_t*)bits, (int*)area, (const uint32_t*)with_bits, (int*)with_inter);
    CVLM_CHECK_LAUNCH();
    return 0;
}

// The same pixels on host memory, plane by plane and word by word, through the functions of edgepack_logic.h.
int cvlm_debug_edge_pack_host(const float* prob, int32_t P, int32_t hin, int32_t win, int32_t hout, int32_t wout, float threshold,
                              uint8_t* bits, int32_t* area, const uint8_t* with_bits, int32_t* with_inter) {
    if (ep_bad_request(prob, P, hin, win, hout, wout, threshold, bits, area, with_bits, with_inter)) return CVLM_E_BADARG;
    const float sy = (float)hin / (float)hout, sx = (float)win / (float)wout;
    const int wpr = wout / 32;
    uint32_t* dst = (uint32_t*)bits;
    const uint32_t* with = (const uint32_t*)with_bits;
    for (int p = 0; p < P; ++p) {
        const float* src = prob + (int64_t)p * hin * win;
        const int64_t plane = (int64_t)p * hout * wpr;
        int n_set = 0, n_with = 0;
        for (int oy = 0; oy < hout; ++oy) {
            const ep_tap ty = ep_coord(sy, oy, hin);
            const float* r0 = src + (int64_t)ty.i0 * win;
            const float* r1 = src + (int64_t)ty.i1 * win;
            for (int c = 0; c < wpr; ++c) {
                uint32_t word = 0;
                for (int b = 0; b < 32; ++b) {
                    const ep_tap tx = ep_coord(sx, 32 * c + b, win);
                    word |= ep_above(ep_value(r0[tx.i0], r0[tx.i1], r1[tx.i0], r1[tx.i1], tx.l, ty.l), threshold) << b;
                }
                const int64_t at = plane + (int64_t)oy * wpr + c;
                const uint32_t stored = cc_pack(word);
                dst[at] = stored;
                n_set += __builtin_popcount(word);
                if (with) n_with += __builtin_popcount(stored & with[at]);
            }
        }
        area[p] = n_set;
        if (with_inter) with_inter[p] = n_with;
    }
    return 0;
}

// Which instance cvlm_edge_pack launches for these sizes: 1 the staged one, 0 the direct one, CVLM_E_BADARG for sizes it refuses.
int cvlm_debug_edge_pack_staged(int32_t hin, int32_t win, int32_t hout, int32_t wout) {
    if (hin <= 0 || win <= 0 || hout <= 0 || wout <= 0 || wout % 32 != 0 || (int64_t)hout * wout >= ((int64_t)1 << 31) ||
        (int64_t)hin * win >= ((int64_t)1 << 31))
        return CVLM_E_BADARG;
    return ep_fits_lds(hin, win, hout, wout) ? 1 : 0;
}

}  // extern "C"
