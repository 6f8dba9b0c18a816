// Morphology of packed masks (include/cvlm.h: cvlm_mask_morph): dilation and erosion by the (2r + 1)^2 square and the
// edge band dil & ~ero, on the words cvlm_mask_pack writes.  The per-thread logic -- the horizontal pass of a word by doubling shifts,
// the clipped vertical pass of a word column -- is morph_logic.h, shared with the sequential host entry at the end of this file.
// One launch after the init launch, no workspace: a workgroup stages the horizontal results of its tile and of r halo rows above and
// below in LDS and runs the vertical pass from there.  All results are bits and integer sums.
#include <algorithm>
#include <vector>

#include "../../include/cvlm.h"
#include "common.h"
#include "morph_logic.h"

namespace {

// The tile of one workgroup: MO_TW word columns x MO_TH rows.  MO_TH = 128 keeps the rows read twice at r = 16 to (128 + 32) / 128 =
// 1.25 x; MO_TW = 16 divides W / 32 = 32 and 48 and wastes 6 of 16 lanes at W / 32 = 10.  LDS rows are MO_TW words apart and a wave's
// lanes sit on consecutive words of four consecutive rows: 64 consecutive words, one per bank, in the staging writes and in every
// read of the vertical pass.
constexpr int MO_TW = 16, MO_TH = 128, MO_ROWS = MO_TH + 2 * MO_MAXR;

__global__ __launch_bounds__(256) void mo_init_kernel(int* __restrict__ dil_area, int* __restrict__ ero_area, int* __restrict__ band_area, int P) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    if (dil_area) dil_area[p] = 0;
    if (ero_area) ero_area[p] = 0;
    if (band_area) band_area[p] = 0;
}

// Tile blockIdx.x = (row tile) * col_tiles + (column tile) of plane blockIdx.y.  VEC: the plane's rows are 16-byte aligned (bits is,
// and wpr % 4 == 0), a lane stages four words from one 16-byte load and takes the words next to its quad from the neighbouring lanes;
// otherwise one word per lane by element loads.  Rows outside the plane are neither staged nor read: the vertical window is clipped.
template <bool VEC>
__global__ __launch_bounds__(256) void mo_morph_kernel(const uint32_t* __restrict__ bits, int H, int wpr, int r, int col_tiles,
                                                       uint32_t* __restrict__ dil_bits, int* __restrict__ dil_area,
                                                       uint32_t* __restrict__ ero_bits, int* __restrict__ ero_area,
                                                       uint32_t* __restrict__ band_bits, int* __restrict__ band_area) {
    __shared__ __attribute__((aligned(16))) uint32_t s_hd[MO_ROWS * MO_TW];
    __shared__ __attribute__((aligned(16))) uint32_t s_he[MO_ROWS * MO_TW];
    const int tr = blockIdx.x / col_tiles, tc = blockIdx.x - tr * col_tiles;
    const int64_t plane = (int64_t)blockIdx.y * H * wpr;             // in words; 64-bit: P * H * W / 32 passes 2^31 words at large P
    const uint32_t* src = bits + plane;
    const int c0 = tc * MO_TW, y0 = tr * MO_TH;
    const int ya = max(0, y0 - r), yb = min(H, y0 + MO_TH + r);      // the plane's rows this tile needs: [ya, yb); LDS row = y - y0 + r

    if (VEC) {
        const int q = threadIdx.x & 3;                                // quad of the tile row: words c0 + 4q .. + 3
        for (int yy = ya; yy < yb; yy += 64) {                        // every lane runs every round: the shuffles see the whole wave
            const int y = yy + (threadIdx.x >> 2);
            const bool in = y < yb && c0 + 4 * q < wpr;               // wpr % 4 == 0: a quad is inside the row or beyond it
            const uint32_t* row = src + (int64_t)(in ? y : ya) * wpr;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (in) {
                v = *(const uint4*)(row + c0 + 4 * q);
                v.x = cc_unpack(v.x); v.y = cc_unpack(v.y); v.z = cc_unpack(v.z); v.w = cc_unpack(v.w);
            }
            uint32_t left = __shfl_up(v.w, 1, 64), right = __shfl_down(v.x, 1, 64);   // a quad beyond the row holds zeros
            if (q == 0) left = in ? mo_fetch(row, c0 - 1, wpr) : 0u;
            if (q == 3) right = in ? mo_fetch(row, c0 + MO_TW, wpr) : 0u;
            if (in) {
                const bool hl = c0 + 4 * q > 0, hr = c0 + 4 * q + 4 < wpr;
                const int at = (y - y0 + r) * MO_TW + 4 * q;
                *(uint4*)(s_hd + at) = make_uint4(mo_hdilate(left, v.x, v.y, r), mo_hdilate(v.x, v.y, v.z, r), mo_hdilate(v.y, v.z, v.w, r),
                                                  mo_hdilate(v.z, v.w, right, r));
                *(uint4*)(s_he + at) = make_uint4(mo_herode(left, v.x, v.y, hl, true, r), mo_herode(v.x, v.y, v.z, true, true, r),
                                                  mo_herode(v.y, v.z, v.w, true, true, r), mo_herode(v.z, v.w, right, true, hr, r));
            }
        }
    } else {
        const int c = c0 + (threadIdx.x & 15);
        for (int y = ya + (threadIdx.x >> 4); y < yb; y += 16) {
            if (c >= wpr) break;
            const uint32_t* row = src + (int64_t)y * wpr;
            const uint32_t left = mo_fetch(row, c - 1, wpr), centre = mo_fetch(row, c, wpr), right = mo_fetch(row, c + 1, wpr);
            const int at = (y - y0 + r) * MO_TW + (threadIdx.x & 15);
            s_hd[at] = mo_hdilate(left, centre, right, r);
            s_he[at] = mo_herode(left, centre, right, c > 0, c + 1 < wpr, r);
        }
    }
    __syncthreads();

    const int cl = threadIdx.x & 15, c = c0 + cl;
    int n[3] = {0, 0, 0};                                             // set pixels of the dilation, the erosion, the band
    if (c < wpr) {
        for (int y = y0 + (threadIdx.x >> 4); y < min(H, y0 + MO_TH); y += 16) {
            const int lo = max(0, y - r), hi = min(H - 1, y + r);     // inside [ya, yb)
            const int at = (lo - y0 + r) * MO_TW + cl;
            uint32_t d, e;
            mo_column(s_hd + at, s_he + at, MO_TW, hi - lo + 1, d, e);
            const uint32_t b = d & ~e;
            const int64_t out = plane + (int64_t)y * wpr + c;
            if (dil_bits) dil_bits[out] = cc_pack(d);
            if (ero_bits) ero_bits[out] = cc_pack(e);
            if (band_bits) band_bits[out] = cc_pack(b);
            n[0] += __popc(d); n[1] += __popc(e); n[2] += __popc(b);
        }
    }
    if (mb_block_sum(n)) {
        if (dil_area && n[0]) atomicAdd(&dil_area[blockIdx.y], n[0]);
        if (ero_area && n[1]) atomicAdd(&ero_area[blockIdx.y], n[1]);
        if (band_area && n[2]) atomicAdd(&band_area[blockIdx.y], n[2]);
    }
}

// what both entries refuse
bool mo_bad_request(const uint32_t* bits, int32_t P, int32_t H, int32_t W, int32_t radius, const uint32_t* dil_bits, const int32_t* dil_area,
                    const uint32_t* ero_bits, const int32_t* ero_area, const uint32_t* band_bits, const int32_t* band_area) {
    if (!bits || mb_misaligned(4, bits, dil_bits, ero_bits, band_bits) || mb_bad_planes(P, H, W)) return true;
    if (radius < 1 || radius > MO_MAXR) return true;
    if ((dil_bits != nullptr) != (dil_area != nullptr) || (ero_bits != nullptr) != (ero_area != nullptr) ||
        (band_bits != nullptr) != (band_area != nullptr))
        return true;
    if (!dil_bits && !ero_bits && !band_bits) return true;
    const uint64_t bytes = (uint64_t)P * ((uint64_t)H * W / 8);       // the kernel reads halo rows: no output may lie on the input
    return mb_ranges_meet(bits, bytes, dil_bits, bytes) || mb_ranges_meet(bits, bytes, ero_bits, bytes) ||
           mb_ranges_meet(bits, bytes, band_bits, bytes) || mb_ranges_meet(dil_bits, bytes, ero_bits, bytes) ||
           mb_ranges_meet(dil_bits, bytes, band_bits, bytes) || mb_ranges_meet(ero_bits, bytes, band_bits, bytes);
}

}  // namespace

extern "C" {

int cvlm_mask_morph(const uint32_t* bits, int32_t P, int32_t H, int32_t W, int32_t radius, uint32_t* dil_bits, int32_t* dil_area,
                    uint32_t* ero_bits, int32_t* ero_area, uint32_t* band_bits, int32_t* band_area, void* stream) {
    if (mo_bad_request(bits, P, H, W, radius, dil_bits, dil_area, ero_bits, ero_area, band_bits, band_area)) return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int wpr = W / 32, col_tiles = (wpr + MO_TW - 1) / MO_TW, row_tiles = (H + MO_TH - 1) / MO_TH;   // H * wpr < 2^26: the grid fits
    const bool vec = (((uintptr_t)bits) & 15) == 0 && wpr % 4 == 0;
    hipLaunchKernelGGL(mo_init_kernel, dim3((P + 255) / 256), dim3(256), 0, st, (int*)dil_area, (int*)ero_area, (int*)band_area, (int)P);
    CVLM_CHECK_LAUNCH();
    if (vec)
        hipLaunchKernelGGL(mo_morph_kernel<true>, dim3(col_tiles * row_tiles, P), dim3(256), 0, st, bits, (int)H, wpr, (int)radius, col_tiles,
                           dil_bits, (int*)dil_area, ero_bits, (int*)ero_area, band_bits, (int*)band_area);
    else
        hipLaunchKernelGGL(mo_morph_kernel<false>, dim3(col_tiles * row_tiles, P), dim3(256), 0, st, bits, (int)H, wpr, (int)radius, col_tiles,
                           dil_bits, (int*)dil_area, ero_bits, (int*)ero_area, band_bits, (int*)band_area);
    CVLM_CHECK_LAUNCH();
    return 0;
}

// The same two passes on host memory, plane by plane and word by word, through the functions of morph_logic.h.
int cvlm_debug_mask_morph_host(const uint32_t* bits, int32_t P, int32_t H, int32_t W, int32_t radius, uint32_t* dil_bits, int32_t* dil_area,
                               uint32_t* ero_bits, int32_t* ero_area, uint32_t* band_bits, int32_t* band_area) {
    if (mo_bad_request(bits, P, H, W, radius, dil_bits, dil_area, ero_bits, ero_area, band_bits, band_area)) return CVLM_E_BADARG;
    const int wpr = W / 32, r = radius;
    const int64_t words = (int64_t)H * wpr;
    std::vector<uint32_t> hd((size_t)words), he((size_t)words);
    for (int p = 0; p < P; ++p) {
        const uint32_t* src = bits + (int64_t)p * words;
        for (int y = 0; y < H; ++y) {
            const uint32_t* row = src + (int64_t)y * wpr;
            for (int c = 0; c < wpr; ++c) {
                const uint32_t left = mo_fetch(row, c - 1, wpr), centre = mo_fetch(row, c, wpr), right = mo_fetch(row, c + 1, wpr);
                hd[(size_t)y * wpr + c] = mo_hdilate(left, centre, right, r);
                he[(size_t)y * wpr + c] = mo_herode(left, centre, right, c > 0, c + 1 < wpr, r);
            }
        }
        int n_dil = 0, n_ero = 0, n_band = 0;
        for (int y = 0; y < H; ++y) {
            const int lo = std::max(0, y - r), hi = std::min(H - 1, y + r);
            for (int c = 0; c < wpr; ++c) {
                uint32_t d, e;
                mo_column(hd.data() + (size_t)lo * wpr + c, he.data() + (size_t)lo * wpr + c, wpr, hi - lo + 1, d, e);
                const uint32_t b = d & ~e;
                const int64_t out = (int64_t)p * words + (int64_t)y * wpr + c;
                if (dil_bits) dil_bits[out] = cc_pack(d);
                if (ero_bits) ero_bits[out] = cc_pack(e);
                if (band_bits) band_bits[out] = cc_pack(b);
                n_dil += __builtin_popcount(d); n_ero += __builtin_popcount(e); n_band += __builtin_popcount(b);
            }
        }
        if (dil_area) dil_area[p] = n_dil;
        if (ero_area) ero_area[p] = n_ero;
        if (band_area) band_area[p] = n_band;
    }
    return 0;
}

}  // extern "C"
