// Boundaries of sized planes (include/cvlm.h: cvlm_mask_boundary_sized): X & ~erode(X, radius) with the outside of the
// plane read as clear -- boundary_iou_api's mask_to_boundary -- for planes of any mix of sizes, each at a radius of its own, at a cost
// that does not grow with the radius.  The per-thread logic -- the chunk of a row, the two run lengths of a pixel, the column count,
// the segment length -- is boundary_logic.h, shared with the sequential host entry at the end of this file.  All integers.
//
// Three launches: bd_init_kernel (out_area, status), then through the caller's workspace
//   bd_rows_kernel: a wave per row.  The lanes load 64 words at once; the wave walks their 32 chunks forwards with the carried run
//                   that ends before the chunk, keeps "the run ending here reaches d + 1" per word in LDS, walks them backwards with the
//                   run that starts behind the chunk and stores the AND of both, unpacked, into the workspace;
//   bd_cols_kernel: a wave per (64 pixel columns, segment of rows).  Lane i counts the consecutive surviving rows of column i; the
//                   lanes load 32 rows of the chunk's two words at once; one ballot of "count >= 2 d + 1" is the eroded row y - d, and
//                   X & ~ero goes out as whole words; popcounts are summed per workgroup into at most one atomic per plane.
// No workgroup waits for another; a refused plane is never read.
#include <algorithm>
#include <cstring>

#include "../../include/cvlm.h"
#include "common.h"
#include "boundary_logic.h"

namespace {

__global__ __launch_bounds__(256) void bd_init_kernel(int* __restrict__ out_area, int P, int* __restrict__ status) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p == 0) status[0] = 0;
    if (out_area && p < P) out_area[p] = 0;
}

// word `lane` of the wave's 64 words takes the half of the 64-bit result `a` of chunk k that belongs to it
__device__ __forceinline__ uint32_t bd_take(uint32_t acc, unsigned long long a, int k, int lane) {
    return lane == 2 * k ? (uint32_t)a : lane == 2 * k + 1 ? (uint32_t)(a >> 32) : acc;
}

// Plane blockIdx.y; wave v of workgroup g takes the rows 4 g + v, + 4 gridDim.x, ...  A row has at most 512 words: 8 loads of 64.
__global__ __launch_bounds__(256) void bd_rows_kernel(const uint8_t* __restrict__ bits, int64_t nbytes, const int64_t* __restrict__ offsets,
                                                      const int* __restrict__ dims, const int* __restrict__ radius,
                                                      uint8_t* __restrict__ workspace) {
    __shared__ uint32_t fwd[4][SZ_MAX_SIDE / 32];
    const int p = blockIdx.y;
    const int h = dims[2 * p], w = dims[2 * p + 1], d = radius[p];
    const int64_t off = offsets[p], end = offsets[p + 1];
    if (!sz_plane_ok(h, w, off, end, nbytes) || !bd_radius_ok(d)) return;            // the same for every thread of the plane
    if (blockIdx.x * 4 >= h) return;
    const int ws = sz_words_per_row(w), chunks = (ws + 1) >> 1, nblk = (chunks + 31) >> 5;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t* src = (const uint32_t*)(bits + off);
    uint32_t* dst = (uint32_t*)(workspace + off);
    for (int y = blockIdx.x * 4 + wave; y < h; y += gridDim.x * 4) {
        const uint32_t* row = src + (int64_t)y * ws;
        uint32_t* orow = dst + (int64_t)y * ws;
        int carry = 0;
        for (int b = 0; b < nblk; ++b) {
            const int c = 64 * b + lane;
            const uint32_t v = c < ws ? cc_unpack(row[c]) : 0u;
            const int nch = min(32, chunks - 32 * b);
            uint32_t acc = 0u;
            for (int k = 0; k < nch; ++k) {
                const uint64_t m = bd_chunk(__shfl(v, 2 * k, 64), __shfl(v, 2 * k + 1, 64), 64 * (32 * b + k), w);
                acc = bd_take(acc, __ballot(bd_run_reaches(bd_run_end(m, lane, carry), d)), k, lane);
                carry = bd_run_end(m, 63, carry);
            }
            fwd[wave][c] = acc;                                       // c <= 511; read back by this lane alone
        }
        carry = 0;
        for (int b = nblk - 1; b >= 0; --b) {
            const int c = 64 * b + lane;
            const uint32_t v = c < ws ? cc_unpack(row[c]) : 0u;
            const int nch = min(32, chunks - 32 * b);
            uint32_t acc = 0u;
            for (int k = nch - 1; k >= 0; --k) {
                const uint64_t m = bd_chunk(__shfl(v, 2 * k, 64), __shfl(v, 2 * k + 1, 64), 64 * (32 * b + k), w);
                acc = bd_take(acc, __ballot(bd_run_reaches(bd_run_start(m, lane, carry), d)), k, lane);
                carry = bd_run_start(m, 0, carry);
            }
            if (c < ws) orow[c] = acc & fwd[wave][c];
        }
    }
}

// Plane blockIdx.y.  A UNIT is (segment s, chunk column): upr = ceil(ws / 2) chunk columns times ceil(h / seg) segments; wave v of
// workgroup g takes the units 4 g + v, + 4 gridDim.x, ... -- neighbouring waves read neighbouring words of the same rows.  Lane l loads
// word (l & 1) of row (l >> 1) of a block of 32 rows.
template <bool AREA>
__global__ __launch_bounds__(256) void bd_cols_kernel(const uint8_t* __restrict__ bits, int64_t nbytes, const int64_t* __restrict__ offsets,
                                                      const int* __restrict__ dims, const int* __restrict__ radius,
                                                      const uint8_t* __restrict__ workspace, uint8_t* __restrict__ out_bits,
                                                      int* __restrict__ out_area, int* __restrict__ status) {
    const int p = blockIdx.y;
    const int h = dims[2 * p], w = dims[2 * p + 1], d = radius[p];
    const int64_t off = offsets[p], end = offsets[p + 1];
    if (!sz_plane_ok(h, w, off, end, nbytes) || !bd_radius_ok(d)) {                  // the same for every thread of the plane
        if (bd_slice_ok(off, end, nbytes)) {
            uint32_t* z = (uint32_t*)(out_bits + off);
            const int64_t n = (end - off) >> 2;
            for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) z[i] = 0u;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, 1);
        return;
    }
    const int ws = sz_words_per_row(w), upr = (ws + 1) >> 1;
    const int seg = bd_seg_rows(d), nseg = (h + seg - 1) / seg;
    const int units = upr * nseg;                                     // <= 256 * 128
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane >> 1, odd = lane & 1;
    const uint32_t* src = (const uint32_t*)(bits + off);
    const uint32_t* hero = (const uint32_t*)(workspace + off);
    uint32_t* dst = (uint32_t*)(out_bits + off);
    int cnt = 0;                                                      // the same in every lane of the wave
    for (int u = blockIdx.x * 4 + wave; u < units; u += gridDim.x * 4) {
        const int s = u / upr, c = 2 * (u - s * upr);
        const int r0 = s * seg, r1 = min(h, r0 + seg), x0 = 32 * c;
        const bool mine = c + odd < ws;
        int count = 0;
        const int y1 = min(h, r0 + d);
        for (int yb = max(0, r0 - d); yb < y1; yb += 32) {            // the warm-up: counts only
            const int y = yb + sub;
            const uint32_t hv = mine && y < y1 ? hero[(int64_t)y * ws + c + odd] : 0u;
            const int n = min(32, y1 - yb);
            for (int j = 0; j < n; ++j) {
                const uint64_t m = bd_chunk(__shfl(hv, 2 * j, 64), __shfl(hv, 2 * j + 1, 64), x0, w);
                count = bd_count(count, (m >> lane) & 1);
            }
        }
        for (int rb = r0; rb < r1; rb += 32) {
            const int r = rb + sub;
            const uint32_t xv = mine && r < r1 ? cc_unpack(src[(int64_t)r * ws + c + odd]) : 0u;
            const uint32_t hv = mine && r + d < h ? hero[(int64_t)(r + d) * ws + c + odd] : 0u;
            const int n = min(32, r1 - rb);
            uint32_t acc = 0u;
            for (int j = 0; j < n; ++j) {
                unsigned long long ero = 0ull;
                if (rb + j + d < h) {                                 // a row nearer than d to the last one is never eroded
                    const uint64_t m = bd_chunk(__shfl(hv, 2 * j, 64), __shfl(hv, 2 * j + 1, 64), x0, w);
                    count = bd_count(count, (m >> lane) & 1);
                    ero = __ballot(bd_col_erodes(count, d));
                }
                const uint64_t o = bd_chunk(__shfl(xv, 2 * j, 64), __shfl(xv, 2 * j + 1, 64), x0, w) & ~ero;
                acc = bd_take(acc, o, j, lane);
                cnt += __builtin_popcountll(o);
            }
            if (mine && r < r1) dst[(int64_t)r * ws + c + odd] = cc_pack(acc);
        }
    }
    if (AREA) {
        int v[1] = {lane == 0 ? cnt : 0};
        if (mb_block_sum(v) && v[0]) atomicAdd(&out_area[p], v[0]);
    }
}

// what both entries refuse
bool bd_bad(const uint8_t* bits, int64_t nbytes, const int64_t* offsets, const int32_t* dims, const int32_t* radius, int32_t P,
            int64_t max_words, const void* workspace, const uint8_t* out_bits, const int32_t* out_area, const int32_t* status) {
    if (!bits || !offsets || !dims || !radius || !workspace || !out_bits || !status) return true;
    if (mb_misaligned(4, bits, dims, radius, workspace, out_bits, out_area, status) || mb_misaligned(8, offsets)) return true;
    if (P < 1 || P > 65535 || nbytes < 4 || max_words < 1 || max_words > (int64_t)SZ_MAX_SIDE * (SZ_MAX_SIDE / 32)) return true;
    const uint64_t n = (uint64_t)nbytes;
    return mb_ranges_meet(out_bits, n, bits, n) || mb_ranges_meet(workspace, n, bits, n) || mb_ranges_meet(workspace, n, out_bits, n);
}

}  // namespace

extern "C" {

int cvlm_mask_boundary_sized(const uint8_t* bits, int64_t n_bytes, const int64_t* offsets, const int32_t* dims, const int32_t* radius,
                             int32_t P, int64_t max_words, void* workspace, uint8_t* out_bits, int32_t* out_area, int32_t* status,
                             void* stream) {
    if (bd_bad(bits, n_bytes, offsets, dims, radius, P, max_words, workspace, out_bits, out_area, status)) return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    // workgroups per plane: about 4096 in all and at most 256, and no more than the largest plane has work for (its rows, and its
    // column units, are fewer than its words); the waves walk what is left in strides
    const int64_t by_work = (max_words + 3) / 4;
    const int64_t want = (4096 + P - 1) / P;
    const int gx = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(by_work, want), 256));
    hipLaunchKernelGGL(bd_init_kernel, dim3((P + 255) / 256), dim3(256), 0, st, (int*)out_area, (int)P, (int*)status);
    CVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(bd_rows_kernel, dim3(gx, P), dim3(256), 0, st, bits, n_bytes, offsets, (const int*)dims, (const int*)radius,
                       (uint8_t*)workspace);
    CVLM_CHECK_LAUNCH();
    if (out_area)
        hipLaunchKernelGGL(bd_cols_kernel<true>, dim3(gx, P), dim3(256), 0, st, bits, n_bytes, offsets, (const int*)dims, (const int*)radius,
                           (const uint8_t*)workspace, out_bits, (int*)out_area, (int*)status);
    else
        hipLaunchKernelGGL(bd_cols_kernel<false>, dim3(gx, P), dim3(256), 0, st, bits, n_bytes, offsets, (const int*)dims,
                           (const int*)radius, (const uint8_t*)workspace, out_bits, (int*)nullptr, (int*)status);
    CVLM_CHECK_LAUNCH();
    return 0;
}

// The same functions on host memory: plane by plane, the row pass chunk by chunk and pixel by pixel into the workspace, the column
// pass unit by unit with the kernel's segments and warm-up
int cvlm_debug_mask_boundary_sized_host(const uint8_t* bits, int64_t n_bytes, const int64_t* offsets, const int32_t* dims,
                                        const int32_t* radius, int32_t P, int64_t max_words, void* workspace, uint8_t* out_bits,
                                        int32_t* out_area, int32_t* status) {
    if (bd_bad(bits, n_bytes, offsets, dims, radius, P, max_words, workspace, out_bits, out_area, status)) return CVLM_E_BADARG;
    status[0] = 0;
    for (int p = 0; p < P; ++p) {
        if (out_area) out_area[p] = 0;
        const int h = dims[2 * p], w = dims[2 * p + 1], d = radius[p];
        const int64_t off = offsets[p], end = offsets[p + 1];
        if (!sz_plane_ok(h, w, off, end, n_bytes) || !bd_radius_ok(d)) {
            if (bd_slice_ok(off, end, n_bytes)) memset(out_bits + off, 0, (size_t)(end - off));
            status[0] |= 1;
            continue;
        }
        const int ws = sz_words_per_row(w), chunks = (ws + 1) >> 1;
        const uint32_t* src = (const uint32_t*)(bits + off);
        uint32_t* hero = (uint32_t*)((uint8_t*)workspace + off);
        uint32_t* dst = (uint32_t*)(out_bits + off);
        auto chunk_of = [&](const uint32_t* row, int k, bool stored) {
            const uint32_t lo = row[2 * k], hi = 2 * k + 1 < ws ? row[2 * k + 1] : 0u;
            return bd_chunk(stored ? cc_unpack(lo) : lo, stored ? cc_unpack(hi) : hi, 64 * k, w);
        };
        auto put = [&](uint32_t* row, int k, uint64_t a) {
            row[2 * k] = (uint32_t)a;
            if (2 * k + 1 < ws) row[2 * k + 1] = (uint32_t)(a >> 32);
        };
        for (int y = 0; y < h; ++y) {
            const uint32_t* row = src + (int64_t)y * ws;
            uint32_t* orow = hero + (int64_t)y * ws;
            int carry = 0;
            for (int k = 0; k < chunks; ++k) {
                const uint64_t m = chunk_of(row, k, true);
                uint64_t a = 0;
                for (int i = 0; i < 64; ++i) a |= (uint64_t)bd_run_reaches(bd_run_end(m, i, carry), d) << i;
                carry = bd_run_end(m, 63, carry);
                put(orow, k, a);
            }
            carry = 0;
            for (int k = chunks - 1; k >= 0; --k) {
                const uint64_t m = chunk_of(row, k, true);
                uint64_t a = 0;
                for (int i = 0; i < 64; ++i) a |= (uint64_t)bd_run_reaches(bd_run_start(m, i, carry), d) << i;
                carry = bd_run_start(m, 0, carry);
                put(orow, k, a & chunk_of(orow, k, false));
            }
        }
        const int seg = bd_seg_rows(d), nseg = (h + seg - 1) / seg;
        int64_t cnt = 0;
        for (int s = 0; s < nseg; ++s) {
            const int r0 = s * seg, r1 = std::min(h, r0 + seg);
            for (int k = 0; k < chunks; ++k) {
                int count[64] = {};
                for (int y = std::max(0, r0 - d); y < std::min(h, r0 + d); ++y) {
                    const uint64_t m = chunk_of(hero + (int64_t)y * ws, k, false);
                    for (int i = 0; i < 64; ++i) count[i] = bd_count(count[i], (m >> i) & 1);
                }
                for (int r = r0; r < r1; ++r) {
                    uint64_t ero = 0;
                    if (r + d < h) {
                        const uint64_t m = chunk_of(hero + (int64_t)(r + d) * ws, k, false);
                        for (int i = 0; i < 64; ++i) {
                            count[i] = bd_count(count[i], (m >> i) & 1);
                            ero |= (uint64_t)bd_col_erodes(count[i], d) << i;
                        }
                    }
                    const uint64_t o = chunk_of(src + (int64_t)r * ws, k, true) & ~ero;
                    uint32_t* orow = dst + (int64_t)r * ws;
                    orow[2 * k] = cc_pack((uint32_t)o);
                    if (2 * k + 1 < ws) orow[2 * k + 1] = cc_pack((uint32_t)(o >> 32));
                    cnt += __builtin_popcountll(o);
                }
            }
        }
        if (out_area) out_area[p] = (int32_t)cnt;
    }
    return 0;
}

}  // extern "C"
