// Run-length encoding of packed masks (include/cvlm.h: cvlm_mask_rle_count / cvlm_mask_rle_emit): COCO's column-major
// alternating run counts of the planes cvlm_mask_pack writes.  The per-thread logic -- the transition word, the transposing gather,
// the place of a column block in the stream, the counts of a stream word -- is rle_logic.h, shared with the sequential host entry at
// the end of this file.  Counting is one launch after its init launch and takes no workspace.  Emitting is three launches per round
// of planes: transpose the transition bits into the stream, scan the stream (one workgroup per plane), emit one stream word per
// thread.  All results are integers; no thread waits for another workgroup.
#include <algorithm>
#include <vector>

#include "../../include/cvlm.h"
#include "common.h"
#include "rle_logic.h"

namespace {

// The tile of one workgroup of the transpose: RL_TW word columns x RL_TH rows, 8 KiB of transition words in LDS.  A wave stages 16
// consecutive words of four consecutive rows; in the gather its lanes are the 32 pixel columns of two word columns and read two LDS
// words per step, each broadcast to 32 lanes.
constexpr int RL_TW = 16, RL_TH = 128;
constexpr int RL_COUNT_WORDS = 2048;                                  // words of a plane per workgroup of the count kernel
constexpr int RL_SCAN = 1024;                                         // threads of the scan's one workgroup per plane

// Workspace of one plane of HW pixels: the stream (HW / 32 words), then per stream word the transitions before it and the position
// of the last of them: 12 bytes per 32 pixels, rounded up to 16 bytes.
int64_t rl_plane_ws_bytes(int64_t HW) { return (HW / 32 * 12 + 15) / 16 * 16; }

__global__ __launch_bounds__(256) void rl_init_kernel(int* __restrict__ n_runs, int P, int* __restrict__ status) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (n_runs && p < P) n_runs[p] = 1;                              // the tail run
    if (status && p == 0) status[0] = 0;
}

// n_runs[blockIdx.y] += the transitions of RL_COUNT_WORDS words of the plane
__global__ __launch_bounds__(256) void rl_count_kernel(const uint32_t* __restrict__ bits, int H, int wpr, int Wt, int* __restrict__ n_runs) {
    const int words = H * wpr;                                        // < 2^26
    const uint32_t* src = bits + (int64_t)blockIdx.y * words;         // 64-bit: P * H * W / 32 passes 2^31 words at large P
    int n[1] = {0};
#pragma unroll
    for (int i = 0; i < RL_COUNT_WORDS / 256; ++i) {
        const int wi = blockIdx.x * RL_COUNT_WORDS + i * 256 + threadIdx.x;
        if (wi < words) {
            const int y = wi / wpr;
            n[0] += __popc(rl_transition(src, y, wi - y * wpr, H, wpr, Wt));
        }
    }
    if (mb_block_sum(n) && n[0]) atomicAdd(&n_runs[blockIdx.y], n[0]);
}

// Tile blockIdx.x = (row tile) * col_tiles + (column tile) of plane blockIdx.y of the round.  stream: the round's workspace, planes
// ws_stride words apart.  ALIGNED (H % 32 == 0): a column block is one whole stream word and is stored; otherwise it straddles two
// words that other blocks share, the launcher has zeroed the stream and the non-zero parts are ORed in -- integer atomics that
// commute, so the stream's bits do not depend on the schedule.  Pixel columns at or beyond the true width Wt are no part of the stream.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void rl_transpose_kernel(const uint32_t* __restrict__ bits, int H, int wpr, int Wt, int col_tiles,
                                                           uint32_t* __restrict__ stream, int64_t ws_stride) {
    __shared__ uint32_t s_t[RL_TH * RL_TW];
    const int tr = blockIdx.x / col_tiles, tc = blockIdx.x - tr * col_tiles;
    const uint32_t* src = bits + (int64_t)blockIdx.y * H * wpr;
    uint32_t* out = stream + (int64_t)blockIdx.y * ws_stride;
    const int c0 = tc * RL_TW, y0 = tr * RL_TH;
    const int rows = min(RL_TH, H - y0);                              // >= 1: the grid has no tile below the plane

    const int cl = threadIdx.x & 15, c = c0 + cl;
    if (c < wpr)
        for (int r = threadIdx.x >> 4; r < rows; r += 16) s_t[r * RL_TW + cl] = rl_transition(src, y0 + r, c, H, wpr, Wt);
    __syncthreads();

#pragma unroll 1
    for (int i = 0; i < RL_TH * RL_TW / 256; ++i) {                   // 32 pixel columns x 16 word columns x 4 row blocks
        const int o = i * 256 + threadIdx.x;
        const int bit = o & 31, ocl = (o >> 5) & 15, rb = o >> 9;
        const int n = min(32, rows - 32 * rb);
        if (32 * (c0 + ocl) + bit >= Wt || n <= 0) continue;
        const uint32_t v = rl_gather(s_t + 32 * rb * RL_TW + ocl, RL_TW, n, bit);
        int word;
        uint32_t lo, hi;
        rl_place(v, 32 * (c0 + ocl) + bit, y0 + 32 * rb, H, word, lo, hi);
        if (ALIGNED) {
            out[word] = lo;
        } else {
            if (lo) atomicOr(&out[word], lo);
            if (hi) atomicOr(&out[word + 1], hi);                     // hi != 0: the block's bits pass the word's end, word + 1 exists
        }
    }
}

// One workgroup per plane of the round: for every one of the stream's `words` words (HW = H * Wt bits, the last word may be partly
// filled) the transitions before it (rank) and the position of the last of them (prev), then the tail run, which ends at HW.  Sequential over slabs of RL_SCAN words with a carry; inside a slab a wave scan by shuffles and the
// waves' totals through LDS, double-buffered by the slab's parity: one barrier per slab.
__global__ __launch_bounds__(RL_SCAN) void rl_scan_kernel(uint32_t* __restrict__ ws, int64_t ws_stride, int words, int HW, int p0,
                                                          const int64_t* __restrict__ offsets, int32_t* __restrict__ counts, int64_t total,
                                                          int* __restrict__ status) {
    __shared__ int s_sum[2][RL_SCAN / 64], s_max[2][RL_SCAN / 64];
    uint32_t* stream = ws + (int64_t)blockIdx.x * ws_stride;
    int* rank = (int*)stream + words;
    int* prev = rank + words;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry_sum = 0, carry_max = 0;
    for (int k0 = 0, slab = 0; k0 < words; k0 += RL_SCAN, slab ^= 1) {
        const int k = k0 + threadIdx.x;
        const uint32_t w = k < words ? stream[k] : 0u;
        const int n = __popc(w), last = rl_last(w, k);
        int sum = n, mx = last;                                       // inclusive over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int a = __shfl_up(sum, o, 64), b = __shfl_up(mx, o, 64);
            if (lane >= o) { sum += a; mx = max(mx, b); }
        }
        if (lane == 63) { s_sum[slab][wave] = sum; s_max[slab][wave] = mx; }
        __syncthreads();
        int before_sum = carry_sum, before_max = carry_max, all_sum = carry_sum, all_max = carry_max;
#pragma unroll
        for (int v = 0; v < RL_SCAN / 64; ++v) {
            const int a = s_sum[slab][v], b = s_max[slab][v];
            if (v < wave) { before_sum += a; before_max = max(before_max, b); }
            all_sum += a; all_max = max(all_max, b);
        }
        int ex_max = __shfl_up(mx, 1, 64);                            // exclusive: the lanes below
        if (lane == 0) ex_max = 0;
        if (k < words) {
            rank[k] = before_sum + sum - n;
            prev[k] = max(before_max, ex_max);
        }
        carry_sum = all_sum;
        carry_max = all_max;
    }
    if (threadIdx.x == 0) {
        const int p = p0 + blockIdx.x;
        const int64_t off = offsets[p], end = offsets[p + 1];
        if (rl_emit_tail(HW, carry_sum, carry_max, counts, off, end - off, off >= 0 && end <= total)) atomicOr(status, 1);
    }
}

// One thread per stream word of plane blockIdx.y of the round
__global__ __launch_bounds__(256) void rl_emit_kernel(const uint32_t* __restrict__ ws, int64_t ws_stride, int words, int p0,
                                                      const int64_t* __restrict__ offsets, int32_t* __restrict__ counts, int64_t total,
                                                      int* __restrict__ status) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= words) return;
    const uint32_t* stream = ws + (int64_t)blockIdx.y * ws_stride;
    const uint32_t w = stream[k];
    if (!w) return;
    const int p = p0 + blockIdx.y;
    const int64_t off = offsets[p], end = offsets[p + 1];
    const int* rank = (const int*)stream + words;
    if (rl_emit_word(w, k, rank[k], rank[words + k], counts, off, end - off, off >= 0 && end <= total)) atomicOr(status, 1);
}

// what every entry refuses; Wt: the true width, the last word of a row holds at least one of its columns
bool rl_bad_planes(const uint32_t* bits, int32_t P, int32_t H, int32_t W, int32_t Wt) {
    if (!bits || mb_misaligned(4, bits) || mb_bad_planes(P, H, W)) return true;
    return Wt > W || Wt <= W - 32;
}

bool rl_bad_emit(const int64_t* offsets, const int32_t* counts, int64_t total, const int32_t* status) {
    if (!offsets || !counts || !status || total < 1) return true;
    return mb_misaligned(8, offsets) || mb_misaligned(4, counts, status);
}

int rl_count(const uint32_t* bits, int32_t P, int32_t H, int32_t W, int32_t Wt, int32_t* n_runs, void* stream) {
    if (rl_bad_planes(bits, P, H, W, Wt) || !n_runs || mb_misaligned(4, n_runs)) return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int wpr = W / 32, words = H * wpr;                          // < 2^26: the grid fits
    hipLaunchKernelGGL(rl_init_kernel, dim3((P + 255) / 256), dim3(256), 0, st, (int*)n_runs, (int)P, (int*)nullptr);
    CVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(rl_count_kernel, dim3((words + RL_COUNT_WORDS - 1) / RL_COUNT_WORDS, P), dim3(256), 0, st, bits, (int)H, wpr,
                       (int)Wt, (int*)n_runs);
    CVLM_CHECK_LAUNCH();
    return 0;
}

// The plane's words are H * W / 32 apart and sized the workspace; the stream has H * Wt bits.
int rl_emit(const uint32_t* bits, int32_t P, int32_t H, int32_t W, int32_t Wt, const int64_t* offsets, int32_t* counts, int64_t total,
            int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
    if (rl_bad_planes(bits, P, H, W, Wt) || rl_bad_emit(offsets, counts, total, status)) return CVLM_E_BADARG;
    const int64_t plane_bytes = rl_plane_ws_bytes((int64_t)H * W);
    if (mb_bad_workspace(workspace, workspace_bytes, plane_bytes)) return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int wpr = W / 32, words = H * wpr;
    const int HW = H * Wt, swords = (int)(((int64_t)HW + 31) / 32);   // the stream: swords <= words, equal when Wt = W
    const int col_tiles = (wpr + RL_TW - 1) / RL_TW, row_tiles = (H + RL_TH - 1) / RL_TH;   // words < 2^26: the grids fit
    const bool aligned = H % 32 == 0;
    const int fit = mb_fit(P, workspace_bytes, plane_bytes);
    const int64_t ws_stride = plane_bytes / 4;
    uint32_t* ws = (uint32_t*)workspace;
    hipLaunchKernelGGL(rl_init_kernel, dim3(1), dim3(256), 0, st, (int*)nullptr, 0, (int*)status);
    CVLM_CHECK_LAUNCH();
    for (int p0 = 0; p0 < P; p0 += fit) {
        const int n = std::min(fit, P - p0);
        const uint32_t* src = bits + (int64_t)p0 * words;
        if (aligned) {
            hipLaunchKernelGGL(rl_transpose_kernel<true>, dim3(col_tiles * row_tiles, n), dim3(256), 0, st, src, (int)H, wpr, (int)Wt,
                               col_tiles, ws, ws_stride);
        } else {
            const hipError_t e = hipMemsetAsync(ws, 0, (size_t)n * plane_bytes, st);
            if (e != hipSuccess) return (int)e;
            hipLaunchKernelGGL(rl_transpose_kernel<false>, dim3(col_tiles * row_tiles, n), dim3(256), 0, st, src, (int)H, wpr, (int)Wt,
                               col_tiles, ws, ws_stride);
        }
        CVLM_CHECK_LAUNCH();
        hipLaunchKernelGGL(rl_scan_kernel, dim3(n), dim3(RL_SCAN), 0, st, ws, ws_stride, swords, HW, p0, offsets, counts, total,
                           (int*)status);
        CVLM_CHECK_LAUNCH();
        hipLaunchKernelGGL(rl_emit_kernel, dim3((swords + 255) / 256, n), dim3(256), 0, st, (const uint32_t*)ws, ws_stride, swords, p0,
                           offsets, counts, total, (int*)status);
        CVLM_CHECK_LAUNCH();
    }
    return 0;
}

// The same functions on host memory, plane by plane and word by word, through rle_logic.h.  counts == NULL: only n_runs.
int rl_host(const uint32_t* bits, int32_t P, int32_t H, int32_t W, int32_t Wt, int32_t* n_runs, const int64_t* offsets, int32_t* counts,
            int64_t total, int32_t* status) {
    if (rl_bad_planes(bits, P, H, W, Wt) || !n_runs || mb_misaligned(4, n_runs)) return CVLM_E_BADARG;
    if (counts && rl_bad_emit(offsets, counts, total, status)) return CVLM_E_BADARG;
    const int wpr = W / 32, words = H * wpr;
    const int HW = H * Wt, swords = (int)(((int64_t)HW + 31) / 32);
    std::vector<uint32_t> t((size_t)words), stream((size_t)swords);
    if (counts) status[0] = 0;
    for (int p = 0; p < P; ++p) {
        const uint32_t* src = bits + (int64_t)p * words;
        int n = 0;
        for (int y = 0; y < H; ++y)
            for (int c = 0; c < wpr; ++c) {
                t[(size_t)y * wpr + c] = rl_transition(src, y, c, H, wpr, Wt);
                n += __builtin_popcount(t[(size_t)y * wpr + c]);
            }
        n_runs[p] = 1 + n;
        if (!counts) continue;
        std::fill(stream.begin(), stream.end(), 0u);
        for (int x = 0; x < Wt; ++x)
            for (int y = 0; y < H; y += 32) {
                const uint32_t v = rl_gather(t.data() + (size_t)y * wpr + (x >> 5), wpr, std::min(32, H - y), x & 31);
                int word;
                uint32_t lo, hi;
                rl_place(v, x, y, H, word, lo, hi);
                stream[(size_t)word] |= lo;
                if (hi) stream[(size_t)word + 1] |= hi;
            }
        const int64_t off = offsets[p], end = offsets[p + 1];
        const bool ok = off >= 0 && end <= total;
        int rank = 0, prev = 0;
        for (int k = 0; k < swords; ++k) {
            const uint32_t w = stream[(size_t)k];
            if (!w) continue;
            status[0] |= rl_emit_word(w, k, rank, prev, counts, off, end - off, ok);
            rank += __builtin_popcount(w);
            prev = rl_last(w, k);
        }
        status[0] |= rl_emit_tail(HW, rank, prev, counts, off, end - off, ok);
    }
    return 0;
}

}  // namespace

extern "C" {

int64_t cvlm_mask_rle_workspace_bytes(int32_t P, int32_t H, int32_t W) {
    if (mb_bad_planes(P, H, W)) return CVLM_E_BADARG;
    return (int64_t)P * rl_plane_ws_bytes((int64_t)H * W);
}

// The planes of cvlm_mask_pack: every column of every word is the image's, Wt = W
int cvlm_mask_rle_count(const uint32_t* bits, int32_t P, int32_t H, int32_t W, int32_t* n_runs, void* stream) {
    return rl_count(bits, P, H, W, W, n_runs, stream);
}

int cvlm_mask_rle_emit(const uint32_t* bits, int32_t P, int32_t H, int32_t W, const int64_t* offsets, int32_t* counts, int64_t total,
                       int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
    return rl_emit(bits, P, H, W, W, offsets, counts, total, status, workspace, workspace_bytes, stream);
}

int cvlm_debug_mask_rle_host(const uint32_t* bits, int32_t P, int32_t H, int32_t W, int32_t* n_runs, const int64_t* offsets,
                             int32_t* counts, int64_t total, int32_t* status) {
    return rl_host(bits, P, H, W, W, n_runs, offsets, counts, total, status);
}

// Planes whose rows end inside their last word (cvlm_mask_pack_sized's): W - 32 < Wt <= W
int cvlm_mask_rle_count_w(const uint32_t* bits, int32_t P, int32_t H, int32_t W, int32_t Wt, int32_t* n_runs, void* stream) {
    return rl_count(bits, P, H, W, Wt, n_runs, stream);
}

int cvlm_mask_rle_emit_w(const uint32_t* bits, int32_t P, int32_t H, int32_t W, int32_t Wt, const int64_t* offsets, int32_t* counts,
                         int64_t total, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
    return rl_emit(bits, P, H, W, Wt, offsets, counts, total, status, workspace, workspace_bytes, stream);
}

int cvlm_debug_mask_rle_host_w(const uint32_t* bits, int32_t P, int32_t H, int32_t W, int32_t Wt, int32_t* n_runs, const int64_t* offsets,
                               int32_t* counts, int64_t total, int32_t* status) {
    return rl_host(bits, P, H, W, Wt, n_runs, offsets, counts, total, status);
}

}  // extern "C"
