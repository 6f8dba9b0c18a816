// Label maps on the device (include/cvlm.h: cvlm_label_*): which of an image's K hypotheses owns a pixel -- the per-pixel
// argmax of Mask2Former's panoptic_inference over `score * sigmoid-mask` at the image's own size --, the per-hypothesis areas and the
// overlap test of that function, the lookup that turns a map of hypotheses into a map of classes or segment ids, and mmseg's
// intersect_and_union histogram of a label map against ground truth.  The per-thread logic is labels_logic.h, shared with the
// sequential host entries at the end of this file.  The only floating-point results are the value of sized_logic.h and one product;
// everything behind them is integers.
//
// A pixel's state is 8 bytes, and the public maps are part of it: score f32 (the best s so far), winner int16 (-1: none yet),
// segment int16 (the winner where the winner's own sized bit is set, else -1).  cvlm_label_accumulate reads and writes it once per
// call; no thread waits for another workgroup and no pixel is touched by two threads of a launch.
#include <algorithm>

#include "../../include/cvlm.h"
#include "common.h"
#include "labels_logic.h"

namespace {

typedef unsigned long long u64;

__global__ __launch_bounds__(256) void lb_init_kernel(float* __restrict__ score, int16_t* __restrict__ winner, int16_t* __restrict__ segment,
                                                      int64_t n_pix, int* __restrict__ areas, int* __restrict__ segment_id, int64_t P,
                                                      int* __restrict__ n_segments, int B, int* __restrict__ status) {
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_pix || i < 3 * P; i += step) {
        if (i == 0) status[0] = 0;
        if (i < n_pix) { score[i] = 0.0f; winner[i] = -1; segment[i] = -1; }
        if (i < 3 * P) areas[i] = 0;
        if (i < P) segment_id[i] = 0;
        if (i < B) n_segments[i] = 0;
    }
}

// what every pixel kernel does first: image b's table entries, the same for every thread of the image
struct lb_image { int h, w, upr, units; int64_t off; };
__device__ __forceinline__ bool lb_image_of(const int* __restrict__ dims, const int64_t* __restrict__ pix_off, int b, int64_t n_pix,
                                            int* __restrict__ status, lb_image& im) {
    im.h = dims[2 * b]; im.w = dims[2 * b + 1];
    im.off = pix_off[b];
    if (!lb_image_ok(im.h, im.w, im.off, pix_off[b + 1], n_pix)) {    // nothing of the image is read or stored
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, 1);
        return false;
    }
    im.upr = lb_units_per_row(im.w);
    im.units = im.h * im.upr;
    return true;
}

// Image b_first + blockIdx.y, its planes of [p0, p1).  Wave v of workgroup g takes the units 4 g + v, + 4 gridDim.x, ...; a lane
// forms its pixel's two axis tables once, then walks the planes in increasing k with the running best in registers.  The set bits of
// a plane are counted by ballot and popcount into the workgroup's LDS, LB_TILE planes at a time, and reach orig_area as one integer
// atomic per plane and workgroup that found a bit.
__global__ __launch_bounds__(256) void lb_accumulate_kernel(const float* __restrict__ logits, int p0, int p1, int Hs, int Ws, int K,
                                                            const int* __restrict__ dims, const int64_t* __restrict__ pix_off,
                                                            const float* __restrict__ weights, int level, float* __restrict__ score,
                                                            int16_t* __restrict__ winner, int16_t* __restrict__ segment, int64_t n_pix,
                                                            int b_first, int* __restrict__ orig_area, int* __restrict__ status) {
    __shared__ int cnt[LB_TILE];
    const int b = b_first + blockIdx.y;
    lb_image im;
    if (!lb_image_of(dims, pix_off, b, n_pix, status, im)) return;
    if (blockIdx.x * 4 >= im.units) return;                           // the whole workgroup: no barrier has been passed
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int first = b * K;                                          // B * K < 2^30
    const int ka = max(p0, first) - first, kb = min(p1, first + K) - first;
    const double sx = (double)Ws / (double)im.w, sy = (double)Hs / (double)im.h;
    const int64_t plane_elems = (int64_t)Hs * Ws;
    for (int kt = ka; kt < kb; kt += LB_TILE) {
        const int kn = min(LB_TILE, kb - kt);
        for (int i = threadIdx.x; i < kn; i += 256) cnt[i] = 0;
        __syncthreads();
        for (int u = blockIdx.x * 4 + wave; u < im.units; u += gridDim.x * 4) {
            const int y = u / im.upr, x = 64 * (u - y * im.upr) + lane;
            const bool valid = x < im.w;
            const int64_t pix = im.off + (int64_t)y * im.w + x;
            lb_best best = {0.0f, -1, false};
            sz_axis ax = {0, 0, 0.0f, 0.0f}, ay = ax;
            if (valid) {
                best.s = score[pix];
                best.k = winner[pix];
                best.bit = segment[pix] >= 0;
                ax = sz_axis_of(x, Ws, sx, true);
                ay = sz_axis_of(y, Hs, sy, false);
            }
            for (int k = kt; k < kt + kn; ++k) {
                bool bit = false;
                if (valid) {
                    const float v = lb_value(logits + (int64_t)(first + k - p0) * plane_elems, Ws, ax, ay);
                    bit = sz_bit(v, level);
                    lb_offer(best, k, weights ? weights[first + k] : 1.0f, v, bit);
                }
                const u64 m = __ballot(bit);
                if (m && lane == 0) atomicAdd(&cnt[k - kt], __popcll(m));
            }
            if (valid) {
                score[pix] = best.s;
                winner[pix] = (int16_t)best.k;
                segment[pix] = (int16_t)(best.bit ? best.k : -1);
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < kn; i += 256)
            if (cnt[i]) atomicAdd(&orig_area[first + kt + i], cnt[i]);
        __syncthreads();
    }
}

// won_area and kept_area from the state: the lanes of a wave that hold the same k are counted by ballot, and the counts of one k are
// held back (wave-uniform registers) until the wave meets another k -- neighbours usually agree, so a wave that walks a region of one
// winner ends in one atomic per count instead of one per unit
__global__ __launch_bounds__(256) void lb_count_kernel(int K, const int* __restrict__ dims, const int64_t* __restrict__ pix_off,
                                                       const int16_t* __restrict__ winner, const int16_t* __restrict__ segment,
                                                       int64_t n_pix, int* __restrict__ won_area, int* __restrict__ kept_area,
                                                       int* __restrict__ status) {
    const int b = blockIdx.y;
    lb_image im;
    if (!lb_image_of(dims, pix_off, b, n_pix, status, im)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int held_k = -1, held_won = 0, held_kept = 0;                     // the same in every lane; a wave sees fewer than 2^29 pixels
    for (int u = blockIdx.x * 4 + wave; u < im.units; u += gridDim.x * 4) {
        const int y = u / im.upr, x = 64 * (u - y * im.upr) + lane;
        int k = -1;
        bool in = false;
        if (x < im.w) {
            const int64_t pix = im.off + (int64_t)y * im.w + x;
            k = winner[pix];
            in = segment[pix] >= 0;
        }
        bool todo = k >= 0 && k < K;
        for (u64 open = __ballot(todo); open; open = __ballot(todo)) {
            const int lead = __ffsll(open) - 1;
            const int k0 = __shfl(k, lead, 64);
            const bool same = todo && k == k0;
            const u64 m = __ballot(same), mk = __ballot(same && in);
            if (k0 != held_k) {
                if (held_k >= 0 && lane == 0) {
                    atomicAdd(&won_area[b * K + held_k], held_won);
                    if (held_kept) atomicAdd(&kept_area[b * K + held_k], held_kept);
                }
                held_k = k0; held_won = 0; held_kept = 0;
            }
            held_won += __popcll(m);
            held_kept += __popcll(mk);
            if (same) todo = false;
        }
    }
    if (held_k >= 0 && lane == 0) {
        atomicAdd(&won_area[b * K + held_k], held_won);
        if (held_kept) atomicAdd(&kept_area[b * K + held_k], held_kept);
    }
}

// one wave per image: kept, and the running count of the kept in increasing k
__global__ __launch_bounds__(64) void lb_segments_kernel(int K, double overlap_threshold, const int* __restrict__ areas, int64_t P,
                                                         int* __restrict__ segment_id, int* __restrict__ n_segments) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int run = 0;
    for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + lane;
        const int64_t p = (int64_t)b * K + k;
        const bool kept = k < K && lb_kept(areas[P + p], areas[p], areas[2 * P + p], overlap_threshold);
        const u64 m = __ballot(kept);
        if (k < K) segment_id[p] = kept ? run + __popcll(m & (((u64)1 << lane) - 1)) + 1 : 0;
        run += __popcll(m);
    }
    if (lane == 0) n_segments[b] = run;
}

// segment: the winner where its bit is set AND it is kept
__global__ __launch_bounds__(256) void lb_paint_kernel(int K, const int* __restrict__ dims, const int64_t* __restrict__ pix_off,
                                                       int16_t* __restrict__ segment, int64_t n_pix, const int* __restrict__ segment_id,
                                                       int* __restrict__ status) {
    const int b = blockIdx.y;
    lb_image im;
    if (!lb_image_of(dims, pix_off, b, n_pix, status, im)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int u = blockIdx.x * 4 + wave; u < im.units; u += gridDim.x * 4) {
        const int y = u / im.upr, x = 64 * (u - y * im.upr) + lane;
        if (x >= im.w) continue;
        const int64_t pix = im.off + (int64_t)y * im.w + x;
        const int s = segment[pix];
        if (s >= 0 && !(s < K && segment_id[b * K + s] > 0)) segment[pix] = -1;
    }
}

__global__ __launch_bounds__(256) void lb_lookup_kernel(const int16_t* __restrict__ map, int K, const int* __restrict__ dims,
                                                        const int64_t* __restrict__ pix_off, int64_t n_pix, const int* __restrict__ table,
                                                        int void_value, int* __restrict__ out, int* __restrict__ status) {
    const int b = blockIdx.y;
    lb_image im;
    if (!lb_image_of(dims, pix_off, b, n_pix, status, im)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int u = blockIdx.x * 4 + wave; u < im.units; u += gridDim.x * 4) {
        const int y = u / im.upr, x = 64 * (u - y * im.upr) + lane;
        if (x >= im.w) continue;
        const int64_t pix = im.off + (int64_t)y * im.w + x;
        const int k = map[pix];
        out[pix] = k >= 0 && k < K ? table[b * K + k] : void_value;
    }
}

__global__ __launch_bounds__(256) void lb_zero_kernel(u64* __restrict__ totals, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) totals[i] = 0;
}

// One pixel of the histogram -> (pred, gt) as classes, or false where the pixel is ignored
template <typename G>
__device__ __forceinline__ bool lb_hist_pixel(const int* __restrict__ pred, const G* __restrict__ gt, int64_t i, int ignore_index,
                                              bool reduce_zero_label, int& p, int& g) {
    g = (int)gt[i];
    if (reduce_zero_label) g = lb_reduce_gt(g);
    if (g == ignore_index) return false;
    p = pred[i];
    return true;
}

// 3 C <= 3 LB_LDS_C counters in the workgroup's LDS (dynamic: 12 C bytes), flushed as 64-bit atomics where non-zero.  A workgroup
// counts fewer than 2^32 pixels.
template <typename G>
__global__ __launch_bounds__(256) void lb_hist_lds_kernel(const int* __restrict__ pred, const G* __restrict__ gt, int64_t n, int C,
                                                          int ignore_index, int reduce_zero_label, u64* __restrict__ totals) {
    extern __shared__ unsigned lb_bins[];
    for (int i = threadIdx.x; i < 3 * C; i += 256) lb_bins[i] = 0u;
    __syncthreads();
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
        int p, g;
        if (!lb_hist_pixel(pred, gt, i, ignore_index, reduce_zero_label != 0, p, g)) continue;
        if (lb_class(p, C)) {
            atomicAdd(&lb_bins[C + p], 1u);
            if (p == g) atomicAdd(&lb_bins[p], 1u);
        }
        if (lb_class(g, C)) atomicAdd(&lb_bins[2 * C + g], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * C; i += 256)
        if (lb_bins[i]) atomicAdd(&totals[i], (u64)lb_bins[i]);
}

// Any C: lanes of a wave that hold the same class issue one 64-bit atomic per count
template <typename G>
__global__ __launch_bounds__(256) void lb_hist_global_kernel(const int* __restrict__ pred, const G* __restrict__ gt, int64_t n, int C,
                                                             int ignore_index, int reduce_zero_label, u64* __restrict__ totals) {
    const int lane = threadIdx.x & 63;
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t i0 = (int64_t)blockIdx.x * 256 + (threadIdx.x - lane); i0 < n; i0 += step) {        // the same for a whole wave
        const int64_t i = i0 + lane;
        int p = -1, g = -1;
        const bool held = i < n && lb_hist_pixel(pred, gt, i, ignore_index, reduce_zero_label != 0, p, g);
        bool todo = held && lb_class(p, C);
        for (u64 open = __ballot(todo); open; open = __ballot(todo)) {
            const int lead = __ffsll(open) - 1;
            const int c = __shfl(p, lead, 64);
            const bool same = todo && p == c;
            const u64 m = __ballot(same), mi = __ballot(same && g == c);
            if (lane == lead) {
                atomicAdd(&totals[C + c], (u64)__popcll(m));
                if (mi) atomicAdd(&totals[c], (u64)__popcll(mi));
            }
            if (same) todo = false;
        }
        todo = held && lb_class(g, C);
        for (u64 open = __ballot(todo); open; open = __ballot(todo)) {
            const int lead = __ffsll(open) - 1;
            const int c = __shfl(g, lead, 64);
            const bool same = todo && g == c;
            const u64 m = __ballot(same);
            if (lane == lead) atomicAdd(&totals[2 * C + c], (u64)__popcll(m));
            if (same) todo = false;
        }
    }
}

// ---- what the entries refuse ----------------------------------------------------------------------------------------------------------
bool lb_bad_tables(int32_t B, int32_t K, const int32_t* dims, const int64_t* pix_off, int64_t n_pix, int64_t max_pixels,
                   const int32_t* status) {
    if (!dims || !pix_off || !status || mb_misaligned(4, dims, status) || mb_misaligned(8, pix_off)) return true;
    if (B < 1 || B > LB_MAX_B || K < 1 || K > LB_MAX_K || n_pix < 1) return true;
    return max_pixels < 1 || max_pixels > (int64_t)SZ_MAX_SIDE * SZ_MAX_SIDE;
}
bool lb_bad_state(const float* score, const int16_t* winner, const int16_t* segment, const int32_t* areas) {
    return !score || !winner || !segment || !areas || mb_misaligned(4, score, areas) || mb_misaligned(2, winner, segment);
}
bool lb_init_bad(const float* score, const int16_t* winner, const int16_t* segment, int64_t n_pix, const int32_t* areas,
                 const int32_t* segment_id, int32_t B, int32_t K, const int32_t* n_segments, const int32_t* status) {
    if (lb_bad_state(score, winner, segment, areas) || !segment_id || !n_segments || !status) return true;
    if (mb_misaligned(4, segment_id, n_segments, status)) return true;
    return B < 1 || B > LB_MAX_B || K < 1 || K > LB_MAX_K || n_pix < 1;
}
bool lb_accumulate_bad(const float* logits, int32_t p0, int32_t p1, int32_t Hs, int32_t Ws, int32_t B, int32_t K, const int32_t* dims,
                       const int64_t* pix_off, const float* weights, int32_t level, const float* score, const int16_t* winner,
                       const int16_t* segment, int64_t n_pix, int64_t max_pixels, const int32_t* areas, const int32_t* status) {
    if (!logits || lb_bad_state(score, winner, segment, areas) || lb_bad_tables(B, K, dims, pix_off, n_pix, max_pixels, status)) return true;
    if (mb_misaligned(4, logits, weights)) return true;
    if (Hs <= 0 || Ws <= 0 || (int64_t)Hs * Ws >= ((int64_t)1 << 31) || level < 1 || level > 255) return true;
    return p0 < 0 || p1 <= p0 || p1 > B * K;
}
bool lb_finish_bad(int32_t B, int32_t K, const int32_t* dims, const int64_t* pix_off, const double* overlap_threshold,
                   const int16_t* winner, const int16_t* segment, int64_t n_pix, int64_t max_pixels, const int32_t* areas,
                   const int32_t* segment_id, const int32_t* n_segments, const int32_t* status) {
    if (!winner || !segment || !areas || !segment_id || !n_segments || !overlap_threshold) return true;
    if (lb_bad_tables(B, K, dims, pix_off, n_pix, max_pixels, status)) return true;
    if (mb_misaligned(4, areas, segment_id, n_segments) || mb_misaligned(2, winner, segment)) return true;
    const double t = overlap_threshold[0];
    return !(t > 0.0 && t <= 1.0);                                    // a NaN is refused too
}
bool lb_lookup_bad(const int16_t* map, int32_t B, int32_t K, const int32_t* dims, const int64_t* pix_off, int64_t n_pix,
                   int64_t max_pixels, const int32_t* table, const int32_t* out, const int32_t* status) {
    if (!map || !table || !out || lb_bad_tables(B, K, dims, pix_off, n_pix, max_pixels, status)) return true;
    return mb_misaligned(4, table, out) || mb_misaligned(2, map);
}
bool lb_hist_bad(const int32_t* pred, const void* gt, int32_t gt_is_u8, int64_t n, int32_t C, const int64_t* totals) {
    if (!pred || !gt || !totals || n < 1 || C < 1 || C > LB_MAX_C || (gt_is_u8 != 0 && gt_is_u8 != 1)) return true;
    return mb_misaligned(4, pred) || mb_misaligned(8, totals) || (!gt_is_u8 && mb_misaligned(4, gt));
}

// workgroups per image of a pixel kernel: one per four units of the largest image, about 8192 in all; the waves walk the rest in strides
int lb_grid_x(int64_t max_pixels, int images) {
    const int64_t by_work = (max_pixels / 64 + SZ_MAX_SIDE + 3) / 4;  // units <= h * w / 64 + h
    const int64_t want = (8192 + images - 1) / images;
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(by_work, want), 2048));
}

template <typename G>
void lb_hist_launch(const int32_t* pred, const G* gt, int64_t n, int32_t C, int32_t ignore_index, int32_t reduce_zero_label,
                    int64_t* totals, hipStream_t st) {
    const int gx = (int)std::max<int64_t>(1, std::min<int64_t>((n + 4095) / 4096, 512));
    if (C <= LB_LDS_C)
        hipLaunchKernelGGL(lb_hist_lds_kernel<G>, dim3(gx), dim3(256), (size_t)12 * C, st, (const int*)pred, gt, n, (int)C, (int)ignore_index,
                           (int)reduce_zero_label, (u64*)totals);
    else
        hipLaunchKernelGGL(lb_hist_global_kernel<G>, dim3(gx), dim3(256), 0, st, (const int*)pred, gt, n, (int)C, (int)ignore_index,
                           (int)reduce_zero_label, (u64*)totals);
}

template <typename G>
void lb_hist_host(const int32_t* pred, const G* gt, int64_t n, int32_t C, int32_t ignore_index, bool reduce_zero_label, int64_t* totals) {
    for (int64_t i = 0; i < n; ++i) {
        int g = (int)gt[i];
        if (reduce_zero_label) g = lb_reduce_gt(g);
        if (g == ignore_index) continue;
        const int p = pred[i];
        if (lb_class(p, C)) {
            ++totals[C + p];
            if (p == g) ++totals[p];
        }
        if (lb_class(g, C)) ++totals[2 * C + g];
    }
}

}  // namespace

extern "C" {

int cvlm_label_init(float* score, int16_t* winner, int16_t* segment, int64_t n_pix, int32_t* areas, int32_t* segment_id, int32_t B,
                    int32_t K, int32_t* n_segments, int32_t* status, void* stream) {
    if (lb_init_bad(score, winner, segment, n_pix, areas, segment_id, B, K, n_segments, status)) return CVLM_E_BADARG;
    const int64_t P = (int64_t)B * K, cells = std::max(n_pix, 3 * P);
    const int gx = (int)std::min<int64_t>((cells + 255) / 256, 8192);
    hipLaunchKernelGGL(lb_init_kernel, dim3(gx), dim3(256), 0, (hipStream_t)stream, score, winner, segment, n_pix, (int*)areas,
                       (int*)segment_id, P, (int*)n_segments, (int)B, (int*)status);
    CVLM_CHECK_LAUNCH();
    return 0;
}

int cvlm_label_accumulate(const float* logits, int32_t p0, int32_t p1, int32_t Hs, int32_t Ws, int32_t B, int32_t K, const int32_t* dims,
                          const int64_t* pix_offsets, const float* weights, int32_t level, float* score, int16_t* winner,
                          int16_t* segment, int64_t n_pix, int64_t max_pixels, int32_t* areas, int32_t* status, void* stream) {
    if (lb_accumulate_bad(logits, p0, p1, Hs, Ws, B, K, dims, pix_offsets, weights, level, score, winner, segment, n_pix, max_pixels, areas,
                          status))
        return CVLM_E_BADARG;
    const int b_first = p0 / K, images = (p1 - 1) / K - b_first + 1;
    hipLaunchKernelGGL(lb_accumulate_kernel, dim3(lb_grid_x(max_pixels, images), images), dim3(256), 0, (hipStream_t)stream, logits, (int)p0,
                       (int)p1, (int)Hs, (int)Ws, (int)K, (const int*)dims, pix_offsets, weights, (int)level, score, winner, segment, n_pix,
                       b_first, (int*)areas, (int*)status);
    CVLM_CHECK_LAUNCH();
    return 0;
}

int cvlm_label_finish(int32_t B, int32_t K, const int32_t* dims, const int64_t* pix_offsets, const double* overlap_threshold,
                      const int16_t* winner, int16_t* segment, int64_t n_pix, int64_t max_pixels, int32_t* areas, int32_t* segment_id,
                      int32_t* n_segments, int32_t* status, void* stream) {
    if (lb_finish_bad(B, K, dims, pix_offsets, overlap_threshold, winner, segment, n_pix, max_pixels, areas, segment_id, n_segments, status))
        return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int64_t P = (int64_t)B * K;
    const dim3 grid(lb_grid_x(max_pixels, B), B);
    hipLaunchKernelGGL(lb_count_kernel, grid, dim3(256), 0, st, (int)K, (const int*)dims, pix_offsets, winner, (const int16_t*)segment, n_pix,
                       (int*)areas + P, (int*)areas + 2 * P, (int*)status);
    CVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(lb_segments_kernel, dim3(B), dim3(64), 0, st, (int)K, overlap_threshold[0], (const int*)areas, P, (int*)segment_id,
                       (int*)n_segments);
    CVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(lb_paint_kernel, grid, dim3(256), 0, st, (int)K, (const int*)dims, pix_offsets, segment, n_pix,
                       (const int*)segment_id, (int*)status);
    CVLM_CHECK_LAUNCH();
    return 0;
}

int cvlm_label_lookup(const int16_t* map, int32_t B, int32_t K, const int32_t* dims, const int64_t* pix_offsets, int64_t n_pix,
                      int64_t max_pixels, const int32_t* table, int32_t void_value, int32_t* out, int32_t* status, void* stream) {
    if (lb_lookup_bad(map, B, K, dims, pix_offsets, n_pix, max_pixels, table, out, status)) return CVLM_E_BADARG;
    hipLaunchKernelGGL(lb_lookup_kernel, dim3(lb_grid_x(max_pixels, B), B), dim3(256), 0, (hipStream_t)stream, map, (int)K, (const int*)dims,
                       pix_offsets, n_pix, (const int*)table, (int)void_value, (int*)out, (int*)status);
    CVLM_CHECK_LAUNCH();
    return 0;
}

int cvlm_label_iou_hist(const int32_t* pred, const void* gt, int32_t gt_is_u8, int64_t n, int32_t C, int32_t ignore_index,
                        int32_t reduce_zero_label, int32_t zero_first, int64_t* totals, void* stream) {
    if (lb_hist_bad(pred, gt, gt_is_u8, n, C, totals)) return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (zero_first) {
        hipLaunchKernelGGL(lb_zero_kernel, dim3((3 * C + 255) / 256), dim3(256), 0, st, (u64*)totals, 3 * (int)C);
        CVLM_CHECK_LAUNCH();
    }
    if (gt_is_u8) lb_hist_launch(pred, (const uint8_t*)gt, n, C, ignore_index, reduce_zero_label, totals, st);
    else lb_hist_launch(pred, (const int32_t*)gt, n, C, ignore_index, reduce_zero_label, totals, st);
    CVLM_CHECK_LAUNCH();
    return 0;
}

// ---- the same functions on host memory, image by image and pixel by pixel --------------------------------------------------------------
int cvlm_debug_label_init_host(float* score, int16_t* winner, int16_t* segment, int64_t n_pix, int32_t* areas, int32_t* segment_id,
                               int32_t B, int32_t K, int32_t* n_segments, int32_t* status) {
    if (lb_init_bad(score, winner, segment, n_pix, areas, segment_id, B, K, n_segments, status)) return CVLM_E_BADARG;
    const int64_t P = (int64_t)B * K;
    status[0] = 0;
    for (int64_t i = 0; i < n_pix; ++i) { score[i] = 0.0f; winner[i] = -1; segment[i] = -1; }
    for (int64_t i = 0; i < 3 * P; ++i) areas[i] = 0;
    for (int64_t i = 0; i < P; ++i) segment_id[i] = 0;
    for (int b = 0; b < B; ++b) n_segments[b] = 0;
    return 0;
}

int cvlm_debug_label_accumulate_host(const float* logits, int32_t p0, int32_t p1, int32_t Hs, int32_t Ws, int32_t B, int32_t K,
                                     const int32_t* dims, const int64_t* pix_offsets, const float* weights, int32_t level, float* score,
                                     int16_t* winner, int16_t* segment, int64_t n_pix, int64_t max_pixels, int32_t* areas,
                                     int32_t* status) {
    if (lb_accumulate_bad(logits, p0, p1, Hs, Ws, B, K, dims, pix_offsets, weights, level, score, winner, segment, n_pix, max_pixels, areas,
                          status))
        return CVLM_E_BADARG;
    const int64_t plane_elems = (int64_t)Hs * Ws;
    for (int b = p0 / K; b <= (p1 - 1) / K; ++b) {
        const int h = dims[2 * b], w = dims[2 * b + 1];
        const int64_t off = pix_offsets[b];
        if (!lb_image_ok(h, w, off, pix_offsets[b + 1], n_pix)) { status[0] |= 1; continue; }
        const int first = b * K;
        const int ka = std::max(p0, first) - first, kb = std::min(p1, first + K) - first;
        const double sx = (double)Ws / (double)w, sy = (double)Hs / (double)h;
        for (int y = 0; y < h; ++y) {
            const sz_axis ay = sz_axis_of(y, Hs, sy, false);
            for (int x = 0; x < w; ++x) {
                const sz_axis ax = sz_axis_of(x, Ws, sx, true);
                const int64_t pix = off + (int64_t)y * w + x;
                lb_best best = {score[pix], winner[pix], segment[pix] >= 0};
                for (int k = ka; k < kb; ++k) {
                    const float v = lb_value(logits + (int64_t)(first + k - p0) * plane_elems, Ws, ax, ay);
                    const bool bit = sz_bit(v, level);
                    lb_offer(best, k, weights ? weights[first + k] : 1.0f, v, bit);
                    if (bit) ++areas[first + k];
                }
                score[pix] = best.s;
                winner[pix] = (int16_t)best.k;
                segment[pix] = (int16_t)(best.bit ? best.k : -1);
            }
        }
    }
    return 0;
}

int cvlm_debug_label_finish_host(int32_t B, int32_t K, const int32_t* dims, const int64_t* pix_offsets, const double* overlap_threshold,
                                 const int16_t* winner, int16_t* segment, int64_t n_pix, int64_t max_pixels, int32_t* areas,
                                 int32_t* segment_id, int32_t* n_segments, int32_t* status) {
    if (lb_finish_bad(B, K, dims, pix_offsets, overlap_threshold, winner, segment, n_pix, max_pixels, areas, segment_id, n_segments, status))
        return CVLM_E_BADARG;
    const int64_t P = (int64_t)B * K;
    for (int b = 0; b < B; ++b) {
        const int h = dims[2 * b], w = dims[2 * b + 1];
        const int64_t off = pix_offsets[b];
        const bool ok = lb_image_ok(h, w, off, pix_offsets[b + 1], n_pix);
        if (!ok) status[0] |= 1;
        for (int64_t i = 0; ok && i < (int64_t)h * w; ++i) {
            const int k = winner[off + i];
            if (k < 0 || k >= K) continue;
            ++areas[P + (int64_t)b * K + k];
            if (segment[off + i] >= 0) ++areas[2 * P + (int64_t)b * K + k];
        }
        int run = 0;
        for (int k = 0; k < K; ++k) {
            const int64_t p = (int64_t)b * K + k;
            const bool kept = lb_kept(areas[P + p], areas[p], areas[2 * P + p], overlap_threshold[0]);
            segment_id[p] = kept ? ++run : 0;
        }
        n_segments[b] = run;
        for (int64_t i = 0; ok && i < (int64_t)h * w; ++i) {
            const int s = segment[off + i];
            if (s >= 0 && !(s < K && segment_id[(int64_t)b * K + s] > 0)) segment[off + i] = -1;
        }
    }
    return 0;
}

int cvlm_debug_label_lookup_host(const int16_t* map, int32_t B, int32_t K, const int32_t* dims, const int64_t* pix_offsets, int64_t n_pix,
                                 int64_t max_pixels, const int32_t* table, int32_t void_value, int32_t* out, int32_t* status) {
    if (lb_lookup_bad(map, B, K, dims, pix_offsets, n_pix, max_pixels, table, out, status)) return CVLM_E_BADARG;
    for (int b = 0; b < B; ++b) {
        const int h = dims[2 * b], w = dims[2 * b + 1];
        const int64_t off = pix_offsets[b];
        if (!lb_image_ok(h, w, off, pix_offsets[b + 1], n_pix)) { status[0] |= 1; continue; }
        for (int64_t i = 0; i < (int64_t)h * w; ++i) {
            const int k = map[off + i];
            out[off + i] = k >= 0 && k < K ? table[(int64_t)b * K + k] : void_value;
        }
    }
    return 0;
}

int cvlm_debug_label_iou_hist_host(const int32_t* pred, const void* gt, int32_t gt_is_u8, int64_t n, int32_t C, int32_t ignore_index,
                                   int32_t reduce_zero_label, int32_t zero_first, int64_t* totals) {
    if (lb_hist_bad(pred, gt, gt_is_u8, n, C, totals)) return CVLM_E_BADARG;
    if (zero_first)
        for (int i = 0; i < 3 * C; ++i) totals[i] = 0;
    if (gt_is_u8) lb_hist_host(pred, (const uint8_t*)gt, n, C, ignore_index, reduce_zero_label != 0, totals);
    else lb_hist_host(pred, (const int32_t*)gt, n, C, ignore_index, reduce_zero_label != 0, totals);
    return 0;
}

}  // extern "C"
