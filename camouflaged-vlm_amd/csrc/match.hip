// COCO matching on the device (include/cvlm.h: cvlm_coco_match): detections against annotations per (image, category)
// group, the published greedy loop of COCOeval.evaluateImg for every (area range, IoU threshold) instance at once, from the
// intersections cvlm_mask_inter_sized left on the device.  Integers and one double division per pair; nothing is accumulated in
// floating point, so the device and cvlm_debug_coco_match_host give the same bytes.
//
// Two launches: mt_init_kernel fills every output with "no match, ignored"; mt_match_kernel runs one workgroup of two waves per group.
//   1. stage the scores, the crowd flags and the ignore bytes in LDS, write gt_ignore;
//   2. stable rank of the scores by counting (D <= 1024: at most 8 passes of 1024 comparisons per thread), write dt_order;
//   3. per detection in rank order: all threads divide the IoU row into LDS (threads over annotations), then thread i < A * T runs
//      its instance over the row -- uniform LDS reads, its own column of the taken-bitset -- and stores the detection's match.
// No workgroup waits for another; a refused group reads nothing of its block and leaves what mt_init_kernel wrote.
#include <algorithm>
#include <vector>

#include "../../include/cvlm.h"
#include "common.h"
#include "match_logic.h"

namespace {

constexpr int MT_THREADS = 128;                  // one thread per instance
static_assert(MT_THREADS >= MT_MAX_A * MT_MAX_T, "an instance needs a thread");

__global__ __launch_bounds__(256) void mt_init_kernel(int* __restrict__ dt_order, int* __restrict__ dt_match, uint8_t* __restrict__ dt_ignore,
                                                      int* __restrict__ gt_match, uint8_t* __restrict__ gt_ignore, int ND, int NG, int A,
                                                      int AT, int* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) status[0] = 0;
    if (i < ND) dt_order[i] = -1;
    if (i < (int64_t)AT * ND) { dt_match[i] = -1; dt_ignore[i] = 1; }
    if (i < (int64_t)AT * NG) gt_match[i] = -1;
    if (i < (int64_t)A * NG) gt_ignore[i] = 1;
}

// BOUNDARY: step (3) divides twice per pair -- the mask's integers and the boundary's (inter_b, det_area_b, gt_area_b)
// -- and keeps the minimum; the false form never reads the three tables.
template <bool BOUNDARY>
__global__ __launch_bounds__(MT_THREADS) void mt_match_kernel(const int* __restrict__ det_off, const int* __restrict__ gt_off,
                                                              const int64_t* __restrict__ pair_off, const int* __restrict__ inter, int64_t N,
                                                              const int* __restrict__ det_area, const float* __restrict__ score, int ND,
                                                              const int* __restrict__ gt_area, const double* __restrict__ gt_range_area,
                                                              const uint8_t* __restrict__ gt_crowd, int NG, const double* __restrict__ iou_thrs,
                                                              int T, const double* __restrict__ area_rngs, int A, int max_det,
                                                              int* __restrict__ dt_order, int* __restrict__ dt_match,
                                                              uint8_t* __restrict__ dt_ignore, int* __restrict__ gt_match,
                                                              uint8_t* __restrict__ gt_ignore, int* __restrict__ status,
                                                              const int* __restrict__ inter_b, const int* __restrict__ det_area_b,
                                                              const int* __restrict__ gt_area_b) {
    __shared__ double row[MT_CAP];                              // the scores (as floats) until the order stands, then one IoU row
    __shared__ uint32_t taken[(MT_CAP / 32) * MT_THREADS];      // word-major: word k of instance i at [k * MT_THREADS + i]
    __shared__ int order[MT_CAP];
    __shared__ uint8_t ign[MT_CAP], crowd[MT_CAP];
    const int tid = threadIdx.x;
    mt_group q;
    if (!mt_group_ok(det_off, gt_off, pair_off, blockIdx.x, ND, NG, N, q)) {      // the same for every thread of the group
        if (tid == 0) atomicOr(status, 1);
        return;
    }
    float* sc = (float*)row;
    for (int i = tid; i < q.D; i += MT_THREADS) sc[i] = score[q.d0 + i];
    for (int g = tid; g < q.G; g += MT_THREADS) {
        const bool c = gt_crowd[q.g0 + g] != 0;
        const uint32_t m = mt_ignore_mask(c, gt_range_area[q.g0 + g], area_rngs, A);
        crowd[g] = c;
        ign[g] = (uint8_t)m;
        for (int a = 0; a < A; ++a) gt_ignore[(int64_t)a * NG + q.g0 + g] = (m >> a) & 1u;
    }
    const int words = (q.G + 31) >> 5;
    for (int k = tid; k < words * MT_THREADS; k += MT_THREADS) taken[k] = 0u;
    __syncthreads();
    for (int i = tid; i < q.D; i += MT_THREADS) {
        const float si = sc[i];
        int r = 0;
        for (int j = 0; j < q.D; ++j) r += mt_precedes(sc[j], j, si, i) ? 1 : 0;
        order[r] = i;
        dt_order[q.d0 + r] = q.d0 + i;
    }
    __syncthreads();
    const int AT = A * T;
    const bool active = tid < AT;
    const int a = active ? tid / T : 0, t = active ? tid % T : 0;
    const double thr = mt_threshold(iou_thrs[t]), lo = area_rngs[2 * a], hi = area_rngs[2 * a + 1];
    const int R = q.D < max_det ? q.D : max_det;
    for (int r = 0; r < R; ++r) {
        const int d = order[r];
        const int ad = det_area[q.d0 + d];
        const int* block = inter + q.p0 + (int64_t)d * q.G;
        if constexpr (BOUNDARY) {
            const int adb = det_area_b[q.d0 + d];
            const int* block_b = inter_b + q.p0 + (int64_t)d * q.G;
            for (int g = tid; g < q.G; g += MT_THREADS)
                row[g] = mt_iou_min(block[g], ad, gt_area[q.g0 + g], block_b[g], adb, gt_area_b[q.g0 + g], crowd[g] != 0);
        } else {
            for (int g = tid; g < q.G; g += MT_THREADS) row[g] = mt_iou(block[g], ad, gt_area[q.g0 + g], crowd[g] != 0);
        }
        __syncthreads();
        if (active) {
            const int m = mt_pick(row, q.G, ign, crowd, a, thr, taken + tid, MT_THREADS);
            const int64_t at = (int64_t)a * T + t;
            bool ig;
            if (m >= 0) {
                taken[(m >> 5) * MT_THREADS + tid] |= 1u << (m & 31);
                gt_match[at * NG + q.g0 + m] = q.d0 + d;
                ig = (ign[m] >> a) & 1;
            } else {
                ig = (double)ad < lo || (double)ad > hi;
            }
            dt_match[at * ND + q.d0 + r] = m >= 0 ? q.g0 + m : -1;
            dt_ignore[at * ND + q.d0 + r] = ig ? 1 : 0;
        }
        __syncthreads();
    }
}

// what both entries refuse
bool mt_bad(const int32_t* det_off, const int32_t* gt_off, const int64_t* pair_off, int32_t E, const int32_t* inter, int64_t N,
            const int32_t* det_area, const float* score, int32_t ND, const int32_t* gt_area, const double* gt_range_area,
            const uint8_t* gt_crowd, int32_t NG, const double* iou_thrs, int32_t T, const double* area_rngs, int32_t A, int32_t max_det,
            const int32_t* dt_order, const int32_t* dt_match, const uint8_t* dt_ignore, const int32_t* gt_match, const uint8_t* gt_ignore,
            const int32_t* status) {
    if (!det_off || !gt_off || !pair_off || !iou_thrs || !area_rngs || !status) return true;
    if (E < 1 || E > MT_MAX_ROWS || N < 0 || N > MT_MAX_ROWS || ND < 0 || ND > MT_MAX_ROWS || NG < 0 || NG > MT_MAX_ROWS) return true;
    if (T < 1 || T > MT_MAX_T || A < 1 || A > MT_MAX_A || max_det < 1) return true;
    if (N > 0 && !inter) return true;
    if (ND > 0 && (!det_area || !score || !dt_order || !dt_match || !dt_ignore)) return true;
    if (NG > 0 && (!gt_area || !gt_range_area || !gt_crowd || !gt_match || !gt_ignore)) return true;
    if (mb_misaligned(4, det_off, gt_off, inter, det_area, score, gt_area, dt_order, dt_match, gt_match, status)) return true;
    return mb_misaligned(8, pair_off, gt_range_area, iou_thrs, area_rngs);
}

// what the boundary entries refuse on top of it: each of the three tables NULL where its count is not 0, or off 4 bytes
bool mt_bad_boundary(const int32_t* inter_b, int64_t N, const int32_t* det_area_b, int32_t ND, const int32_t* gt_area_b, int32_t NG) {
    if ((N > 0 && !inter_b) || (ND > 0 && !det_area_b) || (NG > 0 && !gt_area_b)) return true;
    return mb_misaligned(4, inter_b, det_area_b, gt_area_b);
}

// the two launches of both device entries
template <bool BOUNDARY>
int mt_launch(const int32_t* det_offsets, const int32_t* gt_offsets, const int64_t* pair_offsets, int32_t E, const int32_t* inter, int64_t N,
              const int32_t* det_area, const float* score, int32_t ND, const int32_t* gt_area, const double* gt_range_area,
              const uint8_t* gt_crowd, int32_t NG, const double* iou_thrs, int32_t T, const double* area_rngs, int32_t A, int32_t max_det,
              int32_t* dt_order, int32_t* dt_match, uint8_t* dt_ignore, int32_t* gt_match, uint8_t* gt_ignore, int32_t* status,
              const int32_t* inter_b, const int32_t* det_area_b, const int32_t* gt_area_b, hipStream_t st) {
    const int AT = A * T;
    const int64_t cells = std::max<int64_t>(1, (int64_t)AT * std::max(ND, NG));             // <= 2^27
    hipLaunchKernelGGL(mt_init_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, (int*)dt_order, (int*)dt_match, dt_ignore,
                       (int*)gt_match, gt_ignore, (int)ND, (int)NG, (int)A, AT, (int*)status);
    CVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(mt_match_kernel<BOUNDARY>, dim3(E), dim3(MT_THREADS), 0, st, (const int*)det_offsets, (const int*)gt_offsets,
                       pair_offsets, (const int*)inter, N, (const int*)det_area, score, (int)ND, (const int*)gt_area, gt_range_area, gt_crowd,
                       (int)NG, iou_thrs, (int)T, area_rngs, (int)A, (int)max_det, (int*)dt_order, (int*)dt_match, dt_ignore, (int*)gt_match,
                       gt_ignore, (int*)status, (const int*)inter_b, (const int*)det_area_b, (const int*)gt_area_b);
    CVLM_CHECK_LAUNCH();
    return 0;
}

// the sequential form of both host entries
int mt_host(const int32_t* det_offsets, const int32_t* gt_offsets, const int64_t* pair_offsets, int32_t E, const int32_t* inter, int64_t N,
            const int32_t* det_area, const float* score, int32_t ND, const int32_t* gt_area, const double* gt_range_area,
            const uint8_t* gt_crowd, int32_t NG, const double* iou_thrs, int32_t T, const double* area_rngs, int32_t A, int32_t max_det,
            int32_t* dt_order, int32_t* dt_match, uint8_t* dt_ignore, int32_t* gt_match, uint8_t* gt_ignore, int32_t* status, bool boundary,
            const int32_t* inter_b, const int32_t* det_area_b, const int32_t* gt_area_b) {
    const int AT = A * T;
    status[0] = 0;
    for (int i = 0; i < ND; ++i) dt_order[i] = -1;
    for (int64_t i = 0; i < (int64_t)AT * ND; ++i) { dt_match[i] = -1; dt_ignore[i] = 1; }
    for (int64_t i = 0; i < (int64_t)AT * NG; ++i) gt_match[i] = -1;
    for (int64_t i = 0; i < (int64_t)A * NG; ++i) gt_ignore[i] = 1;
    std::vector<double> row;
    std::vector<uint32_t> taken;
    std::vector<int> order;
    std::vector<uint8_t> ign, crowd;
    for (int e = 0; e < E; ++e) {
        mt_group q;
        if (!mt_group_ok(det_offsets, gt_offsets, pair_offsets, e, ND, NG, N, q)) {
            status[0] |= 1;
            continue;
        }
        const int words = (q.G + 31) >> 5;
        row.assign((size_t)q.G, 0.0);
        taken.assign((size_t)(words + 1) * AT, 0u);                  // never empty: instance i starts at element i
        order.assign((size_t)q.D, 0);
        ign.assign((size_t)q.G, 0);
        crowd.assign((size_t)q.G, 0);
        for (int g = 0; g < q.G; ++g) {
            const bool c = gt_crowd[q.g0 + g] != 0;
            const uint32_t m = mt_ignore_mask(c, gt_range_area[q.g0 + g], area_rngs, A);
            crowd[(size_t)g] = c;
            ign[(size_t)g] = (uint8_t)m;
            for (int a = 0; a < A; ++a) gt_ignore[(int64_t)a * NG + q.g0 + g] = (m >> a) & 1u;
        }
        for (int i = 0; i < q.D; ++i) {
            int r = 0;
            for (int j = 0; j < q.D; ++j) r += mt_precedes(score[q.d0 + j], j, score[q.d0 + i], i) ? 1 : 0;
            order[(size_t)r] = i;
            dt_order[q.d0 + r] = q.d0 + i;
        }
        const int R = q.D < max_det ? q.D : max_det;
        for (int r = 0; r < R; ++r) {
            const int d = order[(size_t)r];
            const int ad = det_area[q.d0 + d];
            for (int g = 0; g < q.G; ++g) {
                const int64_t at = q.p0 + (int64_t)d * q.G + g;
                const bool c = crowd[(size_t)g] != 0;
                row[(size_t)g] = boundary ? mt_iou_min(inter[at], ad, gt_area[q.g0 + g], inter_b[at], det_area_b[q.d0 + d], gt_area_b[q.g0 + g], c)
                                          : mt_iou(inter[at], ad, gt_area[q.g0 + g], c);
            }
            for (int inst = 0; inst < AT; ++inst) {
                const int a = inst / T, t = inst % T;
                const int m = mt_pick(row.data(), q.G, ign.data(), crowd.data(), a, mt_threshold(iou_thrs[t]), taken.data() + inst, AT);
                const int64_t at = (int64_t)a * T + t;
                bool ig;
                if (m >= 0) {
                    taken[(size_t)(m >> 5) * AT + inst] |= 1u << (m & 31);
                    gt_match[at * NG + q.g0 + m] = q.d0 + d;
                    ig = (ign[(size_t)m] >> a) & 1;
                } else {
                    ig = (double)ad < area_rngs[2 * a] || (double)ad > area_rngs[2 * a + 1];
                }
                dt_match[at * ND + q.d0 + r] = m >= 0 ? q.g0 + m : -1;
                dt_ignore[at * ND + q.d0 + r] = ig ? 1 : 0;
            }
        }
    }
    return 0;
}

}  // namespace

extern "C" {

int cvlm_coco_match(const int32_t* det_offsets, const int32_t* gt_offsets, const int64_t* pair_offsets, int32_t E, const int32_t* inter,
                    int64_t N, const int32_t* det_area, const float* score, int32_t ND, const int32_t* gt_area, const double* gt_range_area,
                    const uint8_t* gt_crowd, int32_t NG, const double* iou_thrs, int32_t T, const double* area_rngs, int32_t A,
                    int32_t max_det, int32_t* dt_order, int32_t* dt_match, uint8_t* dt_ignore, int32_t* gt_match, uint8_t* gt_ignore,
                    int32_t* status, void* stream) {
    if (mt_bad(det_offsets, gt_offsets, pair_offsets, E, inter, N, det_area, score, ND, gt_area, gt_range_area, gt_crowd, NG, iou_thrs, T,
               area_rngs, A, max_det, dt_order, dt_match, dt_ignore, gt_match, gt_ignore, status))
        return CVLM_E_BADARG;
    return mt_launch<false>(det_offsets, gt_offsets, pair_offsets, E, inter, N, det_area, score, ND, gt_area, gt_range_area, gt_crowd, NG,
                            iou_thrs, T, area_rngs, A, max_det, dt_order, dt_match, dt_ignore, gt_match, gt_ignore, status, nullptr, nullptr,
                            nullptr, (hipStream_t)stream);
}

int cvlm_debug_coco_match_host(const int32_t* det_offsets, const int32_t* gt_offsets, const int64_t* pair_offsets, int32_t E,
                               const int32_t* inter, int64_t N, const int32_t* det_area, const float* score, int32_t ND,
                               const int32_t* gt_area, const double* gt_range_area, const uint8_t* gt_crowd, int32_t NG,
                               const double* iou_thrs, int32_t T, const double* area_rngs, int32_t A, int32_t max_det, int32_t* dt_order,
                               int32_t* dt_match, uint8_t* dt_ignore, int32_t* gt_match, uint8_t* gt_ignore, int32_t* status) {
    if (mt_bad(det_offsets, gt_offsets, pair_offsets, E, inter, N, det_area, score, ND, gt_area, gt_range_area, gt_crowd, NG, iou_thrs, T,
               area_rngs, A, max_det, dt_order, dt_match, dt_ignore, gt_match, gt_ignore, status))
        return CVLM_E_BADARG;
    return mt_host(det_offsets, gt_offsets, pair_offsets, E, inter, N, det_area, score, ND, gt_area, gt_range_area, gt_crowd, NG, iou_thrs, T,
                   area_rngs, A, max_det, dt_order, dt_match, dt_ignore, gt_match, gt_ignore, status, false, nullptr, nullptr, nullptr);
}

// The boundary matching: the same two launches, the matching kernel in its form that divides twice per pair
int cvlm_coco_match_boundary(const int32_t* det_offsets, const int32_t* gt_offsets, const int64_t* pair_offsets, int32_t E,
                             const int32_t* inter, int64_t N, const int32_t* det_area, const float* score, int32_t ND, const int32_t* gt_area,
                             const double* gt_range_area, const uint8_t* gt_crowd, int32_t NG, const double* iou_thrs, int32_t T,
                             const double* area_rngs, int32_t A, int32_t max_det, const int32_t* inter_b, const int32_t* det_area_b,
                             const int32_t* gt_area_b, int32_t* dt_order, int32_t* dt_match, uint8_t* dt_ignore, int32_t* gt_match,
                             uint8_t* gt_ignore, int32_t* status, void* stream) {
    if (mt_bad(det_offsets, gt_offsets, pair_offsets, E, inter, N, det_area, score, ND, gt_area, gt_range_area, gt_crowd, NG, iou_thrs, T,
               area_rngs, A, max_det, dt_order, dt_match, dt_ignore, gt_match, gt_ignore, status) ||
        mt_bad_boundary(inter_b, N, det_area_b, ND, gt_area_b, NG))
        return CVLM_E_BADARG;
    return mt_launch<true>(det_offsets, gt_offsets, pair_offsets, E, inter, N, det_area, score, ND, gt_area, gt_range_area, gt_crowd, NG,
                           iou_thrs, T, area_rngs, A, max_det, dt_order, dt_match, dt_ignore, gt_match, gt_ignore, status, inter_b, det_area_b,
                           gt_area_b, (hipStream_t)stream);
}

int cvlm_debug_coco_match_boundary_host(const int32_t* det_offsets, const int32_t* gt_offsets, const int64_t* pair_offsets, int32_t E,
                                        const int32_t* inter, int64_t N, const int32_t* det_area, const float* score, int32_t ND,
                                        const int32_t* gt_area, const double* gt_range_area, const uint8_t* gt_crowd, int32_t NG,
                                        const double* iou_thrs, int32_t T, const double* area_rngs, int32_t A, int32_t max_det,
                                        const int32_t* inter_b, const int32_t* det_area_b, const int32_t* gt_area_b, int32_t* dt_order,
                                        int32_t* dt_match, uint8_t* dt_ignore, int32_t* gt_match, uint8_t* gt_ignore, int32_t* status) {
    if (mt_bad(det_offsets, gt_offsets, pair_offsets, E, inter, N, det_area, score, ND, gt_area, gt_range_area, gt_crowd, NG, iou_thrs, T,
               area_rngs, A, max_det, dt_order, dt_match, dt_ignore, gt_match, gt_ignore, status) ||
        mt_bad_boundary(inter_b, N, det_area_b, ND, gt_area_b, NG))
        return CVLM_E_BADARG;
    return mt_host(det_offsets, gt_offsets, pair_offsets, E, inter, N, det_area, score, ND, gt_area, gt_range_area, gt_crowd, NG, iou_thrs, T,
                   area_rngs, A, max_det, dt_order, dt_match, dt_ignore, gt_match, gt_ignore, status, true, inter_b, det_area_b, gt_area_b);
}

}  // extern "C"
