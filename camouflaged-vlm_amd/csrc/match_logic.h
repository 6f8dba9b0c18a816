// COCO matching on the device: the per-thread logic of cvlm_coco_match, written once for the device kernel (match.hip)
// and for the sequential host entry cvlm_debug_coco_match_host, which runs these same functions on the CPU.  No HIP call, no allocation.
//
// A GROUP is one (image, category) pair with D detections and G annotations; its intersections are a D x G block, detection-major.  The
// published loop of COCOeval.evaluateImg walks the annotations sorted ignore-last and keeps the last one that is at least as good as
// the best so far; §22 shows that this is the choice below, which needs no sort of the annotations:
//   - mt_group_ok:    what is checked before anything of a group is read or stored;
//   - mt_precedes:    the order of two detections: score descending, NaN last, equal scores in the caller's order;
//   - mt_iou:         rleIou's quotient from integers, one correctly rounded double division;
//   - mt_iou_min:     the smaller of the mask's and the boundary's IoU of a pair, two such divisions;
//   - mt_ignore_mask: bit a of an annotation's byte = it is ignored in area range a;
//   - mt_pick:        the annotation one detection takes in one (area range, threshold) instance, or -1.
#pragma once
#include <stdint.h>

#include "maskbits.h"

#define MT_HD CC_HD

constexpr int MT_CAP = 1024;       // detections, and annotations, of one group
constexpr int MT_MAX_T = 16;       // IoU thresholds
constexpr int MT_MAX_A = 8;        // area ranges: one bit each of an annotation's ignore byte
constexpr int MT_MAX_ROWS = 1 << 20;

struct mt_group {
    int d0, D, g0, G;
    int64_t p0;
};

// Group e of the three offset tables: forwards, inside the tables, within the cap, and a pair block of exactly D * G inside [0, N)
MT_HD bool mt_group_ok(const int* det_off, const int* gt_off, const int64_t* pair_off, int e, int ND, int NG, int64_t N, mt_group& q) {
    const int d0 = det_off[e], d1 = det_off[e + 1], g0 = gt_off[e], g1 = gt_off[e + 1];
    const int64_t p0 = pair_off[e], p1 = pair_off[e + 1];
    if (d0 < 0 || d1 < d0 || d1 > ND || g0 < 0 || g1 < g0 || g1 > NG) return false;
    if (d1 - d0 > MT_CAP || g1 - g0 > MT_CAP) return false;
    if (p0 < 0 || p1 < p0 || p1 > N || p1 - p0 != (int64_t)(d1 - d0) * (g1 - g0)) return false;
    q.d0 = d0; q.D = d1 - d0; q.g0 = g0; q.G = g1 - g0; q.p0 = p0;
    return true;
}

// Detection j (score sj) comes before detection i (score si): numpy.argsort(-score, kind="mergesort") -- NaN behind every number
MT_HD bool mt_precedes(float sj, int j, float si, int i) {
    const bool nj = sj != sj, ni = si != si;
    if (nj || ni) return nj == ni ? j < i : ni;
    return sj > si || (sj == si && j < i);
}

// IoU of a detection and an annotation from their pixel counts: 0 where nothing is shared, -1 (never matches) for a refused pair and
// for areas that cannot belong to the intersection (a union below 1)
MT_HD double mt_iou(int inter, int area_d, int area_g, bool crowd) {
#pragma clang fp contract(off)
    if (inter < 0) return -1.0;
    if (inter == 0) return 0.0;
    const int64_t u = crowd ? (int64_t)area_d : (int64_t)area_d + area_g - inter;
    if (u < 1) return -1.0;
    return (double)inter / (double)u;
}

// What the boundary matching compares with a threshold (boundary_iou_api's COCOeval, iouType = "boundary"): min(mask IoU, boundary
// IoU), each mt_iou of its own integers under the same crowd flag.  -1 on either side stays -1: no other value is negative.
MT_HD double mt_iou_min(int inter, int area_d, int area_g, int inter_b, int area_d_b, int area_g_b, bool crowd) {
    const double m = mt_iou(inter, area_d, area_g, crowd), b = mt_iou(inter_b, area_d_b, area_g_b, crowd);
    return b < m ? b : m;
}

// Bit a set: the annotation is ignored in area range a (rngs[2 a], rngs[2 a + 1])
MT_HD uint32_t mt_ignore_mask(bool crowd, double range_area, const double* rngs, int A) {
    uint32_t m = 0u;
    for (int a = 0; a < A; ++a)
        if (crowd || range_area < rngs[2 * a] || range_area > rngs[2 * a + 1]) m |= 1u << a;
    return m;
}

MT_HD double mt_threshold(double t) { return t < 1 - 1e-10 ? t : 1 - 1e-10; }

// The annotation that a detection with the IoU row iou[0 .. G) takes in the instance of area range a and threshold thr: among the
// annotations that are not ignored and not taken, the largest IoU >= thr, the largest index on ties; only if there is none, the same
// among the ignored ones, where a crowd annotation can be taken again.  taken: bit g & 31 of taken[(g >> 5) * stride].
MT_HD int mt_pick(const double* iou, int G, const uint8_t* ign, const uint8_t* crowd, int a, double thr, const uint32_t* taken, int stride) {
    double best0 = thr, best1 = thr;
    int m0 = -1, m1 = -1;
    for (int g = 0; g < G; ++g) {
        if (((taken[(g >> 5) * stride] >> (g & 31)) & 1u) && !crowd[g]) continue;
        const double v = iou[g];
        if ((ign[g] >> a) & 1) {
            if (v >= best1) { best1 = v; m1 = g; }
        } else if (v >= best0) {
            best0 = v; m0 = g;
        }
    }
    return m0 >= 0 ? m0 : m1;
}
