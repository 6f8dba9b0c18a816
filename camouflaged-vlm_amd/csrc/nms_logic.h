// Mask NMS on the device: the per-thread logic of cvlm_mask_nms_inter and cvlm_mask_nms, written once for the device
// kernels (nms.hip) and for the sequential host entries cvlm_debug_mask_nms_inter_host / cvlm_debug_mask_nms_host, which run these same
// functions on the CPU.  No HIP call, no allocation.  Integers, and doubles under fp contract(off) where §30 says so.
//
// A GROUP is the instances of one image: rows member[m0 .. m0 + D) of a table of Q sized planes, D <= 1024.  Its intersections are the
// strict upper triangle of D x D, row-major: pair (i, j), i < j in member order, at i D - i (i + 1) / 2 + (j - i - 1).
//   - nm_group_span, nm_member_ok: what is checked before anything of a group is read or stored;
//   - nm_pair_at, nm_pair_of:      the place of a pair in the triangle and back;
//   - nm_pair_ok:                  the check of a pair of planes and of their boxes;
//   - nm_window_of, nm_word:       the words the two boxes share and the set pixels of one of them inside the shared columns;
//   - nm_measure:                  IoU (mt_iou's arithmetic) or intersection over the smaller area, 0 across categories;
//   - nm_linear_term, nm_gauss_arg: one (i, j) term of Matrix NMS (Wang et al., SOLOv2, §3.3).
// The order of a group is match_logic.h's mt_precedes.
#pragma once
#include <math.h>
#include <stdint.h>

#include "match_logic.h"
#include "sized_logic.h"

#define NM_HD CC_HD

constexpr int NM_CAP = MT_CAP;                     // instances of one group
constexpr int NM_MAX_ROWS = 1 << 20;               // Q and G of a call
constexpr int64_t NM_MAX_PAIRS = (int64_t)1 << 22; // N of a call

enum { NM_IOU = 0, NM_MIN = 1 };                   // measure
enum { NM_GREEDY = 0, NM_LINEAR = 1, NM_GAUSS = 2 };   // method
enum { NM_PAIR_REFUSED = 1, NM_GROUP_REFUSED = 2 };    // status bits

struct nm_group {
    int m0, D;
    int64_t p0;
};

// Group g of the two offset tables: forwards, inside member[0, Q), within the cap, and a pair block of exactly the triangle inside [0, N]
NM_HD bool nm_group_span(const int* group_off, const int64_t* pair_off, int g, int Q, int64_t N, nm_group& q) {
    const int m0 = group_off[g], m1 = group_off[g + 1];
    const int64_t p0 = pair_off[g], p1 = pair_off[g + 1];
    if (m0 < 0 || m1 < m0 || m1 > Q || m1 - m0 > NM_CAP) return false;
    const int D = m1 - m0;
    if (p0 < 0 || p1 < p0 || p1 > N || p1 - p0 != (int64_t)D * (D - 1) / 2) return false;
    q.m0 = m0; q.D = D; q.p0 = p0;
    return true;
}
NM_HD bool nm_member_ok(int row, int Q) { return row >= 0 && row < Q; }

NM_HD int64_t nm_row_start(int i, int D) { return (int64_t)i * D - (int64_t)i * (i + 1) / 2; }
NM_HD int64_t nm_pair_at(int i, int j, int D) { return nm_row_start(i, D) + (j - i - 1); }                 // i < j
// The pair at place t of the triangle, 0 <= t < D (D - 1) / 2: the root of the quadratic as a first guess, then exact in integers
NM_HD void nm_pair_of(int64_t t, int D, int& i, int& j) {
    const double b = 2.0 * D - 1.0;
    int r = (int)((b - sqrt(b * b - 8.0 * (double)t)) * 0.5);
    r = r < 0 ? 0 : (r > D - 2 ? D - 2 : r);
    while (r < D - 2 && nm_row_start(r + 1, D) <= t) ++r;
    while (r > 0 && nm_row_start(r, D) > t) --r;
    i = r;
    j = r + 1 + (int)(t - nm_row_start(r, D));
}

// ---- intersections inside the boxes -----------------------------------------------------------------------------------------------------
NM_HD bool nm_box_empty(const int* b) { return b[0] == -1 && b[1] == -1 && b[2] == -1 && b[3] == -1; }
// the empty box, or corners in order inside [0, w) x [0, h)
NM_HD bool nm_box_ok(const int* b, int h, int w) {
    if (nm_box_empty(b)) return true;
    return b[0] >= 0 && b[0] <= b[2] && b[2] < w && b[1] >= 0 && b[1] <= b[3] && b[3] < h;
}
// Rows a and b of one table: both planes pass §19's check, equal sizes, boxes that are boxes of that size
NM_HD bool nm_pair_ok(int a, int b, const int* dims, const int64_t* off, int64_t nbytes, const int* box) {
    const int h = dims[2 * a], w = dims[2 * a + 1];
    if (h != dims[2 * b] || w != dims[2 * b + 1]) return false;
    if (!sz_plane_ok(h, w, off[a], off[a + 1], nbytes) || !sz_plane_ok(h, w, off[b], off[b + 1], nbytes)) return false;
    return nm_box_ok(box + 4 * a, h, w) && nm_box_ok(box + 4 * b, h, w);
}

// What two boxes share: rows y0 .. y0 + rows - 1, word columns c0 .. c0 + cols - 1, pixel columns x0 .. x1.  rows = 0: nothing --
// an empty box, an instance without pixels, or boxes that do not meet -- and no word of either plane is read.
struct nm_window { int y0, rows, c0, cols, x0, x1; };
NM_HD nm_window nm_window_of(const int* a, int area_a, const int* b, int area_b) {
    nm_window v = {0, 0, 0, 0, 0, -1};
    if (area_a < 1 || area_b < 1 || nm_box_empty(a) || nm_box_empty(b)) return v;
    const int x0 = a[0] > b[0] ? a[0] : b[0], y0 = a[1] > b[1] ? a[1] : b[1];
    const int x1 = a[2] < b[2] ? a[2] : b[2], y1 = a[3] < b[3] ? a[3] : b[3];
    if (x0 > x1 || y0 > y1) return v;
    v.y0 = y0; v.rows = y1 - y0 + 1; v.c0 = x0 >> 5; v.cols = (x1 >> 5) - v.c0 + 1; v.x0 = x0; v.x1 = x1;
    return v;
}
// Bits of the unpacked word of word column c that are pixel columns x0 .. x1; c0 <= c <= c1, so at least one
NM_HD uint32_t nm_columns(int c, int x0, int x1) {
    const int lo = x0 - 32 * c > 0 ? x0 - 32 * c : 0, hi = x1 - 32 * c < 31 ? x1 - 32 * c : 31;
    const uint32_t upto = hi == 31 ? 0xffffffffu : (1u << (hi + 1)) - 1u;
    return upto & ~((1u << lo) - 1u);
}
// Set pixels of stored words x AND y of word column c inside the pixel columns x0 .. x1
NM_HD int nm_word(uint32_t x, uint32_t y, int c, int x0, int x1) { return __builtin_popcount(x & y & cc_pack(nm_columns(c, x0, x1))); }

// ---- the measure and the Matrix NMS terms ----------------------------------------------------------------------------------------------
// m(i, j): 0 where nothing is shared or the categories differ, -1 (never above a threshold) for a refused pair and for areas that
// cannot belong to the intersection
NM_HD double nm_measure(int inter, int area_i, int area_j, int measure, bool same_category) {
#pragma clang fp contract(off)
    if (!same_category) return 0.0;
    if (measure == NM_IOU) return mt_iou(inter, area_i, area_j, false);
    if (inter < 0) return -1.0;
    if (inter == 0) return 0.0;
    const int s = area_i < area_j ? area_i : area_j;
    if (s < 1) return -1.0;
    return (double)inter / (double)s;
}
// Matrix NMS takes a negative measure as 0: a refused pair decays nothing
NM_HD double nm_clamp(double m) { return m < 0.0 ? 0.0 : m; }
// (1 - m_ij) / (1 - c_i); 1 where 1 - c_i == 0 -- such an i is itself decayed to 0 by its duplicate, which decays j directly
NM_HD double nm_linear_term(double m, double c) {
#pragma clang fp contract(off)
    const double d = 1.0 - c;
    return d == 0.0 ? 1.0 : (1.0 - m) / d;
}
// m_ij^2 - c_i^2: decay_j = min_i exp(-sigma x_i) = exp(-sigma max_i x_i)
NM_HD double nm_gauss_arg(double m, double c) {
#pragma clang fp contract(off)
    const double mm = m * m, cc = c * c;
    return mm - cc;
}
NM_HD double nm_gauss_decay(double sigma, double x) {
#pragma clang fp contract(off)
    const double a = sigma * x;
    return exp(-a);
}
