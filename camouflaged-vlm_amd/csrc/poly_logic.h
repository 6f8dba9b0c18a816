// COCO polygon annotations on the device: the per-thread logic of cvlm_mask_poly_decode, written once for the device
// kernels (gt.hip) and for the sequential host entry cvlm_debug_mask_poly_decode_host, which runs these same functions on the CPU.  No
// HIP call, no allocation.
//
// The definition is the published maskApi.c's rleFrPoly, restated in §21: the vertices are scaled by 5 and rounded, every edge is
// walked along its longer axis, and wherever the walk changes its column u, the pair of points gives one BOUNDARY position x h + y of
// the plane's column-major stream -- §20's stream (gt_logic.h): toggle, prefix XOR, transpose.
//   - pl_slice_ok, pl_coord_ok, pl_polys_ok: what is checked of a polygon and of a plane's list before anything is walked;
//   - pl_scale: a coordinate -> the scaled integer (floating point, one product and one sum, each rounded on its own);
//   - pl_edge_of: an edge's end points, flipped as the walk wants them, and its point count max(dx, dy) + 1;
//   - pl_point: point d of an edge -- the one floating-point function of the walk: one quotient, one product, two sums, each one IEEE
//     double operation rounded on its own (no contraction into an fma: the pragma holds on the host and on the device);
//   - pl_candidate: the boundary position of a pair of consecutive points, in integers.
//
// pl_candidate in integers.  The definition forms xd = ((double)um + 0.5) / 5.0 - 0.5 for the integer um = (u < u' ? u : u - 1), |um| <
// 2^20, and keeps the pair iff floor(xd) == xd and 0 <= xd <= w - 1.  um + 0.5 is exact.  For um = 5 q + 2 the quotient is q + 0.5
// exactly, so the correctly rounded division returns it and xd = q exactly.  For every other um the real value lies 0.2 or more from
// an integer and the two roundings move it by less than 2^-30: it is no integer.  So the pair is kept iff um mod 5 == 2 (um - 2
// divisible by 5) and 0 <= q <= w - 1, q = (um - 2) / 5.  Likewise yd = ((double)vm + 0.5) / 5.0 - 0.5 with vm = min(v, v'), clamped to
// [0, h] and rounded up: the real value is (vm - 2) / 5, exact where it is an integer and at least 0.2 from one elsewhere, and the
// clamp's bounds are integers, so ceil(clamp(yd)) = clamp(ceil((vm - 2) / 5)) in integers.
#pragma once
#include <stdint.h>

#include "gt_logic.h"

#define PL_HD GT_HD

constexpr double PL_MAX_COORD = 65536.0;                              // |c| of every coordinate; the scaled integers stay below 2^19
constexpr int PL_MIN_VERTS = 3, PL_MAX_VERTS = 65535;                 // vertices of a polygon
constexpr int64_t PL_MAX_POINTS = (int64_t)1 << 24;                   // walk points of a polygon, counted in 64 bits before any is walked
constexpr int PL_MAX_POLYS = 4096;                                    // polygons of a plane

// The polygon's doubles are xy[off, end): forwards, inside xy[0, total), an even number of them, 3 .. 65535 vertices
PL_HD bool pl_slice_ok(int64_t off, int64_t end, int64_t total) {
    if (off < 0 || off >= end || end > total) return false;
    const int64_t n = end - off;
    return (n & 1) == 0 && n >= 2 * PL_MIN_VERTS && n <= 2 * PL_MAX_VERTS;
}

// Finite and inside the bound: false for a NaN, which fails both compares
PL_HD bool pl_coord_ok(double c) { return c >= -PL_MAX_COORD && c <= PL_MAX_COORD; }

// The plane's polygons are [q0, q1) of the call's Q: 1 .. 4096 of them
PL_HD bool pl_polys_ok(int q0, int q1, int Q) { return q0 >= 0 && q1 <= Q && q1 - q0 >= 1 && q1 - q0 <= PL_MAX_POLYS; }

// (int)(5.0 * c + 0.5) for a coordinate that passed pl_coord_ok: the value fits an int, the conversion truncates toward zero
PL_HD int pl_scale(double c) {
#pragma clang fp contract(off)
    const double m = 5.0 * c;
    return (int)(m + 0.5);
}

struct pl_edge { int xs, ys, xe, ye, dx, dy, n; bool flip; };        // the end points after the flip's swap; n: points of the edge

// Edge from (xs, ys) to (xe, ye), scaled integers
PL_HD pl_edge pl_edge_of(int xs, int ys, int xe, int ye) {
    pl_edge e;
    e.dx = xe > xs ? xe - xs : xs - xe;
    e.dy = ye > ys ? ye - ys : ys - ye;
    e.flip = (e.dx >= e.dy && xs > xe) || (e.dx < e.dy && ys > ye);
    e.xs = e.flip ? xe : xs; e.ys = e.flip ? ye : ys;
    e.xe = e.flip ? xs : xe; e.ye = e.flip ? ys : ye;
    e.n = (e.dx >= e.dy ? e.dx : e.dy) + 1;
    return e;
}

// Point d of the edge, 0 <= d < e.n.  An edge of no length (a repeated vertex) is its one point, without a division.
PL_HD void pl_point(const pl_edge& e, int d, int& u, int& v) {
#pragma clang fp contract(off)
    if (e.dx == 0 && e.dy == 0) { u = e.xs; v = e.ys; return; }
    if (e.dx >= e.dy) {
        const double s = (double)(e.ye - e.ys) / (double)e.dx;
        const int t = e.flip ? e.dx - d : d;
        const double m = s * (double)t;
        const double a = (double)e.ys + m;
        u = t + e.xs;
        v = (int)(a + 0.5);
    } else {
        const double s = (double)(e.xe - e.xs) / (double)e.dy;
        const int t = e.flip ? e.dy - d : d;
        const double m = s * (double)t;
        const double a = (double)e.xs + m;
        v = t + e.ys;
        u = (int)(a + 0.5);
    }
}

// floor(a / 5) and whether 5 divides a, for any int a
PL_HD int pl_floor5(int a, bool& exact) {
    int q = a / 5;
    const int r = a - 5 * q;
    if (r < 0) --q;
    exact = r == 0;
    return q;
}

// Consecutive points (up, vp), (u, v) of a polygon's sequence on a plane of h x w -> true and the boundary position e = x h + y, 0 <= e
// <= h w (y = h is legal: the first pixel of the next column, or h w, which is no pixel's); false: the pair gives no boundary.
PL_HD bool pl_candidate(int up, int vp, int u, int v, int h, int w, int64_t& e) {
    if (u == up) return false;
    bool exact;
    const int x = pl_floor5((u < up ? u : u - 1) - 2, exact);
    if (!exact || x < 0 || x > w - 1) return false;
    int y = pl_floor5((v < vp ? v : vp) - 2, exact);
    if (!exact) ++y;                                                  // the ceiling
    y = y < 0 ? 0 : y > h ? h : y;
    e = (int64_t)x * h + y;
    return true;
}
