// Ramer-Douglas-Peucker on closed rings in exact integers: the key of a vertex under a chord, the keep test and the
// anchor rule of cvlm_contour_simplify_mark / cvlm_contour_simplify_emit, written once for the device kernels (simplify.hip) and for the
// sequential host entry cvlm_debug_contour_simplify_host.  No HIP call, no allocation.
//
// A ring v_0 .. v_(n-1) is opened into the polyline v_0 .. v_(n-1), v_0; the kept set starts as {v_0, the vertex farthest from v_0 (the
// smallest index on a tie), the closing v_0}.  Under the chord (i, j) a vertex v, i < v < j, has the squared distance to the SEGMENT
// P_i P_j as the numerator `num` over the chord's common denominator L; the vertex with the largest num (the smallest index on a tie)
// is kept iff 16 num > T^2 L, T the tolerance in quarter pixels, and the two halves are split in turn.
#pragma once
#include <stdint.h>

#include "contour_logic.h"

#define SP_HD CC_HD

constexpr int SP_MAX_T = 65535;                                       // quarter pixels: 16383.75 px
constexpr int SP_NONE = 0x7fffffff;                                   // best index of a chord that no vertex has bid for
constexpr int SP_FINAL = -1;                                          // best index of a chord that did not split: its vertices rest

struct sp_pt { int x, y; };

// one vertex as contour.hip's ct_pack_xy stores it
SP_HD sp_pt sp_unpack(uint32_t w) {
    sp_pt p;
    p.x = (int16_t)(w & 0xffffu); p.y = (int16_t)(w >> 16);
    return p;
}

SP_HD uint64_t sp_d2(sp_pt a, sp_pt b) {
    const int64_t dx = (int64_t)a.x - b.x, dy = (int64_t)a.y - b.y;
    return (uint64_t)(dx * dx + dy * dy);
}

// The numerator of v's squared distance to the segment (i, j) -> num, with *L the denominator of the chord.  Coordinates in
// [0, 16384]: |.|^2 <= 2^29, num <= 2^58.  Others wrap in uint64 -- the same on the host and on the device.
SP_HD uint64_t sp_key(sp_pt i, sp_pt j, sp_pt v, uint64_t* L) {
    if (i.x == j.x && i.y == j.y) {                                   // a ring that passes through one point twice
        *L = 1;
        return sp_d2(v, i);
    }
    const int64_t cx = (int64_t)j.x - i.x, cy = (int64_t)j.y - i.y, vx = (int64_t)v.x - i.x, vy = (int64_t)v.y - i.y;
    const int64_t len = cx * cx + cy * cy, t = vx * cx + vy * cy;
    *L = (uint64_t)len;
    if (t <= 0) return sp_d2(v, i) * (uint64_t)len;
    if (t >= len) return sp_d2(v, j) * (uint64_t)len;
    const int64_t cross = cx * vy - cy * vx;
    return (uint64_t)cross * (uint64_t)cross;
}

// the farthest vertex of a chord is kept: it lies more than T / 4 from the segment
SP_HD bool sp_keeps(uint64_t num, uint64_t L, int T) { return 16u * num > (uint64_t)T * (uint64_t)T * L; }

// the order of the bids under one chord, and of the distances to v_0 for the anchor B: the larger key, then the smaller index
SP_HD bool sp_beats(uint64_t num, int idx, uint64_t best_num, int best_idx) { return num > best_num || (num == best_num && idx < best_idx); }

SP_HD bool sp_tolerance_ok(int T) { return T >= 0 && T <= SP_MAX_T; }

// ring_start of the output: 1 on an outer ring's first vertex, 2 on a hole's.  An outer ring's first edge heads east -- the second
// vertex of the INPUT ring has its start's y --, a hole's heads south.
SP_HD uint8_t sp_ring_code(sp_pt start, sp_pt second) { return second.y == start.y ? 1 : 2; }

// index j of a plane of cnt vertices closes a ring: the next ring's start or the end of the slice, whose coordinates are the ring's v_0
SP_HD bool sp_closes(const uint8_t* ring_start, int j, int cnt) { return j >= cnt || ring_start[j] != 0; }
