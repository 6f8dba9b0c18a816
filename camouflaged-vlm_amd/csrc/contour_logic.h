// Crack contours of sized planes: the per-thread logic of cvlm_mask_contour_count / cvlm_mask_contour_emit, written once
// for the device kernels (contour.hip) and for the sequential host entry cvlm_debug_mask_contour_host.  No HIP call, no allocation.
//
// The LATTICE of an h x w plane has the points (i, j), 0 <= i <= h, 0 <= j <= w; point (i, j) is the corner shared by the pixels
// NW = (i - 1, j - 1), NE = (i - 1, j), SW = (i, j - 1), SE = (i, j), a pixel outside the plane read as clear.  A lattice row is
// ct_lattice_words(w) = w / 32 + 1 words, bit j & 31 of word j >> 5 = point j.  Four bit maps describe every point:
//   any   the ring turns here: an odd number of the four pixels is set (one vertex) or they are a diagonal pair (two vertices);
//   two   the diagonal pairs.  Their two vertices are the WEST one (the end of the horizontal segment that arrives from the left, the
//         first in row-major order) and the EAST one;
//   up    one vertex: its vertical segment leaves upwards.  Two vertices: the west one's does, and the east one's leaves downwards;
//         clear: the other way round.  This is where the connectivity enters: 8 turns left at a diagonal point, 4 turns right;
//   hout  the edge that LEAVES the vertex (foreground on its right) is the horizontal one; at a diagonal point that holds for both
//         vertices or for neither.
// The vertices of a lattice row pair up consecutively into horizontal segments and those of a lattice column into vertical ones, so
// with the DENSE index of a vertex -- its row-major rank, the two of a diagonal point west first -- the horizontal partner is index ^ 1
// (a row holds an even number) and the vertical partner is the next marked point up or down the column.
#pragma once
#include <stdint.h>

#include "maskbits.h"
#include "sized_logic.h"

#define CT_HD CC_HD

constexpr int CT_MAX_VERTS = 1 << 22;                                 // vertices of a plane; one beyond it is refused
constexpr int CT_MAX_ROUNDS = 24;                                     // doublings of the rank pass: 2^24 passes every ring
constexpr int CT_RING_ARRAYS = 7;                                     // succ, and two copies each of next, leader, distance
constexpr int CT_MAPS = 5;                                            // any, two, up, hout and the prefix table

CT_HD int ct_lattice_words(int w) { return (w >> 5) + 1; }
// words of one map of a plane of at most max_words = h * ceil(w / 32) words: (h + 1) (ws + 1) <= 2 h ws + 2
CT_HD int64_t ct_map_stride(int64_t max_words) { return 2 * max_words + 2; }

// pixel word c of a row, unpacked; clear beyond the row's words, at its pad bits and for a row outside the plane (row == nullptr)
CT_HD uint32_t ct_row_word(const uint32_t* row, int c, int ws, int w) {
    if (!row || c < 0 || c >= ws) return 0u;
    const uint32_t v = cc_unpack(row[c]);
    const int valid = w - 32 * c;
    return valid >= 32 ? v : v & ((1u << valid) - 1u);
}

struct ct_corner { uint32_t any, two, up, hout; };

// lattice word c of the lattice row between the pixel rows `above` and `below`
CT_HD ct_corner ct_corners(const uint32_t* above, const uint32_t* below, int c, int ws, int w, int connectivity) {
    const uint32_t ne = ct_row_word(above, c, ws, w), se = ct_row_word(below, c, ws, w);
    const uint32_t nw = (ne << 1) | (ct_row_word(above, c - 1, ws, w) >> 31);
    const uint32_t sw = (se << 1) | (ct_row_word(below, c - 1, ws, w) >> 31);
    const uint32_t odd = nw ^ ne ^ sw ^ se;
    const uint32_t main_diag = nw & se & ~ne & ~sw, anti_diag = ne & sw & ~nw & ~se;
    ct_corner q;
    q.two = main_diag | anti_diag;
    q.any = odd | q.two;
    // main diagonal: edges arrive from above and below and leave west and east.  8 joins the arrival from above to the departure
    // east, so the west vertex hangs below; 4 joins it to the departure west.  Anti-diagonal: the mirror image.
    q.up = (odd & (nw ^ ne)) | (connectivity == 8 ? anti_diag : main_diag);
    q.hout = q.any & ((se & ~ne) | (nw & ~sw));
    return q;
}

CT_HD int ct_popc(uint32_t v) { return __builtin_popcount(v); }
CT_HD int ct_vertices(const ct_corner& q) { return ct_popc(q.any) + ct_popc(q.two); }

// the maps of one plane: rows = h + 1 lattice rows of lw words each; table[k]: the vertices before word k in row-major order
struct ct_maps { const uint32_t *any, *two, *up, *hout; const int* table; int rows, lw; };

// dense index of the (west) vertex at bit `bit` of lattice word k
CT_HD int ct_dense(const ct_maps& m, int k, int bit) {
    const uint32_t low = (1u << bit) - 1u;
    return m.table[k] + ct_popc(m.any[k] & low) + ct_popc(m.two[k] & low);
}

// The successor of vertex v = slot `east` (0 / 1) of the marked point at bit `bit` of word c of lattice row i.  A column walk that
// finds no partner -- maps that are no contour's -- answers v itself.
CT_HD int ct_succ(const ct_maps& m, int i, int c, int bit, int east, int v) {
    const int k = i * m.lw + c;
    const uint32_t b = 1u << bit;
    if (m.hout[k] & b) return v ^ 1;
    const bool is_two = (m.two[k] & b) != 0u;
    const bool up = ((m.up[k] & b) != 0u) != (is_two && east);
    const int step = up ? -1 : 1;
    for (int r = i + step; r >= 0 && r < m.rows; r += step) {
        const int t = r * m.lw + c;
        if (!(m.any[t] & b)) continue;
        int slot = 0;
        if (m.two[t] & b) {                                           // walking up we arrive from below: the vertex that hangs below
            const bool west_up = (m.up[t] & b) != 0u;
            slot = up ? (west_up ? 1 : 0) : (west_up ? 0 : 1);
        }
        return ct_dense(m, t, bit) + slot;
    }
    return v;
}

// one vertex as it is stored: int16 x at the lower address, then int16 y
CT_HD uint32_t ct_pack_xy(int x, int y) { return (uint32_t)(x & 0xffff) | ((uint32_t)(y & 0xffff) << 16); }

// The slice [v0, v1) of a plane in the vertex tables of `total` entries, and its place in the ring arrays of a call whose first plane's
// slice starts at first: 0 <= v0 <= v1 <= total, at most CT_MAX_VERTS long, inside the call's round_vertices
CT_HD bool ct_slice_ok(int64_t v0, int64_t v1, int64_t total) { return v0 >= 0 && v1 >= v0 && v1 <= total && v1 - v0 <= CT_MAX_VERTS; }
CT_HD bool ct_ring_ok(int64_t v0, int64_t v1, int64_t first, int64_t round_vertices) { return v0 >= first && v1 - first <= round_vertices; }
// the maps of the plane fit the stride of the call
CT_HD bool ct_maps_ok(int h, int w, int64_t map_stride) { return (int64_t)(h + 1) * ct_lattice_words(w) <= map_stride; }

// Where vertex v of a ring lands: its ring's first slot + its rank.  dist: the steps from v forwards to the leader, len: the ring's length
CT_HD int ct_rank(int dist, int len) { return dist == 0 ? 0 : len - dist; }
