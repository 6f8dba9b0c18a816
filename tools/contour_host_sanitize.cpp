// Stand-alone check of cvlm_debug_mask_contour_host for a host sanitizer: the entry's maps and successors are the
// kernels' (csrc/contour_logic.h), so their indexing is what runs on the device.  Every buffer is a heap block of exactly the size the
// interface states, so that AddressSanitizer sees any access beyond it.  The rings are held against what defines them: closed,
// alternating horizontal and vertical segments, starts in ascending (y, x), signed areas that sum to the popcount, and the even-odd
// fill of all rings is the plane, bit for bit.  Ragged sizes, both connectivities, refused planes at the first, a middle and the last
// position, a vertex table one short, and every CVLM_E_BADARG.
// Build and run on the CPU, from the repository root:
//   hipcc -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/contour_host_sanitize.cpp camouflaged-vlm_amd/csrc/contour.hip -o /tmp/contour_host_sanitize && /tmp/contour_host_sanitize
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../include/cvlm.h"

namespace {

uint32_t rng_state = 2026u;
uint32_t rng() { return rng_state = rng_state * 1664525u + 1013904223u; }

bool pixel(const uint8_t* plane, int ws, int y, int x) { return (plane[(int64_t)y * 4 * ws + (x >> 3)] >> (7 - (x & 7))) & 1; }

enum Refusal { NONE, SHORT_SLICE, ODD_OFFSET, PAST_THE_END, HEIGHT_ZERO, WIDTH_HUGE, VERTEX_SHORT };

// the rings of one plane against the plane
int check_plane(const uint8_t* plane, int h, int w, const int16_t* xy, const uint8_t* start, int n, const int32_t* n_rings) {
    const int ws = (w + 31) / 32;
    int bad = 0, rings = 0, outer = 0, holes = 0;
    int64_t area2 = 0, popcount = 0;
    std::vector<uint8_t> fill((size_t)h * w, 0);
    int prev_y = -1, prev_x = -1;
    for (int a = 0; a < n;) {
        if (!start[a]) return 1;
        int b = a + 1;
        while (b < n && !start[b]) ++b;
        const int len = b - a;
        if (len < 4 || len % 2) ++bad;
        if (xy[2 * a + 1] < prev_y || (xy[2 * a + 1] == prev_y && xy[2 * a] <= prev_x)) ++bad;      // the starts ascend
        prev_y = xy[2 * a + 1]; prev_x = xy[2 * a];
        int64_t ring2 = 0;
        for (int k = 0; k < len; ++k) {
            const int x0 = xy[2 * (a + k)], y0 = xy[2 * (a + k) + 1];
            const int x1 = xy[2 * (a + (k + 1) % len)], y1 = xy[2 * (a + (k + 1) % len) + 1];
            if (x0 < 0 || x0 > w || y0 < 0 || y0 > h) return 1;
            if ((y0 < prev_y) || (y0 == prev_y && x0 < prev_x)) ++bad;                              // the start is the ring's smallest
            const bool horizontal = y0 == y1 && x0 != x1, vertical = x0 == x1 && y0 != y1;
            if (!horizontal && !vertical) ++bad;
            const bool first_horizontal = xy[2 * a + 1] == xy[2 * (a + 1) + 1];
            if (horizontal != ((k % 2 == 0) == first_horizontal)) ++bad;                            // they alternate
            ring2 += (int64_t)x0 * y1 - (int64_t)x1 * y0;
            if (horizontal)                                                                         // even-odd: toggle everything below
                for (int x = x0 < x1 ? x0 : x1; x < (x0 < x1 ? x1 : x0); ++x)
                    for (int y = y0; y < h; ++y) fill[(size_t)y * w + x] ^= 1;
        }
        if (ring2 > 0) ++outer;
        else ++holes;
        const bool east = xy[2 * (a + 1)] > xy[2 * a] && xy[2 * (a + 1) + 1] == xy[2 * a + 1];
        const bool south = xy[2 * (a + 1) + 1] > xy[2 * a + 1] && xy[2 * (a + 1)] == xy[2 * a];
        if (ring2 > 0 ? !east : !south) ++bad;
        area2 += ring2;
        ++rings;
        a = b;
    }
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            popcount += pixel(plane, ws, y, x);
            bad += fill[(size_t)y * w + x] != (uint8_t)pixel(plane, ws, y, x);
        }
    bad += area2 != 2 * popcount;
    bad += n_rings[0] != outer || n_rings[1] != holes;
    return bad;
}

int check_contours(const std::vector<std::pair<int, int>>& sizes, int density_percent, int connectivity, int bad_plane, Refusal how) {
    const int P = (int)sizes.size();
    int32_t* dims = (int32_t*)malloc(sizeof(int32_t) * 2 * P);
    int64_t* offsets = (int64_t*)malloc(sizeof(int64_t) * (P + 1));
    std::vector<int64_t> true_off((size_t)P + 1, 0);
    for (int p = 0; p < P; ++p) {
        dims[2 * p] = sizes[p].first;
        dims[2 * p + 1] = sizes[p].second;
        true_off[p + 1] = true_off[p] + 4 * (int64_t)sizes[p].first * ((sizes[p].second + 31) / 32);
    }
    const int64_t nbytes = true_off[P];
    for (int p = 0; p <= P; ++p) offsets[p] = true_off[p];
    std::vector<int> refused((size_t)P, 0);
    if (bad_plane >= 0 && how != VERTEX_SHORT) {
        refused[bad_plane] = 1;
        if (how == SHORT_SLICE) { offsets[bad_plane + 1] -= 4; if (bad_plane + 1 < P) refused[bad_plane + 1] = 1; }
        if (how == ODD_OFFSET) { offsets[bad_plane] += 2; if (bad_plane > 0) refused[bad_plane - 1] = 1; }
        if (how == PAST_THE_END) { offsets[P] += 4; refused[bad_plane] = 0; refused[P - 1] = 1; }
        if (how == HEIGHT_ZERO) dims[2 * bad_plane] = 0;
        if (how == WIDTH_HUGE) dims[2 * bad_plane + 1] = 16385;
    }
    uint8_t* bits = (uint8_t*)malloc((size_t)nbytes);
    for (int p = 0; p < P; ++p) {
        const int h = sizes[p].first, w = sizes[p].second, ws = (w + 31) / 32;
        uint8_t* plane = bits + true_off[p];
        for (int64_t i = 0; i < (int64_t)4 * h * ws; ++i) plane[i] = 0;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < 32 * ws; ++x)                          // the pad bits are dirty: they read as clear
                if (x >= w || (int)(rng() >> 8) % 100 < density_percent || (how == VERTEX_SHORT && x + y == 0)) plane[(int64_t)y * 4 * ws + (x >> 3)] |= (uint8_t)(0x80 >> (x & 7));
    }
    int32_t* n_vertices = (int32_t*)malloc(sizeof(int32_t) * P);
    int32_t* status = (int32_t*)malloc(sizeof(int32_t));
    int bad = cvlm_debug_mask_contour_host(bits, nbytes, offsets, dims, P, connectivity, n_vertices, nullptr, nullptr, nullptr, nullptr, 0, status) != 0;
    bool any_refused = false;
    for (int p = 0; p < P; ++p) any_refused |= refused[p] != 0;
    bad += status[0] != (any_refused ? 1 : 0);
    int64_t* vo = (int64_t*)malloc(sizeof(int64_t) * (P + 1));
    vo[0] = 0;
    for (int p = 0; p < P; ++p) {
        bad += refused[p] && n_vertices[p] != 0;
        vo[p + 1] = vo[p] + n_vertices[p] - (how == VERTEX_SHORT && p == bad_plane ? 1 : 0);
    }
    const int64_t total = vo[P];
    int16_t* xy = (int16_t*)malloc(sizeof(int16_t) * 2 * (total ? total : 1));
    uint8_t* start = (uint8_t*)malloc((size_t)(total ? total : 1));
    int32_t* n_rings = (int32_t*)malloc(sizeof(int32_t) * 2 * P);
    int32_t* again = (int32_t*)malloc(sizeof(int32_t) * P);
    bad += cvlm_debug_mask_contour_host(bits, nbytes, offsets, dims, P, connectivity, again, vo, total ? xy : nullptr, total ? start : nullptr,
                                        n_rings, total, status) != 0;
    bad += status[0] != (any_refused || how == VERTEX_SHORT ? 1 : 0);
    for (int p = 0; p < P; ++p) {
        const int n = (int)(vo[p + 1] - vo[p]);
        if (refused[p]) { bad += n != 0 || n_rings[2 * p] != 0 || n_rings[2 * p + 1] != 0; continue; }
        if (how == VERTEX_SHORT && p == bad_plane) {
            for (int t = 0; t < n; ++t) bad += xy[2 * (vo[p] + t)] != 0 || xy[2 * (vo[p] + t) + 1] != 0 || start[vo[p] + t] != 0;
            bad += n_rings[2 * p] != 0 || n_rings[2 * p + 1] != 0;
            continue;
        }
        // dirty pad bits: the checker reads the true columns only
        bad += check_plane(bits + true_off[p], sizes[p].first, sizes[p].second, xy + 2 * vo[p], start + vo[p], n, n_rings + 2 * p);
    }
    free(dims); free(offsets); free(bits); free(n_vertices); free(status); free(vo); free(xy); free(start); free(n_rings); free(again);
    return bad;
}

int check_badargs() {
    const int P = 2;
    int32_t dims[4] = {5, 40, 3, 7};
    int64_t offsets[3] = {0, 40, 52}, vo[3] = {0, 4, 8};
    uint8_t* bits = (uint8_t*)calloc(52, 1);
    int32_t n_vertices[2], n_rings[4], status[1];
    int16_t xy[16];
    uint8_t start[8];
    auto call = [&](const uint8_t* b, int64_t nb, const int64_t* off, const int32_t* d, int p, int c, int32_t* nv, const int64_t* v, int16_t* x,
                    uint8_t* s, int32_t* r, int64_t t, int32_t* st) { return cvlm_debug_mask_contour_host(b, nb, off, d, p, c, nv, v, x, s, r, t, st); };
    int bad = call(bits, 52, offsets, dims, P, 8, n_vertices, vo, xy, start, n_rings, 8, status) != 0;
    bad += call(nullptr, 52, offsets, dims, P, 8, n_vertices, vo, xy, start, n_rings, 8, status) != CVLM_E_BADARG;
    bad += call(bits, 52, nullptr, dims, P, 8, n_vertices, vo, xy, start, n_rings, 8, status) != CVLM_E_BADARG;
    bad += call(bits, 52, offsets, nullptr, P, 8, n_vertices, vo, xy, start, n_rings, 8, status) != CVLM_E_BADARG;
    bad += call(bits, 52, offsets, dims, P, 8, nullptr, vo, xy, start, n_rings, 8, status) != CVLM_E_BADARG;
    bad += call(bits, 52, offsets, dims, P, 8, n_vertices, vo, nullptr, start, n_rings, 8, status) != CVLM_E_BADARG;
    bad += call(bits, 52, offsets, dims, P, 8, n_vertices, vo, xy, nullptr, n_rings, 8, status) != CVLM_E_BADARG;
    bad += call(bits, 52, offsets, dims, P, 8, n_vertices, vo, xy, start, nullptr, 8, status) != CVLM_E_BADARG;
    bad += call(bits, 52, offsets, dims, P, 8, n_vertices, vo, xy, start, n_rings, 8, nullptr) != CVLM_E_BADARG;
    bad += call(bits, 52, offsets, dims, P, 8, n_vertices, nullptr, xy, start, n_rings, 8, status) != CVLM_E_BADARG;
    bad += call(bits + 2, 50, offsets, dims, P, 8, n_vertices, vo, xy, start, n_rings, 8, status) != CVLM_E_BADARG;
    bad += call(bits, 52, offsets, (const int32_t*)((const uint8_t*)dims + 2), P, 8, n_vertices, vo, xy, start, n_rings, 8, status) != CVLM_E_BADARG;
    bad += call(bits, 52, (const int64_t*)((const uint8_t*)offsets + 4), dims, P, 8, n_vertices, vo, xy, start, n_rings, 8, status) != CVLM_E_BADARG;
    bad += call(bits, 52, offsets, dims, P, 8, n_vertices, (const int64_t*)((const uint8_t*)vo + 4), xy, start, n_rings, 8, status) != CVLM_E_BADARG;
    bad += call(bits, 52, offsets, dims, P, 8, n_vertices, vo, xy + 1, start, n_rings, 7, status) != CVLM_E_BADARG;
    bad += call(bits, 52, offsets, dims, 0, 8, n_vertices, vo, xy, start, n_rings, 8, status) != CVLM_E_BADARG;
    bad += call(bits, 52, offsets, dims, 65536, 8, n_vertices, vo, xy, start, n_rings, 8, status) != CVLM_E_BADARG;
    bad += call(bits, 3, offsets, dims, P, 8, n_vertices, vo, xy, start, n_rings, 8, status) != CVLM_E_BADARG;
    bad += call(bits, 52, offsets, dims, P, 6, n_vertices, vo, xy, start, n_rings, 8, status) != CVLM_E_BADARG;
    bad += call(bits, 52, offsets, dims, P, 0, n_vertices, vo, xy, start, n_rings, 8, status) != CVLM_E_BADARG;
    bad += call(bits, 52, offsets, dims, P, 8, n_vertices, vo, xy, start, n_rings, -1, status) != CVLM_E_BADARG;
    bad += call(bits, 52, offsets, dims, P, 8, n_vertices, vo, (int16_t*)bits, start, n_rings, 8, status) != CVLM_E_BADARG;      // outputs meeting bits
    bad += call(bits, 52, offsets, dims, P, 8, n_vertices, vo, xy, bits + 48, n_rings, 8, status) != CVLM_E_BADARG;
    bad += call(bits, 52, offsets, dims, P, 8, n_vertices, vo, xy, (uint8_t*)xy + 31, n_rings, 8, status) != CVLM_E_BADARG;      // and each other
    bad += call(bits, 52, offsets, dims, P, 8, n_vertices, vo, xy, start, (int32_t*)xy, 8, status) != CVLM_E_BADARG;
    bad += cvlm_mask_contour_workspace_bytes(0, 1, 1) != CVLM_E_BADARG;
    bad += cvlm_mask_contour_workspace_bytes(1, -1, 1) != CVLM_E_BADARG;
    bad += cvlm_mask_contour_workspace_bytes(1, 1, 0) != CVLM_E_BADARG;
    bad += cvlm_mask_contour_workspace_bytes(2, 12, 10) != 16 + 20 * 2 * 22 + 28 * 12;
    free(bits);
    return bad;
}

}  // namespace

int main() {
    const std::vector<std::pair<int, int>> ragged = {{1, 1}, {70, 33}, {5, 65}, {33, 31}, {1, 32}, {97, 131}, {2, 64}};
    int bad = 0, runs = 0;
    for (int connectivity : {4, 8})
        for (int density : {2, 20, 50, 80, 97, 100, 0}) {
            bad += check_contours(ragged, density, connectivity, -1, NONE);
            ++runs;
        }
    const Refusal hows[] = {SHORT_SLICE, ODD_OFFSET, PAST_THE_END, HEIGHT_ZERO, WIDTH_HUGE, VERTEX_SHORT};
    for (Refusal how : hows)
        for (int where : {0, 3, 6}) {                                  // the first, a middle and the last plane
            bad += check_contours(ragged, 60, 8, where, how);
            ++runs;
        }
    bad += check_contours({{300, 300}, {40, 257}}, 50, 8, -1, NONE);
    bad += check_badargs();
    printf("contour_host_sanitize: %d runs, %d mismatches\n", runs + 1, bad);
    return bad != 0;
}
