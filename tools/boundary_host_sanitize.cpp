// Stand-alone check of cvlm_debug_mask_boundary_sized_host and cvlm_debug_coco_match_boundary_host for a host
// sanitizer: the entries' per-thread functions are the kernels' (csrc/boundary_logic.h, csrc/match_logic.h), so their indexing is what
// runs on the device.  Every buffer is a heap block of exactly the size the interface states, so that AddressSanitizer sees any
// access beyond it; the boundaries are held against a plain window loop, the matching against the mask matching where the boundary
// cannot decide and against a hand-worked pair where it does.
// Build and run on the CPU, from the repository root:
//   hipcc -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/boundary_host_sanitize.cpp camouflaged-vlm_amd/csrc/boundary.hip camouflaged-vlm_amd/csrc/match.hip \
//         -o /tmp/boundary_host_sanitize && /tmp/boundary_host_sanitize
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../include/cvlm.h"

namespace {

uint32_t rng_state = 2025u;
uint32_t rng() { return rng_state = rng_state * 1664525u + 1013904223u; }

bool pixel(const uint8_t* plane, int ws, int y, int x) { return (plane[(int64_t)y * 4 * ws + (x >> 3)] >> (7 - (x & 7))) & 1; }

// the window definition: every pixel of the window inside the plane and set
bool eroded(const uint8_t* plane, int h, int w, int ws, int y, int x, int d) {
    if (y - d < 0 || x - d < 0 || y + d > h - 1 || x + d > w - 1) return false;
    for (int yy = y - d; yy <= y + d; ++yy)
        for (int xx = x - d; xx <= x + d; ++xx)
            if (!pixel(plane, ws, yy, xx)) return false;
    return true;
}

enum Refusal { NONE, SHORT_SLICE, ODD_OFFSET, PAST_THE_END, RADIUS_ZERO, RADIUS_HUGE, HEIGHT_ZERO };

// one call over planes of the given sizes and radii; plane `bad_plane` is doctored as `how` says and must be refused
int check_boundary(const std::vector<std::pair<int, int>>& sizes, const std::vector<int>& radii, int density_percent, int bad_plane,
                   Refusal how, bool with_area) {
    const int P = (int)sizes.size();
    int32_t* dims = (int32_t*)malloc(sizeof(int32_t) * 2 * P);
    int32_t* radius = (int32_t*)malloc(sizeof(int32_t) * P);
    int64_t* offsets = (int64_t*)malloc(sizeof(int64_t) * (P + 1));
    std::vector<int64_t> true_off((size_t)P + 1, 0);
    int64_t max_words = 1;
    for (int p = 0; p < P; ++p) {
        dims[2 * p] = sizes[p].first;
        dims[2 * p + 1] = sizes[p].second;
        radius[p] = radii[p];
        const int64_t words = (int64_t)sizes[p].first * ((sizes[p].second + 31) / 32);
        max_words = words > max_words ? words : max_words;
        true_off[p + 1] = true_off[p] + 4 * words;
    }
    const int64_t nbytes = true_off[P];
    for (int p = 0; p <= P; ++p) offsets[p] = true_off[p];
    // what is refused besides bad_plane: a doctored offset is shared with the plane before it
    std::vector<int> refused((size_t)P, 0), untouched((size_t)P, 0);
    if (bad_plane >= 0) {
        refused[bad_plane] = 1;
        if (how == SHORT_SLICE) { offsets[bad_plane + 1] -= 4; if (bad_plane + 1 < P) refused[bad_plane + 1] = 1; }
        if (how == ODD_OFFSET) { offsets[bad_plane] += 2; untouched[bad_plane] = 1; if (bad_plane > 0) refused[bad_plane - 1] = untouched[bad_plane - 1] = 1; }
        if (how == PAST_THE_END) { offsets[P] += 4; refused[bad_plane] = 0; refused[P - 1] = untouched[P - 1] = 1; }
        if (how == RADIUS_ZERO) radius[bad_plane] = 0;
        if (how == RADIUS_HUGE) radius[bad_plane] = 16385;
        if (how == HEIGHT_ZERO) dims[2 * bad_plane] = 0;
    }
    uint8_t* bits = (uint8_t*)malloc((size_t)nbytes);
    for (int p = 0; p < P; ++p) {
        const int h = sizes[p].first, w = sizes[p].second, ws = (w + 31) / 32;
        uint8_t* plane = bits + true_off[p];
        for (int64_t i = 0; i < (int64_t)4 * h * ws; ++i) plane[i] = 0;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
                if ((int)(rng() >> 8) % 100 < density_percent) plane[(int64_t)y * 4 * ws + (x >> 3)] |= (uint8_t)(0x80 >> (x & 7));
    }
    uint8_t* out = (uint8_t*)malloc((size_t)nbytes);
    uint8_t* workspace = (uint8_t*)malloc((size_t)nbytes);
    for (int64_t i = 0; i < nbytes; ++i) out[i] = workspace[i] = 0xA5;
    int32_t* area = with_area ? (int32_t*)malloc(sizeof(int32_t) * P) : nullptr;
    int32_t* status = (int32_t*)malloc(sizeof(int32_t));
    int bad = cvlm_debug_mask_boundary_sized_host(bits, nbytes, offsets, dims, radius, P, max_words, workspace, out, area, status) != 0;
    bad |= status[0] != (bad_plane >= 0 ? 1 : 0);
    int64_t set = 0;
    for (int p = 0; p < P; ++p) {
        const int h = sizes[p].first, w = sizes[p].second, ws = (w + 31) / 32;
        if (refused[p]) {
            // zeroed where the doctored slice is whole words inside the buffer, the sentinel where it is not; a byte of the true slice
            // that the doctored one does not cover keeps the sentinel too
            for (int64_t i = true_off[p]; i < true_off[p + 1]; ++i) {
                const bool covered = !untouched[p] && i >= offsets[p] && i < offsets[p + 1];
                const bool by_neighbour = (p > 0 && refused[p - 1] && !untouched[p - 1] && i < offsets[p]) ||
                                          (p + 1 < P && refused[p + 1] && !untouched[p + 1] && i >= offsets[p + 1]);
                bad |= out[i] != (covered || by_neighbour ? 0 : 0xA5);
            }
            if (with_area) bad |= area[p] != 0;
            continue;
        }
        const uint8_t* src = bits + true_off[p];
        const uint8_t* got = out + true_off[p];
        int n = 0;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < 32 * ws; ++x) {
                const bool want = x < w && pixel(src, ws, y, x) && !eroded(src, h, w, ws, y, x, radii[p]);
                bad |= pixel(got, ws, y, x) != want;
                n += want;
            }
        set += n;
        if (with_area) bad |= area[p] != n;
    }
    printf("%s  boundary: %d planes, density %d %%, refusal %d of plane %d, %s: %lld bytes, %lld set\n", bad ? "FAIL" : "ok  ", P,
           density_percent, (int)how, bad_plane, with_area ? "areas" : "bits only", (long long)nbytes, (long long)set);
    free(status); free(area); free(workspace); free(out); free(bits); free(offsets); free(radius); free(dims);
    return bad;
}

// every CVLM_E_BADARG of the boundary entry: nothing may be read or written
int check_badargs() {
    const int64_t n = 64;
    uint8_t* block = (uint8_t*)malloc((size_t)(3 * n));
    int32_t dims[2] = {4, 100}, radius[1] = {1}, area[1], status[1];
    int64_t offsets[2] = {0, 64};
    uint8_t *bits = block, *ws = block + n, *out = block + 2 * n;
    int bad = cvlm_debug_mask_boundary_sized_host(bits, n, offsets, dims, radius, 1, 16, ws, out, area, status) != 0;
    auto refuses = [&](const uint8_t* b, int64_t nb, const int64_t* o, const int32_t* d, const int32_t* r, int32_t P, int64_t mw, void* w,
                       uint8_t* ob, int32_t* a, int32_t* s) { return cvlm_debug_mask_boundary_sized_host(b, nb, o, d, r, P, mw, w, ob, a, s) == CVLM_E_BADARG; };
    bad |= !refuses(nullptr, n, offsets, dims, radius, 1, 16, ws, out, area, status);
    bad |= !refuses(bits, n, nullptr, dims, radius, 1, 16, ws, out, area, status);
    bad |= !refuses(bits, n, offsets, nullptr, radius, 1, 16, ws, out, area, status);
    bad |= !refuses(bits, n, offsets, dims, nullptr, 1, 16, ws, out, area, status);
    bad |= !refuses(bits, n, offsets, dims, radius, 1, 16, nullptr, out, area, status);
    bad |= !refuses(bits, n, offsets, dims, radius, 1, 16, ws, nullptr, area, status);
    bad |= !refuses(bits, n, offsets, dims, radius, 1, 16, ws, out, area, nullptr);
    bad |= !refuses(bits + 2, n, offsets, dims, radius, 1, 16, ws, out, area, status);
    bad |= !refuses(bits, n, offsets, dims, radius, 1, 16, ws + 2, out, area, status);
    bad |= !refuses(bits, n, offsets, dims, radius, 1, 16, ws, out - 2, area, status);
    bad |= !refuses(bits, n, (const int64_t*)((const uint8_t*)offsets + 4), dims, radius, 1, 16, ws, out, area, status);
    bad |= !refuses(bits, n, offsets, dims, radius, 0, 16, ws, out, area, status);
    bad |= !refuses(bits, n, offsets, dims, radius, 65536, 16, ws, out, area, status);
    bad |= !refuses(bits, 3, offsets, dims, radius, 1, 16, ws, out, area, status);
    bad |= !refuses(bits, n, offsets, dims, radius, 1, 0, ws, out, area, status);
    bad |= !refuses(bits, n, offsets, dims, radius, 1, (int64_t)16384 * 512 + 1, ws, out, area, status);
    bad |= !refuses(bits, n, offsets, dims, radius, 1, 16, ws, bits, area, status);               // out_bits is bits
    bad |= !refuses(bits, n, offsets, dims, radius, 1, 16, ws, bits + n - 4, area, status);       // out_bits meets bits
    bad |= !refuses(bits, n, offsets, dims, radius, 1, 16, bits + 4, out, area, status);          // the workspace meets bits
    bad |= !refuses(bits, n, offsets, dims, radius, 1, 16, ws, ws + 4, area, status);             // out_bits meets the workspace
    printf("%s  boundary: every CVLM_E_BADARG\n", bad ? "FAIL" : "ok  ");
    free(block);
    return bad;
}

// D detections against G annotations in one group; the boundary tables hold either the masks' own integers (then the minimum is the
// mask IoU and the tables must equal the mask matching's) or intersections of 0 (then nothing may match)
int check_match(int D, int G, bool zero_boundary, bool refuse) {
    const int T = 10, A = 4;
    auto i32 = [](int n) { return (int32_t*)malloc(sizeof(int32_t) * (size_t)(n > 0 ? n : 1)); };
    int32_t *det_off = i32(2), *gt_off = i32(2), *inter = i32(D * G), *inter_b = i32(D * G), *det_area = i32(D), *gt_area = i32(G);
    int32_t *det_area_b = i32(D), *gt_area_b = i32(G);
    int64_t* pair_off = (int64_t*)malloc(sizeof(int64_t) * 2);
    float* score = (float*)malloc(sizeof(float) * (size_t)(D > 0 ? D : 1));
    double* range_area = (double*)malloc(sizeof(double) * (size_t)(G > 0 ? G : 1));
    uint8_t* crowd = (uint8_t*)malloc((size_t)(G > 0 ? G : 1));
    double thrs[T], rngs[2 * A] = {0, 1e10, 0, 15, 15, 25, 25, 1e10};
    for (int t = 0; t < T; ++t) thrs[t] = 0.5 + 0.05 * t;
    det_off[0] = gt_off[0] = 0; det_off[1] = D; gt_off[1] = G;
    pair_off[0] = 0; pair_off[1] = (int64_t)D * G - (refuse ? 1 : 0);
    for (int d = 0; d < D; ++d) { det_area[d] = det_area_b[d] = 1 + (int)(rng() >> 8) % 40; score[d] = (float)((int)(rng() >> 8) % 4) / 4; }
    for (int g = 0; g < G; ++g) { gt_area[g] = gt_area_b[g] = 1 + (int)(rng() >> 8) % 40; range_area[g] = gt_area[g]; crowd[g] = (rng() >> 8) % 4 == 0; }
    for (int d = 0; d < D; ++d)
        for (int g = 0; g < G; ++g) {
            const int m = det_area[d] < gt_area[g] ? det_area[d] : gt_area[g];
            inter[d * G + g] = (int)(rng() >> 8) % (m + 1);
            inter_b[d * G + g] = zero_boundary ? 0 : inter[d * G + g];
        }
    const int AT = A * T;
    struct Out { int32_t *order, *dtm, *gtm, *status; uint8_t *dti, *gti; } o[2];
    for (Out& x : o) {
        x.order = i32(D); x.dtm = i32(AT * D); x.gtm = i32(AT * G); x.status = i32(1);
        x.dti = (uint8_t*)malloc((size_t)(AT * D > 0 ? AT * D : 1)); x.gti = (uint8_t*)malloc((size_t)(A * G > 0 ? A * G : 1));
    }
    auto nn = [](auto* p, int n) { return n > 0 ? p : (decltype(p))nullptr; };
    int bad = cvlm_debug_coco_match_host(det_off, gt_off, pair_off, 1, nn(inter, D * G), (int64_t)D * G, nn(det_area, D), nn(score, D), D,
                                         nn(gt_area, G), nn(range_area, G), nn(crowd, G), G, thrs, T, rngs, A, 100, nn(o[0].order, D),
                                         nn(o[0].dtm, D), nn(o[0].dti, D), nn(o[0].gtm, G), nn(o[0].gti, G), o[0].status) != 0;
    bad |= cvlm_debug_coco_match_boundary_host(det_off, gt_off, pair_off, 1, nn(inter, D * G), (int64_t)D * G, nn(det_area, D), nn(score, D), D,
                                               nn(gt_area, G), nn(range_area, G), nn(crowd, G), G, thrs, T, rngs, A, 100, nn(inter_b, D * G),
                                               nn(det_area_b, D), nn(gt_area_b, G), nn(o[1].order, D), nn(o[1].dtm, D), nn(o[1].dti, D),
                                               nn(o[1].gtm, G), nn(o[1].gti, G), o[1].status) != 0;
    bad |= o[0].status[0] != (refuse ? 1 : 0) || o[1].status[0] != (refuse ? 1 : 0);
    int matched = 0;
    for (int i = 0; i < D; ++i) bad |= o[0].order[i] != o[1].order[i];
    for (int i = 0; i < AT * D; ++i) {
        matched += o[1].dtm[i] >= 0;
        if (!zero_boundary || refuse) bad |= o[0].dtm[i] != o[1].dtm[i] || o[0].dti[i] != o[1].dti[i];
    }
    for (int i = 0; i < AT * G; ++i)
        if (!zero_boundary || refuse) bad |= o[0].gtm[i] != o[1].gtm[i];
    for (int i = 0; i < A * G; ++i) bad |= o[0].gti[i] != o[1].gti[i];
    if (zero_boundary) bad |= matched != 0;
    printf("%s  match:    %d x %d, boundary %s, %s: %d matches\n", bad ? "FAIL" : "ok  ", D, G, zero_boundary ? "disjoint" : "as the mask",
           refuse ? "refused group" : "accepted", matched);
    for (Out& x : o) { free(x.order); free(x.dtm); free(x.gtm); free(x.status); free(x.dti); free(x.gti); }
    free(crowd); free(range_area); free(score); free(pair_off); free(gt_area_b); free(det_area_b); free(gt_area); free(det_area); free(inter_b);
    free(inter); free(gt_off); free(det_off);
    return bad;
}

}  // namespace

int main() {
    int bad = 0;
    const std::vector<std::pair<int, int>> ragged = {{1, 1}, {70, 33}, {5, 65}, {33, 31}, {1, 32}, {97, 131}, {2, 64}};
    const std::vector<int> radii = {1, 2, 1, 16, 17, 3, 1};
    for (int density : {0, 50, 90, 98, 100}) bad |= check_boundary(ragged, radii, density, -1, NONE, true);
    bad |= check_boundary(ragged, radii, 95, -1, NONE, false);
    bad |= check_boundary({{389, 70}, {300, 40}, {40, 300}}, {3, 40, 463}, 99, -1, NONE, true);  // row segments: 128 and 160 rows; 2 d + 1 > h
    for (Refusal how : {SHORT_SLICE, ODD_OFFSET, PAST_THE_END, RADIUS_ZERO, RADIUS_HUGE, HEIGHT_ZERO})
        for (int p : {0, 3, 6}) bad |= check_boundary(ragged, radii, 95, p, how, p != 3);
    bad |= check_badargs();
    for (const auto& s : std::vector<std::pair<int, int>>{{0, 3}, {3, 0}, {1, 1}, {5, 4}, {33, 31}, {64, 65}, {130, 70}})
        for (int zero = 0; zero < 2; ++zero) bad |= check_match(s.first, s.second, zero != 0, false);
    bad |= check_match(5, 4, false, true);
    printf(bad ? "FAILED\n" : "all equal to the plain loops\n");
    return bad;
}
