// Stand-alone check of cvlm_debug_mask_regions_sized_host and cvlm_debug_region_alpha_host for a host sanitizer: the
// entries run the kernels' own per-thread functions (csrc/components_logic.h, csrc/regions_logic.h), so their indexing is what runs on
// the device.  Every buffer is a heap block of exactly the size the interface states, so that AddressSanitizer sees any access beyond
// it; the sizes are ragged, the pad bits dirty, a refused plane sits at the first, a middle and the last position, every CVLM_E_BADARG
// is tried, and the result is held against a flood fill written from the definition.
// Build and run on the CPU, from the repository root:
//   hipcc -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/regions_host_sanitize.cpp camouflaged-vlm_amd/csrc/regions.hip -o /tmp/regions_host_sanitize && /tmp/regions_host_sanitize
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../include/cvlm.h"

namespace {

uint32_t rng_state = 2029u;
uint32_t rng() { return rng_state = rng_state * 1664525u + 1013904223u; }

typedef std::vector<uint8_t> Plane;                                   // h * w bytes, 0 or 1
struct Region { int area, x0, y0, x1, y1, seed; std::vector<int> pixels; };

// the regions of a plane by flood fill in raster order of their first pixels, then sorted by (-area, seed)
std::vector<Region> regions_of(const Plane& x, int h, int w, int connectivity, int min_area) {
    std::vector<int> label((size_t)h * w, -1), stack;
    std::vector<Region> out;
    for (int i = 0; i < h * w; ++i) {
        if (!x[i] || label[i] >= 0) continue;
        Region r = {0, w, h, -1, -1, i, {}};
        stack.assign(1, i);
        label[i] = (int)out.size();
        while (!stack.empty()) {
            const int j = stack.back(), y = j / w, c = j % w;
            stack.pop_back();
            ++r.area;
            r.pixels.push_back(j);
            r.x0 = std::min(r.x0, c); r.y0 = std::min(r.y0, y); r.x1 = std::max(r.x1, c); r.y1 = std::max(r.y1, y);
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if ((dy == 0 && dx == 0) || (connectivity == 4 && dy != 0 && dx != 0)) continue;
                    const int yy = y + dy, cc = c + dx;
                    if (yy < 0 || yy >= h || cc < 0 || cc >= w || !x[(size_t)yy * w + cc] || label[(size_t)yy * w + cc] >= 0) continue;
                    label[(size_t)yy * w + cc] = label[i];
                    stack.push_back(yy * w + cc);
                }
        }
        if (r.area >= std::max(min_area, 1)) out.push_back(r);
    }
    std::stable_sort(out.begin(), out.end(), [](const Region& a, const Region& b) { return a.area != b.area ? a.area > b.area : a.seed < b.seed; });
    return out;
}

enum Refusal { NONE, SHORT_SLICE, ODD_OFFSET, PAST_THE_END, HEIGHT_ZERO, WIDTH_HUGE };

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

int check_regions(const std::vector<std::pair<int, int>>& sizes, int density_percent, int connectivity, int M, int min_area, int bad_plane,
                  Refusal how) {
    const int P = (int)sizes.size();
    int32_t* dims = (int32_t*)malloc(sizeof(int32_t) * 2 * P);
    int64_t* offsets = (int64_t*)malloc(sizeof(int64_t) * (P + 1));
    std::vector<int64_t> true_off((size_t)P + 1, 0);
    int64_t max_words = 1;
    for (int p = 0; p < P; ++p) {
        dims[2 * p] = sizes[p].first;
        dims[2 * p + 1] = sizes[p].second;
        const int64_t words = (int64_t)sizes[p].first * ((sizes[p].second + 31) / 32);
        max_words = std::max(max_words, words);
        true_off[p + 1] = true_off[p] + 4 * words;
    }
    const int64_t nbytes = true_off[P];
    for (int p = 0; p <= P; ++p) offsets[p] = true_off[p];
    std::vector<int> refused((size_t)P, 0), untouched((size_t)P, 0);
    if (bad_plane >= 0) {
        refused[bad_plane] = 1;
        if (how == SHORT_SLICE && bad_plane + 1 < P) { offsets[bad_plane + 1] -= 4; refused[bad_plane + 1] = 1; }
        if (how == SHORT_SLICE && bad_plane + 1 == P) { offsets[bad_plane] += 4; refused[bad_plane - 1] = 1; }
        if (how == ODD_OFFSET) { offsets[bad_plane] += 2; untouched[bad_plane] = 1; if (bad_plane > 0) refused[bad_plane - 1] = untouched[bad_plane - 1] = 1; }
        if (how == PAST_THE_END) { offsets[P] += 4; refused[bad_plane] = 0; refused[P - 1] = untouched[P - 1] = 1; }
        if (how == HEIGHT_ZERO) dims[2 * bad_plane] = 0;
        if (how == WIDTH_HUGE) dims[2 * bad_plane + 1] = 16385;
    }
    uint8_t* bits = (uint8_t*)malloc((size_t)nbytes);
    std::vector<Plane> planes((size_t)P);
    for (int p = 0; p < P; ++p) {
        const int h = sizes[p].first, w = sizes[p].second, ws = (w + 31) / 32;
        uint8_t* stored = bits + true_off[p];
        memset(stored, 0, (size_t)4 * h * ws);
        planes[p].assign((size_t)h * w, 0);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < 32 * ws; ++x) {
                const bool on = x >= w ? true : (int)(rng() >> 8) % 100 < density_percent;      // dirty pad bits
                if (x < w) planes[p][(size_t)y * w + x] = on;
                if (on) stored[(int64_t)y * 4 * ws + (x >> 3)] |= (uint8_t)(0x80u >> (x & 7));
            }
    }
    uint8_t* out = (uint8_t*)malloc((size_t)(M * nbytes));
    memset(out, 0xA5, (size_t)(M * nbytes));
    int32_t* n_regions = (int32_t*)malloc(sizeof(int32_t) * P);
    int32_t* table = (int32_t*)malloc(sizeof(int32_t) * 6 * P * M);
    int32_t* status = (int32_t*)malloc(sizeof(int32_t));
    status[0] = 77;
    const int rc = cvlm_debug_mask_regions_sized_host(bits, nbytes, offsets, dims, P, max_words, connectivity, M, min_area, n_regions, table, out,
                                                      status);
    if (rc != 0) FAIL("rc %d", rc);
    bool any_refused = false;
    for (int p = 0; p < P; ++p) any_refused |= refused[p] != 0;
    if (status[0] != (any_refused ? 1 : 0)) FAIL("status %d", status[0]);
    for (int p = 0; p < P; ++p) {
        const int h = sizes[p].first, w = sizes[p].second, ws = (w + 31) / 32;
        const int64_t size = (int64_t)4 * h * ws;
        const uint8_t* got = out + M * true_off[p];
        const int32_t* rows = table + (int64_t)p * M * 6;
        if (refused[p]) {
            for (int64_t i = 0; i < M * size; ++i)
                if (got[i] != (untouched[p] ? 0xA5 : 0)) FAIL("plane %d: a refused slice holds %d", p, got[i]);
            if (n_regions[p] != 0) FAIL("plane %d: refused, %d regions", p, n_regions[p]);
            for (int m = 0; m < M; ++m)
                if (rows[6 * m] != 0 || rows[6 * m + 1] != -1 || rows[6 * m + 5] != -1) FAIL("plane %d: refused, row %d", p, m);
            continue;
        }
        const std::vector<Region> want = regions_of(planes[p], h, w, connectivity, min_area);
        if (n_regions[p] != (int)want.size()) FAIL("plane %d: %d regions, want %zu", p, n_regions[p], want.size());
        for (int m = 0; m < M; ++m) {
            const int32_t* r = rows + 6 * m;
            Plane slot((size_t)h * w, 0);
            if (m < (int)want.size()) {
                const Region& q = want[m];
                if (r[0] != q.area || r[1] != q.x0 || r[2] != q.y0 || r[3] != q.x1 || r[4] != q.y1 || r[5] != q.seed)
                    FAIL("plane %d row %d: %d %d %d %d %d %d, want %d %d %d %d %d %d", p, m, r[0], r[1], r[2], r[3], r[4], r[5], q.area, q.x0, q.y0,
                         q.x1, q.y1, q.seed);
                for (int j : q.pixels) slot[j] = 1;
            } else if (r[0] != 0 || r[1] != -1 || r[2] != -1 || r[3] != -1 || r[4] != -1 || r[5] != -1) {
                FAIL("plane %d row %d is no filler", p, m);
            }
            const uint8_t* s = got + m * size;
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < 32 * ws; ++x) {
                    const int bit = (s[(int64_t)y * 4 * ws + (x >> 3)] >> (7 - (x & 7))) & 1;
                    if (bit != (x < w ? slot[(size_t)y * w + x] : 0)) FAIL("plane %d slot %d (%d x %d): pixel (%d, %d) is %d", p, m, h, w, y, x, bit);
                }
        }
    }
    free(dims); free(offsets); free(bits); free(out); free(n_regions); free(table); free(status);
    return 0;
}

// cvlm_debug_region_alpha_host against the four-tap definition in double, and its exact cases
int check_alpha(const std::vector<std::pair<int, int>>& sizes, int R) {
    const int Q = (int)sizes.size(), N = 2;
    int32_t* dims = (int32_t*)malloc(sizeof(int32_t) * 2 * Q);
    int64_t* offsets = (int64_t*)malloc(sizeof(int64_t) * (Q + 1));
    int32_t* src = (int32_t*)malloc(sizeof(int32_t) * Q);
    offsets[0] = 0;
    for (int q = 0; q < Q; ++q) {
        dims[2 * q] = sizes[q].first;
        dims[2 * q + 1] = sizes[q].second;
        offsets[q + 1] = offsets[q] + (int64_t)4 * sizes[q].first * ((sizes[q].second + 31) / 32);
        src[q] = q % N;
    }
    const int64_t nbytes = offsets[Q], RR = (int64_t)R * R;
    uint8_t* bits = (uint8_t*)malloc((size_t)nbytes);
    for (int64_t i = 0; i < nbytes; ++i) bits[i] = (uint8_t)(rng() >> 13);
    float* alpha = (float*)malloc(sizeof(float) * N * RR);
    for (int64_t i = 0; i < N * RR; ++i) alpha[i] = (float)(rng() >> 8) / 16777216.0f;
    float* out = (float*)malloc(sizeof(float) * Q * RR);
    int32_t status[1] = {77};
    if (cvlm_debug_region_alpha_host(bits, nbytes, offsets, dims, Q, alpha, N, R, src, out, status) != 0 || status[0] != 0) FAIL("alpha: rc or status");
    for (int q = 0; q < Q; ++q) {
        const int h = sizes[q].first, w = sizes[q].second, ws = (w + 31) / 32;
        const uint8_t* plane = bits + offsets[q];
        auto bit = [&](int y, int x) { return (double)((plane[(int64_t)y * 4 * ws + (x >> 3)] >> (7 - (x & 7))) & 1); };
        for (int oy = 0; oy < R; ++oy)
            for (int ox = 0; ox < R; ++ox) {
                const float fy = std::max(0.0f, (float)h / (float)R * ((float)oy + 0.5f) - 0.5f), fx = std::max(0.0f, (float)w / (float)R * ((float)ox + 0.5f) - 0.5f);
                const int y0 = (int)fy, x0 = (int)fx, y1 = y0 + (y0 < h - 1), x1 = x0 + (x0 < w - 1);
                const double ly = (double)(fy - (float)y0), lx = (double)(fx - (float)x0);
                const double g = (1 - ly) * ((1 - lx) * bit(y0, x0) + lx * bit(y0, x1)) + ly * ((1 - lx) * bit(y1, x0) + lx * bit(y1, x1));
                const double want = (double)alpha[src[q] * RR + (int64_t)oy * R + ox] * g, got = out[q * RR + (int64_t)oy * R + ox];
                if (std::fabs(got - want) > 1e-6) FAIL("alpha: plane %d (%d, %d): %g, want %g", q, oy, ox, got, want);
                if (h == R && w == R && got != (double)(alpha[src[q] * RR + (int64_t)oy * R + ox] * (float)bit(oy, ox))) FAIL("alpha: (R, R) is not exact");
            }
    }
    src[Q - 1] = N;                                                   // outside [0, N): refused through status, its out zeroed
    if (cvlm_debug_region_alpha_host(bits, nbytes, offsets, dims, Q, alpha, N, R, src, out, status) != 0 || status[0] != 1) FAIL("alpha: a bad src is taken");
    for (int64_t i = 0; i < RR; ++i)
        if (out[(Q - 1) * RR + i] != 0.0f) FAIL("alpha: a refused plane is not zeroed");
    if (cvlm_debug_region_alpha_host(bits, nbytes, offsets, dims, Q, alpha, N, 0, src, out, status) != CVLM_E_BADARG ||
        cvlm_debug_region_alpha_host(nullptr, nbytes, offsets, dims, Q, alpha, N, R, src, out, status) != CVLM_E_BADARG ||
        cvlm_debug_region_alpha_host(bits, nbytes, offsets, dims, Q, nullptr, N, R, src, out, status) != CVLM_E_BADARG ||
        cvlm_debug_region_alpha_host(bits, nbytes, offsets, dims, 0, alpha, N, R, src, out, status) != CVLM_E_BADARG)
        FAIL("alpha: a bad argument is taken");
    free(dims); free(offsets); free(src); free(bits); free(alpha); free(out);
    return 0;
}

int check_badargs() {
    int32_t dims[4] = {5, 40, 3, 7};
    int64_t offsets[3] = {0, 40, 52};
    const int64_t nbytes = 52, max_words = 10;
    const int M = 2;
    if (cvlm_mask_regions_workspace_bytes(nbytes, 2, max_words) != 112 * nbytes || cvlm_mask_regions_workspace_bytes(40, 1, 10) != 4480)
        FAIL("workspace_bytes");
    if (cvlm_mask_regions_workspace_bytes(3, 1, 1) != CVLM_E_BADARG || cvlm_mask_regions_workspace_bytes(8, 0, 1) != CVLM_E_BADARG ||
        cvlm_mask_regions_workspace_bytes(8, 65536, 1) != CVLM_E_BADARG || cvlm_mask_regions_workspace_bytes(8, 1, 0) != CVLM_E_BADARG)
        FAIL("workspace_bytes takes arguments out of range");
    uint8_t* bits = (uint8_t*)calloc(1, (size_t)nbytes);
    uint8_t* out = (uint8_t*)malloc((size_t)(M * nbytes));
    int32_t n[2], table[2 * M * 6], status[1];
    struct Args { const uint8_t* bits; int64_t nb; const int64_t* off; const int32_t* dims; int32_t P; int64_t mw; int32_t conn, M, min_area;
                  int32_t *n, *table; uint8_t* out; int32_t* status; };
    const Args good = {bits, nbytes, offsets, dims, 2, max_words, 8, M, 0, n, table, out, status};
    auto call = [](const Args& a) {
        return cvlm_debug_mask_regions_sized_host(a.bits, a.nb, a.off, a.dims, a.P, a.mw, a.conn, a.M, a.min_area, a.n, a.table, a.out, a.status);
    };
    if (call(good) != 0 || status[0] != 0 || n[0] != 0 || n[1] != 0) FAIL("the good call fails");
    std::vector<Args> bad;
    Args a;
#define BAD(stmt) a = good; stmt; bad.push_back(a)
    BAD(a.bits = nullptr); BAD(a.off = nullptr); BAD(a.dims = nullptr); BAD(a.n = nullptr); BAD(a.table = nullptr); BAD(a.out = nullptr);
    BAD(a.status = nullptr); BAD(a.bits = bits + 2); BAD(a.dims = (const int32_t*)((const uint8_t*)dims + 2)); BAD(a.out = out + 2);
    BAD(a.n = (int32_t*)((uint8_t*)n + 2)); BAD(a.table = (int32_t*)((uint8_t*)table + 2)); BAD(a.status = (int32_t*)((uint8_t*)status + 2));
    BAD(a.off = (const int64_t*)((const uint8_t*)offsets + 4)); BAD(a.P = 0); BAD(a.P = 65536); BAD(a.nb = 3); BAD(a.mw = 0);
    BAD(a.mw = (int64_t)16384 * 512 + 1); BAD(a.conn = 6); BAD(a.M = 0); BAD(a.M = 65); BAD(a.min_area = -1); BAD(a.out = bits);
    BAD(a.out = (uint8_t*)dims); BAD(a.n = status); BAD(a.table = n); BAD(a.status = (int32_t*)out);
#undef BAD
    for (size_t i = 0; i < bad.size(); ++i)
        if (call(bad[i]) != CVLM_E_BADARG) FAIL("bad call %zu is taken", i);
    free(bits); free(out);
    return 0;
}

}  // namespace

int main() {
    const std::vector<std::pair<int, int>> ragged = {{1, 1}, {70, 33}, {5, 65}, {33, 31}, {1, 32}, {97, 131}, {4, 64}};
    int calls = 0;
    for (int density : {0, 20, 45, 59, 80, 100})
        for (int connectivity : {4, 8}) {
            if (check_regions(ragged, density, connectivity, connectivity == 4 ? 5 : 64, density == 45 ? 4 : 0, -1, NONE)) return 1;
            ++calls;
        }
    if (check_regions({{32, 32}, {2, 2}}, 50, 4, 1, 1, -1, NONE)) return 1;
    for (int bad_plane : {0, 3, 6})
        for (Refusal how : {SHORT_SLICE, ODD_OFFSET, PAST_THE_END, HEIGHT_ZERO, WIDTH_HUGE}) {
            if (check_regions(ragged, 55, 8, 3, 0, bad_plane, how)) {
                fprintf(stderr, "refusal %d at plane %d\n", (int)how, bad_plane);
                return 1;
            }
            ++calls;
        }
    if (check_alpha({{1, 1}, {5, 33}, {20, 30}, {56, 56}, {90, 130}}, 56) || check_alpha({{7, 7}, {3, 70}}, 7)) return 1;
    if (check_badargs()) return 1;
    printf("regions_host_sanitize: %d calls, two alpha checks and every refused argument: ok\n", calls + 1);
    return 0;
}
