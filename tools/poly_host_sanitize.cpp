// Stand-alone check of cvlm_debug_mask_poly_decode_host for a host sanitizer: the entry's per-thread functions are the
// kernels' (csrc/poly_logic.h, csrc/gt_logic.h), so their indexing is what runs on the device.  Every buffer is a heap block of exactly
// the size the interface states, so that AddressSanitizer sees any access beyond it; the planes are held against a restatement of §21
// in doubles that ends in a plain pixel loop: the boundary positions sorted, the value flipping at each of them, the union by OR.
// Refused planes -- a NaN, an infinity, a coordinate beyond the bound, two vertices, an odd slice, a polygon over the point cap, an
// empty list, slices that run backwards or beyond the end, a plane beyond max_pixels, a table that does not fit -- run through the same
// exact-size buffers.
// Build and run on the CPU, from the repository root:
//   hipcc -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/poly_host_sanitize.cpp camouflaged-vlm_amd/csrc/gt.hip -o /tmp/poly_host_sanitize && /tmp/poly_host_sanitize
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/cvlm.h"

#pragma clang fp contract(off)

namespace {

uint32_t rng_state = 2121u;
uint32_t rng() { return rng_state = rng_state * 1664525u + 1013904223u; }
double uniform(double lo, double hi) { return lo + (hi - lo) * ((rng() >> 8) / 16777216.0); }

typedef std::vector<double> Poly;
struct Case { std::vector<Poly> polys; int h, w; };

bool poly_ok(const Poly& xy) {
    if (xy.size() % 2 || xy.size() < 6 || xy.size() > 2 * 65535) return false;
    for (double c : xy)
        if (!(c >= -65536.0 && c <= 65536.0)) return false;
    const size_t k = xy.size() / 2;
    int64_t pts = 0;
    for (size_t j = 0; j < k; ++j) {
        const size_t n = (j + 1) % k;
        const int dx = std::abs((int)(5.0 * xy[2 * j] + 0.5) - (int)(5.0 * xy[2 * n] + 0.5));
        const int dy = std::abs((int)(5.0 * xy[2 * j + 1] + 0.5) - (int)(5.0 * xy[2 * n + 1] + 0.5));
        pts += std::max(dx, dy) + 1;
    }
    return pts <= ((int64_t)1 << 24);
}

// §21 in doubles, as the published rleFrPoly has it, then a pixel loop: px[y * w + x] |= inside
void paint(const Poly& xy, int h, int w, std::vector<uint8_t>& px) {
    const size_t k = xy.size() / 2;
    std::vector<int> x(k + 1), y(k + 1), u, v;
    for (size_t j = 0; j < k; ++j) { x[j] = (int)(5.0 * xy[2 * j] + 0.5); y[j] = (int)(5.0 * xy[2 * j + 1] + 0.5); }
    x[k] = x[0]; y[k] = y[0];
    for (size_t j = 0; j < k; ++j) {
        int xs = x[j], xe = x[j + 1], ys = y[j], ye = y[j + 1];
        const int dx = std::abs(xe - xs), dy = std::abs(ys - ye);
        const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
        if (flip) { std::swap(xs, xe); std::swap(ys, ye); }
        if (dx == 0 && dy == 0) { u.push_back(xs); v.push_back(ys); continue; }
        const double s = dx >= dy ? (double)(ye - ys) / dx : (double)(xe - xs) / dy;
        if (dx >= dy)
            for (int d = 0; d <= dx; ++d) { const int t = flip ? dx - d : d; u.push_back(t + xs); v.push_back((int)(ys + s * t + .5)); }
        else
            for (int d = 0; d <= dy; ++d) { const int t = flip ? dy - d : d; v.push_back(t + ys); u.push_back((int)(xs + s * t + .5)); }
    }
    std::vector<int64_t> a;
    for (size_t j = 1; j < u.size(); ++j)
        if (u[j] != u[j - 1]) {
            double xd = (double)(u[j] < u[j - 1] ? u[j] : u[j] - 1);
            xd = (xd + .5) / 5.0 - .5;
            if (std::floor(xd) != xd || xd < 0 || xd > w - 1) continue;
            double yd = (double)(v[j] < v[j - 1] ? v[j] : v[j - 1]);
            yd = (yd + .5) / 5.0 - .5;
            if (yd < 0) yd = 0; else if (yd > h) yd = h;
            yd = std::ceil(yd);
            a.push_back((int64_t)(int)xd * h + (int)yd);
        }
    std::sort(a.begin(), a.end());
    size_t next = 0;
    int value = 0;
    for (int64_t j = 0; j < (int64_t)h * w; ++j) {
        while (next < a.size() && a[next] <= j) { value ^= 1; ++next; }
        if (value) px[(size_t)(j % h) * w + (size_t)(j / h)] = 1;
    }
}

int words_per_row(int w) { return (w + 31) / 32; }
bool bit_of(const uint8_t* rows, int w, int y, int x) { return (rows[(size_t)y * 4 * words_per_row(w) + (x >> 3)] >> (7 - (x & 7))) & 1; }

// one call over the cases.  bad_table: that plane's bit slice is four bytes short of its size; bend: 1 polygon offsets of plane 1 run
// backwards, 2 the last offset lies beyond the end, 3 plane 1's list is empty; max_pixels_cut: the largest plane the call admits, 0: the
// largest of the cases.  Returns the number of mismatches.
int check(const std::vector<Case>& cases, int bad_table, bool with_stats, int bend, int64_t max_pixels_cut) {
    const int P = (int)cases.size();
    int Q = 0;
    int64_t total = 0, max_pixels = 1;
    for (const Case& c : cases) {
        Q += (int)c.polys.size();
        for (const Poly& p : c.polys) total += (int64_t)p.size();
    }
    double* xy = (double*)malloc(sizeof(double) * (size_t)total);
    int64_t* po = (int64_t*)malloc(sizeof(int64_t) * (Q + 1));
    int32_t* pp = (int32_t*)malloc(sizeof(int32_t) * (P + 1));
    int64_t* bo = (int64_t*)malloc(sizeof(int64_t) * (P + 1));
    int32_t* dims = (int32_t*)malloc(sizeof(int32_t) * 2 * P);
    po[0] = bo[0] = 0;
    pp[0] = 0;
    int q = 0;
    for (int p = 0; p < P; ++p) {
        for (const Poly& poly : cases[p].polys) {
            if (!poly.empty()) memcpy(xy + po[q], poly.data(), sizeof(double) * poly.size());
            po[q + 1] = po[q] + (int64_t)poly.size();
            ++q;
        }
        pp[p + 1] = q;
        dims[2 * p] = cases[p].h;
        dims[2 * p + 1] = cases[p].w;
        bo[p + 1] = bo[p] + (int64_t)4 * cases[p].h * words_per_row(cases[p].w) - (p == bad_table ? 4 : 0);
        max_pixels = std::max(max_pixels, (int64_t)cases[p].h * cases[p].w);
    }
    if (bend == 1) po[pp[1] + 1] = po[pp[1]] - 2;
    if (bend == 2) po[Q] = total + 2;
    if (bend == 3)
        for (int p = P; p > 1; --p) pp[p] = pp[p - 1];
    const int64_t nbytes = bo[P];
    if (max_pixels_cut) max_pixels = max_pixels_cut;
    uint8_t* bits = (uint8_t*)malloc((size_t)nbytes);
    memset(bits, 0xA5, (size_t)nbytes);
    int32_t* area = with_stats ? (int32_t*)malloc(sizeof(int32_t) * P) : nullptr;
    int32_t* box = with_stats ? (int32_t*)malloc(sizeof(int32_t) * 4 * P) : nullptr;
    int32_t* status = (int32_t*)malloc(sizeof(int32_t));
    const int rc = cvlm_debug_mask_poly_decode_host(xy, total, po, pp, dims, bo, P, Q, max_pixels, bits, nbytes, area, box, status);
    int bad = rc != 0;
    bool any_refused = false;
    for (int p = 0; p < P; ++p) {
        const int h = cases[p].h, w = cases[p].w;
        if (p == bad_table) {                                         // nothing of its slice is stored
            for (int64_t i = bo[p]; i < bo[p + 1]; ++i) bad += bits[i] != 0xA5;
            any_refused = true;
            if (with_stats) bad += area[p] != 0 || box[4 * p] != -1;
            continue;
        }
        // what the call was given for this plane: the polygons pp[p] .. pp[p + 1] - 1 as the bent tables state them
        bool good = pp[p + 1] - pp[p] >= 1 && pp[p + 1] - pp[p] <= 4096 && (int64_t)h * w <= max_pixels && (Q > P || pp[p + 1] - pp[p] == 1);
        std::vector<uint8_t> px((size_t)h * w, 0);
        for (int k = pp[p]; k < pp[p + 1] && good; ++k) {
            if (po[k] < 0 || po[k] >= po[k + 1] || po[k + 1] > total) { good = false; break; }
            const Poly poly(xy + po[k], xy + po[k + 1]);
            good = poly_ok(poly);
            if (good) paint(poly, h, w, px);
        }
        if (!good) { px.assign((size_t)h * w, 0); any_refused = true; }
        const uint8_t* rows = bits + bo[p];
        int n = 0, x0 = w, y0 = h, x1 = -1, y1 = -1;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < 32 * words_per_row(w); ++x) {
                const bool want = x < w && px[(size_t)y * w + x];     // the pad bits are 0
                bad += bit_of(rows, w, y, x) != want;
                if (want) { ++n; x0 = std::min(x0, x); y0 = std::min(y0, y); x1 = std::max(x1, x); y1 = std::max(y1, y); }
            }
        if (with_stats) {
            if (n == 0) bad += area[p] != 0 || box[4 * p] != -1 || box[4 * p + 1] != -1 || box[4 * p + 2] != -1 || box[4 * p + 3] != -1;
            else bad += area[p] != n || box[4 * p] != x0 || box[4 * p + 1] != y0 || box[4 * p + 2] != x1 || box[4 * p + 3] != y1;
        }
    }
    bad += status[0] != (any_refused ? 1 : 0);
    free(xy); free(po); free(pp); free(bo); free(dims); free(bits); free(area); free(box); free(status);
    return bad;
}

Poly circle(int n, double cx, double cy, double r) {
    Poly p;
    for (int i = 0; i < n; ++i) { p.push_back(cx + r * std::cos(6.283185307179586 * i / n)); p.push_back(cy + r * std::sin(6.283185307179586 * i / n)); }
    return p;
}

std::vector<Poly> kinds(int h, int w) {
    const double W = w, H = h;
    return {{1, 1, 4, 1, 4, 4, 1, 4}, {1, 1, 1, 1, 4, 1, 4, 4, 4, 4, 1, 4}, {0.5, 0.5, 5.5, 0.5, 3, 5.5}, {1, 1, 3, 3, 5, 1, 5, 5, 1, 5},
            {-3, -3, W + 5, -3, W + 5, H + 5, -3, H + 5}, {2, 2, 2, 2, 2, 2}, {0.5, 0.5, W - 0.5, 0.5, W - 0.5, H - 0.5, 0.5, H - 0.5},
            {0, 0, W * 0.9, H * 0.2, W * 0.3, H * 0.95}, {0, 0, W * 0.3, H * 0.95, W * 0.9, H * 0.2}, {0, 0, W, H, W, 0, 0, H},
            {0, 0, W, 0, W, H, W * 0.5, H * 0.25, 0, H}, {W, H, W, -2.5, -2.5, -2.5, -2.5, H}, {-W - 3, 0, -1, 0, -1, H, -W - 3, H},
            {W / 2, -1, W / 2, H + 1, W / 2 + 0.3, H + 1, W / 2 + 0.3, -1}, {-1, H / 2, W + 1, H / 2, W + 1, H / 2 + 0.3, -1, H / 2 + 0.3},
            circle(1500, W * 0.5, H * 0.5, std::min(W, H) * 0.45)};
}

}  // namespace

int main() {
    const int shapes[][2] = {{1, 1}, {1, 32}, {5, 4}, {33, 31}, {32, 63}, {65, 97}, {130, 517}};
    int bad = 0;
    std::vector<Case> ragged;
    for (const auto& s : shapes) {
        std::vector<Case> cases;
        for (const Poly& p : kinds(s[0], s[1])) cases.push_back({{p}, s[0], s[1]});
        bad += check(cases, -1, true, 0, 0);
        bad += check(cases, -1, false, 0, 0);
        ragged.push_back(cases[7 + (s[0] + s[1]) % 8]);
    }
    // random polygons, three families: uniform doubles, tenths, integers
    for (int family = 0; family < 3; ++family) {
        std::vector<Case> cases;
        for (int i = 0; i < 1500; ++i) {
            Poly p;
            const int k = 3 + (int)(rng() >> 8) % 6;
            for (int j = 0; j < 2 * k; ++j)
                p.push_back(family == 0 ? uniform(-5, 45) : family == 1 ? ((int)((rng() >> 8) % 501) - 50) / 10.0 : (double)((int)((rng() >> 8) % 51) - 5));
            cases.push_back({{p}, 1 + (int)(rng() >> 8) % 40, 1 + (int)(rng() >> 8) % 40});
        }
        bad += check(cases, -1, true, 0, 0);
    }
    // unions: 2, 3 and 17 polygons, one inside another, ragged with planes of one
    std::vector<Case> unions = ragged;
    unions.insert(unions.begin() + 1, {{{1, 1, 20, 1, 20, 20, 1, 20}, {10, 10, 30, 10, 30, 28, 10, 28}}, 33, 31});
    unions.push_back({{{2, 2, 60, 2, 60, 30, 2, 30}, {10, 8, 30, 8, 30, 20, 10, 20}}, 32, 63});
    unions.push_back({{{1, 1, 8, 1, 8, 8, 1, 8}, {12, 3, 20, 3, 20, 9, 12, 9}, {30, 40, 60, 40, 60, 60, 30, 60}}, 65, 97});
    Case many{{}, 65, 97};
    for (int i = 0; i < 17; ++i) many.polys.push_back(circle(12, 16 + 14 * (i % 5), 12 + 14 * (i / 5), 9.5));
    unions.push_back(many);
    bad += check(unions, -1, true, 0, 0);
    bad += check(unions, 4, true, 0, 0);                              // a table that does not fit
    bad += check(unions, 0, true, 0, 0);
    bad += check(unions, -1, true, 0, 65 * 97);                       // the largest plane does not fit max_pixels
    bad += check(unions, -1, true, 1, 0);                             // offsets that run backwards
    bad += check(unions, -1, true, 2, 0);                             // the last offset beyond the end
    bad += check(unions, -1, true, 3, 0);                             // an empty list
    bad += check(ragged, -1, true, 3, 0);                             // ... where every other plane has one polygon
    // polygons that are none, alone, first and last of their plane's list, between planes that are whole
    const Poly tri = {0.5, 0.5, 20.5, 3.0, 7.0, 25.5}, square = {1, 1, 4, 1, 4, 4, 1, 4};
    std::vector<Poly> none = {{0.5, 0.5, NAN, 3.0, 7.0, 25.5}, {0.5, -INFINITY, 20.5, 3.0, 7.0, 25.5}, {0.5, 0.5, 65536.5, 3.0, 7.0, 25.5},
                              {0.5, 0.5, 20.5, 3.0}, {0.5, 0.5, 20.5, 3.0, 7.0, 25.5, 1.0}};
    Poly far;
    for (int i = 0; i < 3000; ++i) { far.push_back(i & 1 ? -65536.0 : 65536.0); far.push_back(i & 1 ? 65536.0 : -65536.0); }
    none.push_back(far);
    for (const Poly& p : none) {
        bad += check({{{tri}, 33, 31}, {{p}, 32, 63}, {{tri}, 5, 4}}, -1, true, 0, 0);
        bad += check({{{tri}, 33, 31}, {{p, square}, 32, 63}, {{tri}, 5, 4}}, -1, true, 0, 0);
        bad += check({{{tri}, 33, 31}, {{tri, square, p}, 32, 63}, {{tri, square}, 5, 4}}, -1, true, 0, 0);
    }
    printf("poly_host_sanitize: %d mismatches\n", bad);
    return bad != 0;
}
