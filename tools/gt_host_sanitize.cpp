// Stand-alone check of cvlm_debug_mask_rle_decode_host and cvlm_debug_mask_inter_sized_host for a host sanitizer: the
// entries' per-thread functions are the kernels' (csrc/gt_logic.h), so their indexing is what runs on the device.  Every buffer is a
// heap block of exactly the size the interface states, so that AddressSanitizer sees any access beyond it; the decoded planes are held
// against a plain pixel loop over the counts, the intersections against a plain pixel loop over the planes.  Refused planes -- a
// negative count, sums one short and one long, two counts of 2^30, an empty, a backwards and an overlong slice, tables that do not fit
// -- and refused pairs run through the same exact-size buffers.
// Build and run on the CPU, from the repository root:
//   hipcc -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/gt_host_sanitize.cpp camouflaged-vlm_amd/csrc/gt.hip -o /tmp/gt_host_sanitize && /tmp/gt_host_sanitize
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/cvlm.h"

namespace {

uint32_t rng_state = 2020u;
uint32_t rng() { return rng_state = rng_state * 1664525u + 1013904223u; }

struct Plane { int h, w; std::vector<uint8_t> px; };                  // px[y * w + x]

Plane make(int h, int w, int kind) {
    Plane p{h, w, std::vector<uint8_t>((size_t)h * w)};
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            uint8_t v = 0;
            switch (kind) {
                case 0: v = 0; break;
                case 1: v = 1; break;
                case 2: v = y == 0 && x == 0; break;
                case 3: v = y == h - 1 && x == w - 1; break;
                case 4: v = (y + x) & 1; break;
                case 5: v = y & 1; break;
                case 6: v = x & 1; break;
                case 7: v = (rng() >> 8) % 100 < 1; break;
                case 8: v = (rng() >> 8) % 100 < 50; break;
                default: v = (rng() >> 8) % 100 < 99; break;
            }
            p.px[(size_t)y * w + x] = v;
        }
    return p;
}

// column-major alternating runs, starting with the 0s; zeros: insert that many zero counts at a random place (the plane they describe
// is then whatever the pixel loop below says)
std::vector<int32_t> encode(const Plane& p, int zeros) {
    std::vector<int32_t> c;
    int value = 0, run = 0;
    for (int x = 0; x < p.w; ++x)
        for (int y = 0; y < p.h; ++y) {
            const int v = p.px[(size_t)y * p.w + x];
            if (v != value) { c.push_back(run); value = v; run = 0; }
            ++run;
        }
    c.push_back(run);
    if (zeros > 0) c.insert(c.begin() + (ptrdiff_t)(rng() % (c.size() + 1)), (size_t)zeros, 0);
    if (zeros < 0) c.push_back(0);                                    // a trailing 0
    return c;
}

// the pixel loop: the value flips at the end of every run; false where the counts describe no plane of h x w
bool decode_loop(const std::vector<int32_t>& c, int h, int w, std::vector<uint8_t>& px) {
    px.assign((size_t)h * w, 0);
    int64_t j = 0;
    int value = 0;
    if (c.empty()) return false;
    for (int32_t n : c) {
        if (n < 0 || j + n > (int64_t)h * w) return false;
        for (int32_t i = 0; i < n; ++i, ++j) px[(size_t)(j % h) * w + (size_t)(j / h)] = (uint8_t)value;
        value ^= 1;
    }
    return j == (int64_t)h * w;
}

int words_per_row(int w) { return (w + 31) / 32; }

bool bit_of(const uint8_t* rows, int w, int y, int x) { return (rows[(size_t)y * 4 * words_per_row(w) + (x >> 3)] >> (7 - (x & 7))) & 1; }

struct Case { std::vector<int32_t> counts; int h, w; };

// one call over the cases; bad_table: that plane's bit slice is four bytes short of its size; max_pixels_cut: the largest plane the
// call admits, 0: the largest of the cases.  Returns the number of mismatches.
int check_decode(const std::vector<Case>& cases, int bad_table, bool with_stats, int64_t max_pixels_cut) {
    const int P = (int)cases.size();
    int64_t total = 0, nbytes = 0, max_pixels = 1;
    for (const Case& c : cases) total += (int64_t)c.counts.size();
    int32_t* counts = (int32_t*)malloc(sizeof(int32_t) * (size_t)total);
    int64_t* ro = (int64_t*)malloc(sizeof(int64_t) * (P + 1));
    int64_t* bo = (int64_t*)malloc(sizeof(int64_t) * (P + 1));
    int32_t* dims = (int32_t*)malloc(sizeof(int32_t) * 2 * P);
    ro[0] = bo[0] = 0;
    for (int p = 0; p < P; ++p) {
        memcpy(counts + ro[p], cases[p].counts.data(), sizeof(int32_t) * cases[p].counts.size());
        ro[p + 1] = ro[p] + (int64_t)cases[p].counts.size();
        dims[2 * p] = cases[p].h;
        dims[2 * p + 1] = cases[p].w;
        bo[p + 1] = bo[p] + (int64_t)4 * cases[p].h * words_per_row(cases[p].w) - (p == bad_table ? 4 : 0);
        if ((int64_t)cases[p].h * cases[p].w > max_pixels) max_pixels = (int64_t)cases[p].h * cases[p].w;
    }
    nbytes = bo[P];
    if (max_pixels_cut) max_pixels = max_pixels_cut;
    uint8_t* bits = (uint8_t*)malloc((size_t)nbytes);
    memset(bits, 0xA5, (size_t)nbytes);
    int32_t* area = with_stats ? (int32_t*)malloc(sizeof(int32_t) * P) : nullptr;
    int32_t* box = with_stats ? (int32_t*)malloc(sizeof(int32_t) * 4 * P) : nullptr;
    int32_t* status = (int32_t*)malloc(sizeof(int32_t));
    const int rc = cvlm_debug_mask_rle_decode_host(counts, total, ro, dims, bo, P, max_pixels, bits, nbytes, area, box, status);
    int bad = rc != 0;
    bool any_refused = false;
    std::vector<uint8_t> px;
    for (int p = 0; p < P; ++p) {
        const int h = cases[p].h, w = cases[p].w;
        if (p == bad_table) {                                         // nothing of its slice is stored
            for (int64_t i = bo[p]; i < bo[p + 1]; ++i) bad += bits[i] != 0xA5;
            any_refused = true;
            if (with_stats) bad += area[p] != 0 || box[4 * p] != -1;
            continue;
        }
        bool good = decode_loop(cases[p].counts, h, w, px) && (int64_t)h * w <= max_pixels;
        if (!good) { px.assign((size_t)h * w, 0); any_refused = true; }
        const uint8_t* rows = bits + bo[p];
        int n = 0, x0 = w, y0 = h, x1 = -1, y1 = -1;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < 32 * words_per_row(w); ++x) {
                const bool want = x < w && px[(size_t)y * w + x];     // the pad bits are 0
                bad += bit_of(rows, w, y, x) != want;
                if (want) {
                    ++n;
                    if (x < x0) x0 = x;
                    if (y < y0) y0 = y;
                    if (x > x1) x1 = x;
                    if (y > y1) y1 = y;
                }
            }
        if (with_stats) {
            if (n == 0) bad += area[p] != 0 || box[4 * p] != -1 || box[4 * p + 1] != -1 || box[4 * p + 2] != -1 || box[4 * p + 3] != -1;
            else bad += area[p] != n || box[4 * p] != x0 || box[4 * p + 1] != y0 || box[4 * p + 2] != x1 || box[4 * p + 3] != y1;
        }
    }
    bad += status[0] != (any_refused ? 1 : 0);
    free(counts); free(ro); free(bo); free(dims); free(bits); free(area); free(box); free(status);
    return bad;
}

// slices that are no slices: the run offsets of plane 1 of three are bent; planes 0 and 2 stay whole where their own slices do
int check_slices() {
    const Plane a = make(8, 33, 8), b = make(33, 31, 8), c = make(1, 32, 4);
    const std::vector<int32_t> ca = encode(a, 0), cb = encode(b, 0), cc = encode(c, 0);
    const int64_t na = (int64_t)ca.size(), nb = (int64_t)cb.size(), nc = (int64_t)cc.size(), total = na + nb + nc;
    int bad = 0;
    for (int kind = 0; kind < 4; ++kind) {
        int32_t* counts = (int32_t*)malloc(sizeof(int32_t) * (size_t)total);
        memcpy(counts, ca.data(), sizeof(int32_t) * ca.size());
        memcpy(counts + na, cb.data(), sizeof(int32_t) * cb.size());
        memcpy(counts + na + nb, cc.data(), sizeof(int32_t) * cc.size());
        int64_t* ro = (int64_t*)malloc(sizeof(int64_t) * 4);
        ro[0] = 0; ro[1] = na; ro[2] = na + nb; ro[3] = total;
        bool first = true, second = false, third = true;
        if (kind == 0) { ro[0] = -1; first = false; second = true; }  // starts below 0
        if (kind == 1) { ro[3] = total + 1; third = false; second = true; }          // ends beyond total
        if (kind == 2) { ro[2] = ro[1]; third = false; }              // an empty slice; plane 2 then holds b's and c's counts: no plane
        if (kind == 3) { ro[2] = ro[1] - 1; third = false; }          // backwards
        const int hs[3] = {8, 33, 1}, wsz[3] = {33, 31, 32};
        int32_t dims[6];
        int64_t* bo = (int64_t*)malloc(sizeof(int64_t) * 4);
        bo[0] = 0;
        for (int p = 0; p < 3; ++p) { dims[2 * p] = hs[p]; dims[2 * p + 1] = wsz[p]; bo[p + 1] = bo[p] + 4 * hs[p] * words_per_row(wsz[p]); }
        uint8_t* bits = (uint8_t*)malloc((size_t)bo[3]);
        int32_t* dd = (int32_t*)malloc(sizeof(dims));
        memcpy(dd, dims, sizeof(dims));
        int32_t* status = (int32_t*)malloc(sizeof(int32_t));
        bad += cvlm_debug_mask_rle_decode_host(counts, total, ro, dd, bo, 3, 33 * 31, bits, bo[3], nullptr, nullptr, status) != 0;
        bad += status[0] != 1;
        const Plane* src[3] = {&a, &b, &c};
        const bool whole[3] = {first, second, third};
        for (int p = 0; p < 3; ++p)
            for (int y = 0; y < hs[p]; ++y)
                for (int x = 0; x < wsz[p]; ++x)
                    bad += bit_of(bits + bo[p], wsz[p], y, x) != (whole[p] && src[p]->px[(size_t)y * wsz[p] + x]);
        free(counts); free(ro); free(bo); free(bits); free(dd); free(status);
    }
    return bad;
}

std::vector<uint8_t> pack(const Plane& p, bool garbage) {
    const int ws = words_per_row(p.w);
    std::vector<uint8_t> rows((size_t)p.h * 4 * ws, 0);
    for (int y = 0; y < p.h; ++y)
        for (int x = 0; x < 32 * ws; ++x) {
            const bool v = x < p.w ? p.px[(size_t)y * p.w + x] != 0 : garbage && (rng() >> 9) % 2;
            if (v) rows[(size_t)y * 4 * ws + (x >> 3)] |= (uint8_t)(1u << (7 - (x & 7)));
        }
    return rows;
}

int check_inter(int h, int w, bool garbage) {
    std::vector<Plane> A, B;
    for (int k = 0; k < 4; ++k) { A.push_back(make(h, w, 7 + (k % 3))); B.push_back(make(h, w, k < 2 ? 8 : 4 + k)); }
    B.push_back(make(h + 1, w, 8));                                   // another size: every pair with it is refused
    auto table = [&](const std::vector<Plane>& ps, int short_plane, uint8_t*& bits, int64_t*& off, int32_t*& dims, int64_t& nbytes) {
        const int P = (int)ps.size();
        off = (int64_t*)malloc(sizeof(int64_t) * (P + 1));
        dims = (int32_t*)malloc(sizeof(int32_t) * 2 * P);
        off[0] = 0;
        for (int p = 0; p < P; ++p) {
            dims[2 * p] = ps[p].h; dims[2 * p + 1] = ps[p].w;
            off[p + 1] = off[p] + (int64_t)4 * ps[p].h * words_per_row(ps[p].w) - (p == short_plane ? 4 : 0);
        }
        nbytes = off[P];
        bits = (uint8_t*)malloc((size_t)nbytes);
        for (int p = 0; p < P; ++p) {
            const std::vector<uint8_t> rows = pack(ps[p], garbage);
            memcpy(bits + off[p], rows.data(), (size_t)(off[p + 1] - off[p]));
        }
    };
    uint8_t *ab, *bb;
    int64_t *ao, *bo, an, bn;
    int32_t *ad, *bd;
    table(A, -1, ab, ao, ad, an);
    table(B, 3, bb, bo, bd, bn);                                      // plane 3 of B: a slice four bytes short of its size
    const int pairs_src[][2] = {{0, 0}, {3, 2}, {1, 1}, {-1, 0}, {4, 0}, {0, 5}, {2, 4}, {0, 3}, {3, 2}, {2, 0}, {0, -7}};
    const int N = (int)(sizeof(pairs_src) / sizeof(pairs_src[0]));
    int32_t* pairs = (int32_t*)malloc(sizeof(int32_t) * 2 * N);
    memcpy(pairs, pairs_src, sizeof(int32_t) * 2 * N);
    int32_t* inter = (int32_t*)malloc(sizeof(int32_t) * N);
    int32_t* status = (int32_t*)malloc(sizeof(int32_t));
    int bad = cvlm_debug_mask_inter_sized_host(ab, an, ao, ad, (int)A.size(), bb, bn, bo, bd, (int)B.size(), pairs, N, (int64_t)h * words_per_row(w),
                                               inter, status) != 0;
    bad += status[0] != 1;
    for (int i = 0; i < N; ++i) {
        const int a = pairs_src[i][0], b = pairs_src[i][1];
        int want = -1;
        if (a >= 0 && a < (int)A.size() && b >= 0 && b < (int)B.size() && b != 3 && B[b].h == h) {
            want = 0;
            for (size_t j = 0; j < A[a].px.size(); ++j) want += A[a].px[j] && B[b].px[j];
        }
        bad += inter[i] != want;
    }
    free(ab); free(ao); free(ad); free(bb); free(bo); free(bd); free(pairs); free(inter); free(status);
    return bad;
}

}  // namespace

int main() {
    const int shapes[][2] = {{1, 1}, {1, 31}, {1, 32}, {8, 33}, {33, 31}, {32, 63}, {33, 65}, {65, 97}, {130, 517}};
    int bad = 0;
    std::vector<Case> ragged;
    for (const auto& s : shapes) {
        for (int zeros = -1; zeros <= 3; ++zeros) {                   // a trailing 0, none, one, two, three in a row
            std::vector<Case> cases;
            for (int kind = 0; kind < 10; ++kind) cases.push_back({encode(make(s[0], s[1], kind), zeros), s[0], s[1]});
            bad += check_decode(cases, -1, true, 0);
            if (zeros == 0) ragged.push_back(cases[4 + (s[0] + s[1]) % 6]);
        }
    }
    bad += check_decode(ragged, -1, true, 0);
    bad += check_decode(ragged, -1, false, 0);
    bad += check_decode(ragged, 4, true, 0);                      // a table that does not fit
    bad += check_decode(ragged, 0, true, 0);
    bad += check_decode(ragged, -1, true, 33 * 65);               // the larger planes do not fit max_pixels
    bad += check_decode({{{0, 0, 6}, 2, 3}, {{0, 6}, 2, 3}, {{6, 0}, 2, 3}}, -1, true, 0);
    // counts that describe no plane, between planes that are whole
    const Case whole{encode(make(8, 33, 8), 0), 8, 33};
    std::vector<int32_t> neg = whole.counts, one_short = whole.counts, one_long = whole.counts;
    neg.back() += 1; neg.push_back(-1);
    one_short.back() -= 1;
    one_long.back() += 1;
    for (const std::vector<int32_t>& c : {neg, one_short, one_long, std::vector<int32_t>{1 << 30, 1 << 30}, std::vector<int32_t>{1 << 30, 1 << 30, 1 << 30, (1 << 30) + 4}})
        bad += check_decode({whole, {c, c.size() > 4 ? 8 : 2, c.size() > 4 ? 33 : 2}, whole}, -1, true, 0);
    bad += check_slices();
    const int inter_shapes[][2] = {{1, 1}, {1, 32}, {33, 31}, {97, 131}, {480, 641}};
    for (const auto& s : inter_shapes)
        for (int garbage = 0; garbage < 2; ++garbage) bad += check_inter(s[0], s[1], garbage != 0);
    printf("gt_host_sanitize: %d mismatches\n", bad);
    return bad != 0;
}
