// Stand-alone check of cvlm_debug_mask_nms_inter_host and cvlm_debug_mask_nms_host for a host sanitizer: the entries'
// per-thread functions are the kernels' (csrc/nms_logic.h), so their indexing is what runs on the device.  Every buffer is a heap block
// of exactly the size the interface states, so that AddressSanitizer sees any access beyond it.  Ragged plane sizes, every pad bit
// dirty, groups interleaved in the planes' order; the intersections are held against a per-pixel loop inside the two boxes, the NMS
// against the textbook greedy loop and the Matrix NMS formulas written out plainly.  Refusals -- a box out of order or outside its
// plane, a size that differs, a slice that is not the plane's; offsets that run backwards, a member outside the rows, a pair block that
// is not the triangle -- each at the first, a middle and the last position, through the same exact-size buffers.
// Build and run on the CPU, from the repository root:
//   hipcc -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/nms_host_sanitize.cpp camouflaged-vlm_amd/csrc/nms.hip -o /tmp/nms_host_sanitize && /tmp/nms_host_sanitize
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#include "../include/cvlm.h"

#pragma clang fp contract(off)

namespace {

uint32_t rng_state = 3030u;
uint32_t rng() { return rng_state = rng_state * 1664525u + 1013904223u; }
int below(int n) { return (int)((rng() >> 8) % (uint32_t)n); }

int failures = 0;
#define EXPECT(c) do { if (!(c)) { ++failures; printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

template <class T> T* exact(const std::vector<T>& v) {             // a heap block of exactly v.size() elements (NULL for none)
    if (v.empty()) return nullptr;
    T* p = (T*)malloc(v.size() * sizeof(T));
    memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}
template <class T> T* blank(size_t n) { return n ? (T*)malloc(n * sizeof(T)) : nullptr; }

struct Plane {
    int h, w, image, area = 0, box[4] = {-1, -1, -1, -1}, cat;
    float score;
    std::vector<uint8_t> px;                                          // h * w
};

Plane make_plane(int h, int w, int image, int kind) {
    Plane p;
    p.h = h; p.w = w; p.image = image; p.cat = below(3);
    const float special[] = {std::numeric_limits<float>::quiet_NaN(), 0.5f, 0.5f, 0.25f, 1.0f};
    p.score = kind == 2 ? special[below(5)] : below(8) / 8.0f;
    p.px.assign((size_t)h * w, 0);
    if (kind != 3) {                                                  // kind 3: an empty instance
        const int y0 = below(h), x0 = below(w), y1 = y0 + below(h - y0), x1 = x0 + below(w - x0);
        unsigned x_lo = 0xffffffffu, y_lo = 0xffffffffu;
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x)
                if (below(8)) {
                    p.px[(size_t)y * w + x] = 1;
                    ++p.area;
                    x_lo = std::min(x_lo, (unsigned)x); y_lo = std::min(y_lo, (unsigned)y);
                    p.box[2] = std::max(p.box[2], x); p.box[3] = std::max(p.box[3], y);
                }
        if (p.area) { p.box[0] = (int)x_lo; p.box[1] = (int)y_lo; }
    }
    return p;
}

struct Doctor { int what = 0, at = 0; };   // 1 box order, 2 box outside, 3 half-empty box, 4 size, 5 slice; 6 .. 9 a group: see run

// one call of both entries on the planes; the groups are the images, their members in plane order
void run(std::vector<Plane> planes, int measure, int method, double thr, double sigma, bool class_aware, Doctor doc) {
    const int Q = (int)planes.size();
    std::vector<uint8_t> bits;
    std::vector<int64_t> off(1, 0);
    std::vector<int32_t> dims, area, box, cat;
    std::vector<float> score;
    for (const Plane& p : planes) {
        const int ws = (p.w + 31) / 32;
        std::vector<uint8_t> rows((size_t)p.h * ws * 4, 0);
        for (int y = 0; y < p.h; ++y)
            for (int x = 0; x < 32 * ws; ++x)
                if (x < p.w ? p.px[(size_t)y * p.w + x] : (uint8_t)below(2)) rows[((size_t)y * ws * 32 + x) >> 3] |= (uint8_t)(0x80u >> (x & 7));
        bits.insert(bits.end(), rows.begin(), rows.end());
        off.push_back((int64_t)bits.size());
        dims.push_back(p.h); dims.push_back(p.w);
        area.push_back(p.area);
        box.insert(box.end(), p.box, p.box + 4);
        cat.push_back(p.cat);
        score.push_back(p.score);
    }
    int n_images = 0;
    for (const Plane& p : planes) n_images = std::max(n_images, p.image + 1);
    std::vector<std::vector<int>> rows((size_t)n_images);
    for (int q = 0; q < Q; ++q) rows[(size_t)planes[q].image].push_back(q);
    const int G = n_images;
    std::vector<int32_t> goff(1, 0), member;
    std::vector<int64_t> poff(1, 0);
    for (const auto& r : rows) {
        member.insert(member.end(), r.begin(), r.end());
        goff.push_back((int32_t)member.size());
        poff.push_back(poff.back() + (int64_t)r.size() * ((int64_t)r.size() - 1) / 2);
    }
    member.resize((size_t)Q, 0);
    const int64_t N = poff.back();
    // the doctoring: planes of the LARGEST group (first, middle, last member), or that group's table entries
    int big = 0;
    for (int g = 0; g < G; ++g)
        if (rows[(size_t)g].size() > rows[(size_t)big].size()) big = g;
    const std::vector<int>& br = rows[(size_t)big];
    const int victim = doc.what ? br[doc.at == 0 ? 0 : doc.at == 1 ? br.size() / 2 : br.size() - 1] : -1;
    std::vector<int> bad_groups;
    if (doc.what == 1) std::swap(box[4 * victim], box[4 * victim + 2]), box[4 * victim] += 1;
    if (doc.what == 2) box[4 * victim + 3] = planes[(size_t)victim].h;
    if (doc.what == 3) { box[4 * victim] = box[4 * victim + 1] = box[4 * victim + 2] = -1; box[4 * victim + 3] = 0; }
    if (doc.what == 4) dims[2 * victim + 1] += 1;
    if (doc.what == 5) off[(size_t)victim] += victim ? 4 : -4;
    if (doc.what == 6) { member[(size_t)goff[(size_t)big] + (doc.at == 0 ? 0 : doc.at == 1 ? br.size() / 2 : br.size() - 1)] = doc.at == 1 ? -1 : Q; bad_groups = {big}; }
    if (doc.what == 7) { goff[(size_t)big + 1] = goff[(size_t)big] - 1; bad_groups = {big, big + 1}; }
    if (doc.what == 8) { poff[(size_t)big + 1] += 1; bad_groups = {big, big + 1}; }
    if (doc.what == 9) { poff[(size_t)big] = -1; bad_groups = {big, big - 1}; }
    auto group_bad = [&](int g) { return std::find(bad_groups.begin(), bad_groups.end(), g) != bad_groups.end() && g >= 0 && g < G; };
    auto plane_bad = [&](int q) {
        if (doc.what < 1 || doc.what > 5) return false;
        return q == victim || (doc.what == 5 && victim > 0 && q == victim - 1);    // a moved offset is the end of the plane before
    };

    uint8_t* p_bits = exact(bits);
    int64_t *p_off = exact(off), *p_poff = exact(poff);
    int32_t *p_dims = exact(dims), *p_area = exact(area), *p_box = exact(box), *p_goff = exact(goff), *p_member = exact(member), *p_cat = exact(cat);
    float* p_score = exact(score);
    int32_t *inter = blank<int32_t>((size_t)N), *status = blank<int32_t>(1), *order = blank<int32_t>(Q), *by = blank<int32_t>(Q), *n_keep = blank<int32_t>(G);
    uint8_t* keep = blank<uint8_t>(Q);
    float* decay = blank<float>(Q);
    double* params = blank<double>(2);
    params[0] = thr; params[1] = sigma;
    int rc = cvlm_debug_mask_nms_inter_host(p_bits, (int64_t)bits.size(), p_off, p_dims, p_area, p_box, Q, p_goff, p_member, p_poff, G, N, inter, status);
    EXPECT(rc == 0);
    bool any_pair_bad = false;
    std::vector<int> want_inter((size_t)N, -1);
    if (rc == 0) {
        for (int g = 0; g < G; ++g) {
            if (group_bad(g)) continue;
            const std::vector<int>& r = rows[(size_t)g];
            const int D = (int)r.size();
            int64_t t = poff[(size_t)g];
            for (int i = 0; i < D; ++i)
                for (int j = i + 1; j < D; ++j, ++t) {
                    const Plane &a = planes[(size_t)r[i]], &b = planes[(size_t)r[j]];
                    int n = 0;
                    if (plane_bad(r[i]) || plane_bad(r[j]) || a.h != b.h || a.w != b.w) { n = -1; any_pair_bad = true; }
                    else if (a.area && b.area)
                        for (int y = std::max(a.box[1], b.box[1]); y <= std::min(a.box[3], b.box[3]); ++y)
                            for (int x = std::max(a.box[0], b.box[0]); x <= std::min(a.box[2], b.box[2]); ++x)
                                n += a.px[(size_t)y * a.w + x] & b.px[(size_t)y * a.w + x];
                    want_inter[(size_t)t] = n;
                    EXPECT(inter[t] == n);
                }
        }
        if (!bad_groups.empty())
            for (int64_t t = 0; t < N; ++t) EXPECT(inter[t] == want_inter[(size_t)t]);        // nothing of a refused group's block stored
        EXPECT(status[0] == ((any_pair_bad ? 1 : 0) | (bad_groups.empty() ? 0 : 2)));
    }
    rc = cvlm_debug_mask_nms_host(p_goff, p_member, p_poff, G, inter, N, p_area, p_score, class_aware ? p_cat : nullptr, Q, measure, method, params,
                                  order, keep, by, decay, n_keep, status);
    EXPECT(rc == 0);
    if (rc == 0) {
        EXPECT(status[0] == (bad_groups.empty() ? 0 : 2));
        for (int g = 0; g < G; ++g) {
            const std::vector<int>& r = rows[(size_t)g];
            const int D = (int)r.size();
            if (group_bad(g)) {
                EXPECT(n_keep[g] == 0);
                if (doc.what != 7)                                    // with doctored row offsets the rows belong to nobody we can name
                    for (int q : r) EXPECT(keep[q] == 0 && by[q] == -1 && decay[q] == 0.0f);
                continue;
            }
            auto m_of = [&](int x, int y) {                           // places in r
                const int lo = std::min(x, y), hi = std::max(x, y);
                const int in = want_inter[(size_t)(poff[(size_t)g] + (int64_t)lo * D - (int64_t)lo * (lo + 1) / 2 + (hi - lo - 1))];
                const int ax = area[(size_t)r[x]], ay = area[(size_t)r[y]];
                if (class_aware && cat[(size_t)r[x]] != cat[(size_t)r[y]]) return 0.0;
                if (in < 0) return -1.0;
                if (in == 0) return 0.0;
                const int64_t den = measure == 0 ? (int64_t)ax + ay - in : std::min(ax, ay);
                return den < 1 ? -1.0 : (double)in / (double)den;
            };
            std::vector<int> ord(D);
            std::iota(ord.begin(), ord.end(), 0);
            std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) {
                const float sx = score[(size_t)r[x]], sy = score[(size_t)r[y]];
                if (std::isnan(sx) || std::isnan(sy)) return !std::isnan(sx) && std::isnan(sy);
                return sx > sy;
            });
            for (int k = 0; k < D; ++k) EXPECT(order[goff[(size_t)g] + k] == r[ord[k]]);
            int kept = 0;
            if (method == 0) {
                std::vector<int> gone(D, 0), sup(D, -1);
                for (int k = 0; k < D; ++k) {
                    const int i = ord[k];
                    if (gone[i] || area[(size_t)r[i]] < 1) continue;
                    for (int s = k + 1; s < D; ++s)
                        if (!gone[ord[s]] && m_of(i, ord[s]) > thr) { gone[ord[s]] = 1; sup[ord[s]] = r[i]; }
                }
                for (int k = 0; k < D; ++k) {
                    const bool live = !gone[k] && area[(size_t)r[k]] >= 1;
                    kept += live;
                    EXPECT(keep[r[k]] == (live ? 1 : 0) && by[r[k]] == sup[k] && decay[r[k]] == (live ? 1.0f : 0.0f));
                }
            } else {
                std::vector<double> c(D, 0.0);
                for (int s = 0; s < D; ++s)
                    for (int t = 0; t < s; ++t) c[s] = std::max(c[s], std::max(0.0, m_of(ord[t], ord[s])));
                for (int s = 0; s < D; ++s) {
                    double d = 1.0;
                    for (int t = 0; t < s; ++t) {
                        const double m = std::max(0.0, m_of(ord[t], ord[s]));
                        const double v = method == 1 ? (1.0 - c[t] == 0.0 ? 1.0 : (1.0 - m) / (1.0 - c[t])) : exp(-sigma * (m * m - c[t] * c[t]));
                        d = std::min(d, v);
                    }
                    const int q = r[ord[s]];
                    kept += area[(size_t)q] >= 1;
                    EXPECT(keep[q] == (area[(size_t)q] >= 1 ? 1 : 0) && by[q] == -1);
                    if (method == 1) EXPECT(decay[q] == (float)d);
                    else EXPECT(fabs((double)decay[q] - (double)(float)d) <= ldexp(fabs((double)(float)d), -23));
                }
            }
            EXPECT(n_keep[g] == kept);
        }
    }
    for (void* p : {(void*)p_bits, (void*)p_off, (void*)p_poff, (void*)p_dims, (void*)p_area, (void*)p_box, (void*)p_goff, (void*)p_member, (void*)p_cat,
                    (void*)p_score, (void*)inter, (void*)status, (void*)order, (void*)by, (void*)n_keep, (void*)keep, (void*)decay, (void*)params})
        free(p);
}

// images of ragged sizes, their instances interleaved; image 1 is the largest group
std::vector<Plane> scene(int scale) {
    const int shapes[][3] = {{1, 1, 1}, {5, 33, 9}, {7, 31, 4}, {3, 70, 3}, {40, 65, 5}, {1, 32, 2}};
    std::vector<Plane> out;
    for (int round = 0; round < 9 * scale; ++round)
        for (int g = 0; g < 6; ++g)
            if (round < shapes[g][2] * scale) out.push_back(make_plane(shapes[g][0], shapes[g][1], g, (round + g) % 4));
    return out;
}

}  // namespace

int main() {
    int calls = 0;
    for (int measure = 0; measure < 2; ++measure)
        for (int method = 0; method < 3; ++method)
            for (int aware = 0; aware < 2; ++aware, ++calls) run(scene(1 + method), measure, method, measure ? 0.7 : 0.3, 0.5 + method, aware != 0, Doctor());
    run(scene(8), 0, 0, 0.5, 2.0, false, Doctor());                  // a group of 72, past a wave
    run({make_plane(4, 4, 0, 0)}, 0, 0, 0.5, 2.0, false, Doctor());   // N = 0: inter is NULL
    calls += 2;
    for (int what = 1; what <= 9; ++what)
        for (int at = 0; at < (what <= 6 ? 3 : 1); ++at, ++calls) {
            Doctor d;
            d.what = what; d.at = at;
            run(scene(1), what & 1, what % 3, 0.4, 1.5, (what & 2) != 0, d);
        }
    // every refused argument, on valid tables
    {
        int32_t goff[2] = {0, 1}, member[1] = {0}, dims[2] = {1, 1}, area[1] = {1}, box[4] = {0, 0, 0, 0}, inter[1], status[1], order[1], by[1], n_keep[1];
        int64_t off[2] = {0, 4}, poff[2] = {0, 0};
        alignas(8) uint8_t bits[4] = {0x80, 0, 0, 0};
        uint8_t keep[1];
        float score[1] = {0.5f}, decay[1];
        double params[2] = {0.5, 2.0};
        const double nan = std::numeric_limits<double>::quiet_NaN();
        EXPECT(cvlm_debug_mask_nms_inter_host(bits, 4, off, dims, area, box, 1, goff, member, poff, 1, 0, nullptr, status) == 0);
        EXPECT(cvlm_debug_mask_nms_host(goff, member, poff, 1, nullptr, 0, area, score, nullptr, 1, 0, 0, params, order, keep, by, decay, n_keep, status) == 0);
        EXPECT(keep[0] == 1 && order[0] == 0 && n_keep[0] == 1 && decay[0] == 1.0f);
        EXPECT(cvlm_debug_mask_nms_inter_host(bits, 3, off, dims, area, box, 1, goff, member, poff, 1, 0, nullptr, status) == CVLM_E_BADARG);
        EXPECT(cvlm_debug_mask_nms_inter_host(bits, 4, off, dims, area, box, 0, goff, member, poff, 1, 0, nullptr, status) == CVLM_E_BADARG);
        EXPECT(cvlm_debug_mask_nms_inter_host(bits, 4, off, dims, area, box, 1, goff, member, poff, 0, 0, nullptr, status) == CVLM_E_BADARG);
        EXPECT(cvlm_debug_mask_nms_inter_host(bits, 4, off, dims, area, box, 1, goff, member, poff, 1, 1, nullptr, status) == CVLM_E_BADARG);
        EXPECT(cvlm_debug_mask_nms_inter_host(bits, 4, off, dims, area, box, 1, goff, member, poff, 1, -1, inter, status) == CVLM_E_BADARG);
        EXPECT(cvlm_debug_mask_nms_inter_host(bits, 4, off, dims, area, box, 1, goff, member, poff, 1, 1, area, status) == CVLM_E_BADARG);
        EXPECT(cvlm_debug_mask_nms_inter_host(bits, 4, off, dims, area, (int32_t*)((char*)box + 2), 1, goff, member, poff, 1, 0, nullptr, status) == CVLM_E_BADARG);
        for (int k = 0; k < 5; ++k) {
            double p[2] = {k == 0 ? -0.1 : k == 1 ? 1.1 : k == 2 ? nan : 0.5, k == 3 ? 0.0 : k == 4 ? nan : 2.0};
            EXPECT(cvlm_debug_mask_nms_host(goff, member, poff, 1, nullptr, 0, area, score, nullptr, 1, 0, 2, p, order, keep, by, decay, n_keep, status) == CVLM_E_BADARG);
        }
        EXPECT(cvlm_debug_mask_nms_host(goff, member, poff, 1, nullptr, 0, area, score, nullptr, 1, 2, 0, params, order, keep, by, decay, n_keep, status) == CVLM_E_BADARG);
        EXPECT(cvlm_debug_mask_nms_host(goff, member, poff, 1, nullptr, 0, area, score, nullptr, 1, 0, 3, params, order, keep, by, decay, n_keep, status) == CVLM_E_BADARG);
        EXPECT(cvlm_debug_mask_nms_host(goff, member, poff, 1, nullptr, 0, area, score, nullptr, 1, 0, 0, nullptr, order, keep, by, decay, n_keep, status) == CVLM_E_BADARG);
        EXPECT(cvlm_debug_mask_nms_host(goff, member, poff, 1, nullptr, 0, area, score, nullptr, 1, 0, 0, params, order, keep, order, decay, n_keep, status) == CVLM_E_BADARG);
        EXPECT(cvlm_debug_mask_nms_host(goff, member, poff, 1, nullptr, 0, area, score, nullptr, 1, 0, 0, params, order, keep, by, (float*)score, n_keep, status) == CVLM_E_BADARG);
    }
    printf("nms_host_sanitize: %d calls and every refused argument: %s\n", calls, failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
