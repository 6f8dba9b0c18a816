// Stand-alone check of cvlm_debug_coco_match_host for a host sanitizer: the entry's per-thread functions are the
// kernel's (csrc/match_logic.h), so their indexing is what runs on the device.  Every buffer is a heap block of exactly the size the
// interface states, so that AddressSanitizer sees any access beyond it; the matches are held against the published loop of
// COCOeval.evaluateImg written out plainly: the annotations stably sorted ignore-last, the break, the last candidate that is at
// least as good.  Refused groups -- offsets that run backwards or leave the tables, a pair block of the wrong length or outside the
// table, more than 1024 rows -- run through the same exact-size buffers and must leave the fill.
// Build and run on the CPU, from the repository root:
//   hipcc -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/match_host_sanitize.cpp camouflaged-vlm_amd/csrc/match.hip -o /tmp/match_host_sanitize && /tmp/match_host_sanitize
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

uint32_t rng_state = 2222u;
uint32_t rng() { return rng_state = rng_state * 1664525u + 1013904223u; }
int below(int n) { return (int)((rng() >> 8) % (uint32_t)n); }

struct Group {
    int D, G;
    std::vector<int> inter, det_area, gt_area;
    std::vector<float> score;
    std::vector<double> range_area;
    std::vector<uint8_t> crowd;
};

Group make_group(int D, int G, int kind) {
    Group q;
    q.D = D; q.G = G;
    const float special[] = {std::numeric_limits<float>::quiet_NaN(), INFINITY, -INFINITY, -0.0f, 0.0f, 0.25f, 1.0f};
    for (int d = 0; d < D; ++d) {
        q.det_area.push_back(1 + below(40));
        q.score.push_back(kind == 0 ? below(4) / 4.0f : kind == 1 ? 0.5f : special[below(7)]);
    }
    for (int g = 0; g < G; ++g) {
        q.gt_area.push_back(1 + below(40));
        q.crowd.push_back(below(4) == 0);
        q.range_area.push_back(kind == 1 ? 12.5 * below(4) : (double)q.gt_area.back());
    }
    for (int d = 0; d < D; ++d)
        for (int g = 0; g < G; ++g) q.inter.push_back(kind == 2 && below(50) == 0 ? -1 : below(std::min(q.det_area[d], q.gt_area[g]) + 1));
    return q;
}

template <class T> T* exact(const std::vector<T>& v) {             // a heap block of exactly v.size() elements (NULL for none)
    if (v.empty()) return nullptr;
    T* p = (T*)malloc(v.size() * sizeof(T));
    memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}
template <class T> T* blank(size_t n) { return n ? (T*)malloc(n * sizeof(T)) : nullptr; }

bool before(float sj, int j, float si, int i) {                      // numpy.argsort(-score, kind="mergesort")
    const bool nj = std::isnan(sj), ni = std::isnan(si);
    if (nj || ni) return nj == ni ? j < i : ni;
    return sj > si || (sj == si && j < i);
}

int failures = 0;
#define EXPECT(c) do { if (!(c)) { ++failures; printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

// one call on the groups; doctor: a change of the offset tables after they are built (index < 0: none); refused: which groups must hold the fill
void run(const std::vector<Group>& groups, const std::vector<double>& thrs, const std::vector<double>& rngs, int max_det, int table, int index,
         int64_t value, const std::vector<int>& refused) {
    const int E = (int)groups.size(), T = (int)thrs.size(), A = (int)rngs.size() / 2;
    std::vector<int32_t> d_off(1, 0), g_off(1, 0), inter, det_area, gt_area;
    std::vector<int64_t> p_off(1, 0);
    std::vector<float> score;
    std::vector<double> range_area;
    std::vector<uint8_t> crowd;
    for (const Group& q : groups) {
        d_off.push_back(d_off.back() + q.D);
        g_off.push_back(g_off.back() + q.G);
        p_off.push_back(p_off.back() + (int64_t)q.D * q.G);
        inter.insert(inter.end(), q.inter.begin(), q.inter.end());
        det_area.insert(det_area.end(), q.det_area.begin(), q.det_area.end());
        gt_area.insert(gt_area.end(), q.gt_area.begin(), q.gt_area.end());
        score.insert(score.end(), q.score.begin(), q.score.end());
        range_area.insert(range_area.end(), q.range_area.begin(), q.range_area.end());
        crowd.insert(crowd.end(), q.crowd.begin(), q.crowd.end());
    }
    const int ND = d_off.back(), NG = g_off.back();
    const int64_t N = p_off.back();
    const std::vector<int32_t> d_true = d_off, g_true = g_off;
    if (index >= 0) {
        if (table == 0) d_off[index] = (int32_t)value;
        if (table == 1) g_off[index] = (int32_t)value;
        if (table == 2) p_off[index] = value;
    }
    int32_t *pd = exact(d_off), *pg = exact(g_off), *pi = exact(inter), *pda = exact(det_area), *pga = exact(gt_area);
    int64_t* pp = exact(p_off);
    float* ps = exact(score);
    double *pra = exact(range_area), *pt = exact(thrs), *pr = exact(rngs);
    uint8_t* pc = exact(crowd);
    int32_t *order = blank<int32_t>(ND), *dtm = blank<int32_t>((size_t)A * T * ND), *gtm = blank<int32_t>((size_t)A * T * NG), *status = blank<int32_t>(1);
    uint8_t *dti = blank<uint8_t>((size_t)A * T * ND), *gti = blank<uint8_t>((size_t)A * NG);
    const int rc = cvlm_debug_coco_match_host(pd, pg, pp, E, pi, N, pda, ps, ND, pga, pra, pc, NG, pt, T, pr, A, max_det, order, dtm, dti, gtm, gti,
                                              status);
    EXPECT(rc == 0);
    if (rc == 0) {
        EXPECT(status[0] == (refused.empty() ? 0 : 1));
        for (int e = 0; e < E; ++e) {
            const Group& q = groups[e];
            const int d0 = d_true[e], g0 = g_true[e];
            if (std::find(refused.begin(), refused.end(), e) != refused.end()) {
                for (int d = 0; d < q.D; ++d) EXPECT(order[d0 + d] == -1);
                for (int at = 0; at < A * T; ++at) {
                    for (int d = 0; d < q.D; ++d) EXPECT(dtm[(size_t)at * ND + d0 + d] == -1 && dti[(size_t)at * ND + d0 + d] == 1);
                    for (int g = 0; g < q.G; ++g) EXPECT(gtm[(size_t)at * NG + g0 + g] == -1);
                }
                for (int a = 0; a < A; ++a)
                    for (int g = 0; g < q.G; ++g) EXPECT(gti[(size_t)a * NG + g0 + g] == 1);
                continue;
            }
            std::vector<int> dtind(q.D);
            std::iota(dtind.begin(), dtind.end(), 0);
            std::stable_sort(dtind.begin(), dtind.end(), [&](int x, int y) { return x != y && before(q.score[x], x, q.score[y], y); });
            for (int r = 0; r < q.D; ++r) EXPECT(order[d0 + r] == d0 + dtind[r]);
            const int R = std::min(q.D, max_det);
            for (int a = 0; a < A; ++a) {
                const double lo = rngs[2 * a], hi = rngs[2 * a + 1];
                std::vector<int> ig(q.G), gtind(q.G);
                for (int g = 0; g < q.G; ++g) {
                    ig[g] = q.crowd[g] || q.range_area[g] < lo || q.range_area[g] > hi;
                    EXPECT(gti[(size_t)a * NG + g0 + g] == ig[g]);
                }
                std::iota(gtind.begin(), gtind.end(), 0);
                std::stable_sort(gtind.begin(), gtind.end(), [&](int x, int y) { return ig[x] < ig[y]; });
                for (int t = 0; t < T; ++t) {
                    const size_t at = (size_t)a * T + t;
                    std::vector<int> gm(q.G, -1);                     // per sorted annotation: the detection that took it
                    for (int r = 0; r < q.D; ++r) {
                        int want_m = -1, want_ig = 1;
                        if (r < R) {
                            const int d = dtind[r];
                            double iou = std::min(thrs[t], 1 - 1e-10);
                            int m = -1;
                            for (int k = 0; k < q.G; ++k) {
                                const int g = gtind[k];
                                if (gm[k] >= 0 && !q.crowd[g]) continue;
                                if (m > -1 && !ig[gtind[m]] && ig[g]) break;
                                const int in = q.inter[(size_t)d * q.G + g];
                                double v = 0.0;
                                if (in < 0) v = -1.0;
                                else if (in > 0) v = (double)in / (double)(q.crowd[g] ? q.det_area[d] : q.det_area[d] + q.gt_area[g] - in);
                                if (v < iou) continue;
                                iou = v;
                                m = k;
                            }
                            if (m >= 0) {
                                gm[m] = d;
                                want_m = g0 + gtind[m];
                                want_ig = ig[gtind[m]];
                            } else {
                                want_ig = q.det_area[d] < lo || q.det_area[d] > hi;
                            }
                        }
                        EXPECT(dtm[at * ND + d0 + r] == want_m);
                        EXPECT(dti[at * ND + d0 + r] == want_ig);
                    }
                    for (int k = 0; k < q.G; ++k) EXPECT(gtm[at * NG + g0 + gtind[k]] == (gm[k] >= 0 ? d0 + gm[k] : -1));
                }
            }
        }
    }
    for (void* p : {(void*)pd, (void*)pg, (void*)pi, (void*)pda, (void*)pga, (void*)pp, (void*)ps, (void*)pra, (void*)pt, (void*)pr, (void*)pc,
                    (void*)order, (void*)dtm, (void*)gtm, (void*)status, (void*)dti, (void*)gti})
        free(p);
}

}  // namespace

int main() {
    const std::vector<double> ten = {0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9 - 1.1102230246251565e-16, 0.95};
    const std::vector<double> small = {0, 1e10, 0, 15, 15, 25, 25, 1e10};
    const std::vector<double> eight = {0, 1e10, 0, 15, 15, 25, 25, 1e10, 10, 30, 0, 0, 40, 40, 5, 1e10};
    const std::vector<double> sixteen = {0.05, 0.1, 0.25, 1.0 / 3, 0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95, 0.99, 1.0};
    const int shapes[][3] = {{0, 3, 100}, {3, 0, 100}, {0, 0, 100}, {1, 1, 100}, {5, 4, 100}, {7, 3, 3}, {33, 31, 100}, {64, 65, 100}, {130, 70, 100}};
    int calls = 0;
    for (const auto& s : shapes)
        for (int kind = 0; kind < 3; ++kind, ++calls) run({make_group(s[0], s[1], kind)}, ten, small, s[2], 0, -1, 0, {});
    run({make_group(33, 31, 0)}, {0.5}, {0, 1e10}, 100, 0, -1, 0, {});
    run({make_group(64, 65, 2), make_group(5, 4, 1)}, sixteen, eight, 100, 0, -1, 0, {});
    std::vector<Group> ragged;
    for (int e = 0; e < 37; ++e) ragged.push_back(make_group(e % 5 ? below(40) : 0, e % 7 ? below(40) : 0, e % 3));
    run(ragged, ten, small, 20, 0, -1, 0, {});
    calls += 3;
    // refusals: three groups of 5 x 4, 6 x 3, 4 x 4 -- detection offsets 0 5 11 15, annotation offsets 0 4 7 11, pair offsets 0 20 38 54
    const std::vector<Group> three = {make_group(5, 4, 0), make_group(6, 3, 1), make_group(4, 4, 2)};
    run(three, ten, small, 100, 0, 1, 12, {0, 1});
    run(three, ten, small, 100, 1, 3, 12, {2});
    run(three, ten, small, 100, 0, 0, -1, {0});
    run(three, ten, small, 100, 2, 2, 37, {1, 2});
    run(three, ten, small, 100, 2, 3, 55, {2});
    run(three, ten, small, 100, 2, 0, -1, {0});
    run({make_group(1025, 1, 0), make_group(2, 2, 0)}, ten, small, 100, 0, -1, 0, {0});
    run({make_group(2, 2, 0), make_group(1, 1025, 0)}, ten, small, 100, 0, -1, 0, {1});
    calls += 8;
    printf("%d calls, %d failures\n", calls, failures);
    return failures ? 1 : 0;
}
