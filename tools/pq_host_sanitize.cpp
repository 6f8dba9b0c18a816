// Stand-alone check of the cvlm_debug_pan_*_host entries for a host sanitizer: their per-thread functions are the
// kernels' (csrc/panoptic_logic.h), so their indexing is what runs on the device.  Every buffer is a heap block of exactly the size the
// interface states, so that AddressSanitizer sees any access beyond it.  Ragged images -- (1, 1), one row, widths around the unit of 64
// pixels --, raw ids as int32 and as RGB bytes (an RGB block has no alignment: it starts one byte into its allocation), tables of one
// key and of many, ids the tables lack; the pair counts, the matching and the totals against a plain restatement of the definition,
// with crowd slots, unused slots, void, slots without a pixel and categories outside the classes; two batches summed; refused tables --
// a size of 0, a slice longer than its size, an image beyond the maps, a key slice beyond the keys --, which must leave their image's
// outputs alone; every refusal of every entry.
// Build and run on the CPU, from the repository root:
//   hipcc -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/pq_host_sanitize.cpp camouflaged-vlm_amd/csrc/panoptic.hip -o /tmp/pq_host_sanitize && /tmp/pq_host_sanitize
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>                                         // the shared headers' device halves, when hipcc compiles this file
#endif

#include "../include/cvlm.h"
#include "../camouflaged-vlm_amd/csrc/panoptic_logic.h"

namespace {

uint32_t rng_state = 2424u;
uint32_t rng() { return rng_state = rng_state * 1664525u + 1013904223u; }
int below(int n) { return (int)((rng() >> 8) % (uint32_t)n); }

template <class T> T* block(size_t n) { return (T*)malloc((n ? n : 1) * sizeof(T)); }     // exactly n elements (1 where n is 0)
template <class T> T* block_of(const std::vector<T>& v) { T* p = block<T>(v.size()); if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T)); return p; }

int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

const int SIZES[7][2] = {{1, 1}, {70, 33}, {5, 65}, {33, 31}, {1, 32}, {97, 131}, {2, 64}};

struct Tables {
    int B;
    int32_t* dims; int64_t* off; int64_t n_pix, max_pixels;
    explicit Tables(int B_) : B(B_) {
        dims = block<int32_t>(2 * B); off = block<int64_t>(B + 1);
        off[0] = 0; max_pixels = 1;
        for (int b = 0; b < B; ++b) {
            dims[2 * b] = SIZES[b % 7][0]; dims[2 * b + 1] = SIZES[b % 7][1];
            const int64_t n = (int64_t)dims[2 * b] * dims[2 * b + 1];
            off[b + 1] = off[b] + n; max_pixels = std::max(max_pixels, n);
        }
        n_pix = off[B];
    }
    ~Tables() { free(dims); free(off); }
};

// a piecewise-constant map over [0, n): runs of random length along the rows
void fill_map(int32_t* m, int64_t n_pix, int n) {
    for (int64_t i = 0; i < n_pix;) {
        const int v = below(n), run = 1 + below(40);
        for (int k = 0; k < run && i < n_pix; ++k) m[i++] = v;
    }
}

// ---- remap ----------------------------------------------------------------------------------------------------------------------------------
void remap_cases() {
    const int B = 7;
    Tables t(B);
    // image b lists 1 + 150 * (b % 3) ids, every third id of its range; the maps hold ids of the whole range and 0
    std::vector<int32_t> keys, vals; std::vector<int64_t> tab(1, 0);
    for (int b = 0; b < B; ++b) {
        const int n = 1 + 150 * (b % 3);
        for (int i = 0; i < n; ++i) { keys.push_back(70000 * b + 5 + 3 * i); vals.push_back(1 + (i * 7) % n); }
        tab.push_back((int64_t)keys.size());
    }
    int32_t* raw = block<int32_t>(t.n_pix);
    uint8_t* rgb_base = block<uint8_t>(3 * t.n_pix + 1);
    uint8_t* rgb = rgb_base + 1;
    std::vector<int> want(t.n_pix), want_unknown(B, 0);
    for (int b = 0; b < B; ++b)
        for (int64_t i = t.off[b]; i < t.off[b + 1]; ++i) {
            const int n = 1 + 150 * (b % 3), pick = below(3 * n + 4);
            const int id = pick == 0 ? 0 : 70000 * b + 5 + pick - 1;
            raw[i] = id;
            rgb[3 * i] = (uint8_t)(id & 255); rgb[3 * i + 1] = (uint8_t)((id >> 8) & 255); rgb[3 * i + 2] = (uint8_t)(id >> 16);
            want[i] = 0;
            if (id != 0) {
                const int k = id - (70000 * b + 5);
                if (k % 3 == 0 && k / 3 < n) want[i] = 1 + ((k / 3) * 7) % n;
                else ++want_unknown[b];
            }
        }
    int32_t *k = block_of(keys), *v = block_of(vals); int64_t* tb = block_of(tab);
    for (int is_rgb = 0; is_rgb < 2; ++is_rgb) {
        int32_t *out = block<int32_t>(t.n_pix), *unknown = block<int32_t>(B), *status = block<int32_t>(1);
        memset(out, 0x5a, t.n_pix * 4); memset(unknown, 0x5a, B * 4); status[0] = 0;
        const int rc = cvlm_debug_pan_remap_host(is_rgb ? (const void*)rgb : (const void*)raw, is_rgb, B, t.dims, t.off, t.n_pix, t.max_pixels, k,
                                                 v, tb, (int64_t)keys.size(), out, unknown, status);
        EXPECT(rc == 0 && status[0] == 0, "remap rgb=%d: rc %d status %d", is_rgb, rc, status[0]);
        for (int64_t i = 0; i < t.n_pix; ++i) if (out[i] != want[i]) { EXPECT(false, "remap rgb=%d: pixel %lld is %d, want %d", is_rgb, (long long)i, out[i], want[i]); break; }
        for (int b = 0; b < B; ++b) EXPECT(unknown[b] == want_unknown[b], "remap rgb=%d: unknown[%d] = %d, want %d", is_rgb, b, unknown[b], want_unknown[b]);
        // refused: image 2's size 0; image 3's key slice ends beyond the keys, so image 4's begins there and runs backwards
        memset(out, 0x5a, t.n_pix * 4); status[0] = 0;
        const int32_t h2 = t.dims[4]; const int64_t t4 = tb[4];
        t.dims[4] = 0; tb[4] = (int64_t)keys.size() + 1;
        const int rc2 = cvlm_debug_pan_remap_host(is_rgb ? (const void*)rgb : (const void*)raw, is_rgb, B, t.dims, t.off, t.n_pix, t.max_pixels, k,
                                                  v, tb, (int64_t)keys.size(), out, unknown, status);
        t.dims[4] = h2; tb[4] = t4;
        EXPECT(rc2 == 0 && status[0] == 1, "remap refused: rc %d status %d", rc2, status[0]);
        for (int b = 0; b < B; ++b)
            for (int64_t i = t.off[b]; i < t.off[b + 1]; ++i) {
                const bool skipped = b >= 2 && b <= 4;
                if (skipped ? out[i] != 0x5a5a5a5a : out[i] != want[i]) { EXPECT(false, "remap refused: image %d pixel %lld is %d", b, (long long)i, out[i]); break; }
            }
        free(out); free(unknown); free(status);
    }
    free(raw); free(rgb_base); free(k); free(v); free(tb);
}

// ---- the definition, plainly ------------------------------------------------------------------------------------------------------------------
struct Want {
    std::vector<int> inter, pred_area, gt_area, pred_match, gt_match;
    std::vector<double> pred_iou;
};
void definition(const int32_t* pred, const int32_t* gt, int64_t n, int G, int S, const int32_t* pc, const int32_t* gc, const uint8_t* gw, int C,
                Want& w, bool& out_of_range) {
    w.inter.assign((size_t)G * S, 0); w.pred_area.assign(S, 0); w.gt_area.assign(G, 0); w.pred_match.assign(S, 0); w.gt_match.assign(G, 0);
    w.pred_iou.assign(S, 0.0);
    for (int64_t i = 0; i < n; ++i) {
        if (gt[i] < 0 || gt[i] >= G || pred[i] < 0 || pred[i] >= S) { out_of_range = true; continue; }
        ++w.inter[(size_t)gt[i] * S + pred[i]]; ++w.pred_area[pred[i]]; ++w.gt_area[gt[i]];
    }
    auto cat = [C](int c) { return c >= 0 && c < C ? c : -1; };
    for (int g = 1; g < G; ++g)
        for (int s = 1; s < S; ++s) {
            const int in = w.inter[(size_t)g * S + s];
            if (cat(gc[g]) < 0 || cat(pc[s]) < 0 || gw[g] || cat(gc[g]) != cat(pc[s]) || in <= 0) continue;
            const double iou = (double)in / (double)(w.pred_area[s] + w.gt_area[g] - in - w.inter[s]);
            if (iou > 0.5) { w.gt_match[g] = s; w.pred_match[s] = g; w.pred_iou[s] = iou; }
        }
    std::vector<int> crowd_of(C, 0);
    for (int g = 1; g < G; ++g) {
        if (cat(gc[g]) < 0 || w.gt_match[g] != 0) continue;
        if (gw[g]) { crowd_of[cat(gc[g])] = g; w.gt_match[g] = -2; }
        else w.gt_match[g] = -1;
    }
    for (int s = 1; s < S; ++s) {
        if (cat(pc[s]) < 0 || w.pred_area[s] <= 0 || w.pred_match[s] != 0) continue;
        int v = w.inter[s];
        if (crowd_of[cat(pc[s])]) v += w.inter[(size_t)crowd_of[cat(pc[s])] * S + s];
        w.pred_match[s] = (double)v / (double)w.pred_area[s] > 0.5 ? -2 : -1;
    }
}

// B ragged images, two batches into one set of totals; `spoil` > 0 breaks a table entry of image 2 in the second batch
void quality_case(int B, int G, int S, int C, int spoil) {
    Tables t(B);
    int32_t *pred = block<int32_t>(t.n_pix), *gt = block<int32_t>(t.n_pix), *inter = block<int32_t>((size_t)B * G * S), *status = block<int32_t>(1);
    int32_t *pc = block<int32_t>((size_t)B * S), *gc = block<int32_t>((size_t)B * G);
    uint8_t* gw = block<uint8_t>((size_t)B * G);
    int32_t *pm = block<int32_t>((size_t)B * S), *pa = block<int32_t>((size_t)B * S), *gm = block<int32_t>((size_t)B * G), *ga = block<int32_t>((size_t)B * G);
    double *pi = block<double>((size_t)B * S), *iou_sum = block<double>(C);
    int64_t* counts = block<int64_t>(3 * (size_t)C);
    std::vector<long long> want_counts(3 * (size_t)C, 0); std::vector<double> want_sum(C, 0.0);
    status[0] = 0;
    memset(inter, 0x5a, (size_t)B * G * S * 4); memset(counts, 0x5a, 3 * (size_t)C * 8); memset(iou_sum, 0x5a, (size_t)C * 8);
    int want_status = 0;
    for (int batch = 0; batch < 2; ++batch) {
        fill_map(pred, t.n_pix, S);
        for (int64_t i = 0; i < t.n_pix; ++i) gt[i] = below(4) ? pred[i] % G : below(G);         // mostly the prediction relabelled: matches occur
        if (batch == 1 && t.n_pix > 40) { pred[37] = S; gt[38] = -1; }                            // two indices out of range
        for (int i = 0; i < B * S; ++i) pc[i] = i % S == 0 ? -1 : below(10) == 0 ? (below(2) ? -1 : C + 3) : (i % S) % C;
        for (int i = 0; i < B * G; ++i) { gc[i] = i % G == 0 ? -1 : below(10) == 0 ? -1 : (i % G) % C; gw[i] = i % G != 0 && below(6) == 0; }
        const int32_t h2 = B > 2 ? t.dims[4] : 0; const int64_t o3 = B > 2 ? t.off[3] : 0;
        const bool spoiled = batch == 1 && spoil && B > 2;
        if (spoiled && spoil == 1) t.dims[4] = 0;
        if (spoiled && spoil == 2) t.off[3] += 1;                                                // image 2's slice longer than its size; image 3's shorter
        int rc = cvlm_debug_pan_pair_hist_host(pred, gt, B, G, S, t.dims, t.off, t.n_pix, t.max_pixels, 1, inter, status);
        if (!rc) rc = cvlm_debug_pan_match_host(inter, B, G, S, pc, gc, gw, C, pm, pi, gm, pa, ga);
        if (!rc) rc = cvlm_debug_pan_accumulate_host(B, G, S, pc, gc, pm, pi, gm, C, batch == 0, counts, iou_sum);
        EXPECT(rc == 0, "quality B=%d G=%d S=%d: rc %d", B, G, S, rc);
        for (int b = 0; b < B; ++b) {
            Want w; bool bad = false;
            const bool skipped = spoiled && (b == 2 || (spoil == 2 && b == 3));
            definition(pred + t.off[b], gt + t.off[b], skipped ? 0 : t.off[b + 1] - t.off[b], G, S, pc + b * S, gc + b * G, gw + b * G, C, w, bad);
            if (bad) want_status |= 2;
            if (skipped) want_status |= 1;
            bool same = true;
            for (int i = 0; i < G * S; ++i) same &= inter[(size_t)b * G * S + i] == w.inter[i];
            for (int s = 0; s < S; ++s) same &= pm[b * S + s] == w.pred_match[s] && pa[b * S + s] == w.pred_area[s] && !memcmp(&pi[b * S + s], &w.pred_iou[s], 8);
            for (int g = 0; g < G; ++g) same &= gm[b * G + g] == w.gt_match[g] && ga[b * G + g] == w.gt_area[g];
            EXPECT(same, "quality B=%d G=%d S=%d batch %d: image %d differs from the definition", B, G, S, batch, b);
            for (int g = 1; g < G; ++g) {
                const int c = gc[b * G + g];
                if (c < 0 || c >= C) continue;
                if (w.gt_match[g] > 0) { ++want_counts[c]; want_sum[c] += w.pred_iou[w.gt_match[g]]; }
                else if (w.gt_match[g] == -1) ++want_counts[2 * C + c];
            }
            for (int s = 1; s < S; ++s) {
                const int c = pc[b * S + s];
                if (c >= 0 && c < C && w.pred_match[s] == -1) ++want_counts[C + c];
            }
        }
        if (B > 2) { t.dims[4] = h2; t.off[3] = o3; }
    }
    bool same = status[0] == want_status;
    for (int i = 0; i < 3 * C; ++i) same &= counts[i] == want_counts[i];
    same &= !memcmp(iou_sum, want_sum.data(), (size_t)C * 8);
    EXPECT(same, "quality B=%d G=%d S=%d C=%d: totals differ (status %d, want %d)", B, G, S, C, status[0], want_status);
    long long tp = 0; for (int c = 0; c < C; ++c) tp += counts[c];
    EXPECT(G * S < 4 || B < 3 || tp > 0, "quality B=%d G=%d S=%d: no true positive: the case checks nothing", B, G, S);
    free(pred); free(gt); free(inter); free(status); free(pc); free(gc); free(gw); free(pm); free(pa); free(gm); free(ga); free(pi); free(iou_sum); free(counts);
}

// ---- refusals -------------------------------------------------------------------------------------------------------------------------------
void refusals() {
    const int B = 2, G = 3, S = 4, C = 5;
    Tables t(B);
    const int64_t n = t.n_pix;
    int32_t *pred = block<int32_t>(n + 1), *gt = block<int32_t>(n + 1), *inter = block<int32_t>(B * G * S + 1), *status = block<int32_t>(2);
    int32_t *pc = block<int32_t>(B * S + 1), *gc = block<int32_t>(B * G + 1), *pm = block<int32_t>(B * S + 1), *pa = block<int32_t>(B * S + 1);
    int32_t *gm = block<int32_t>(B * G + 1), *ga = block<int32_t>(B * G + 1), *keys = block<int32_t>(3), *vals = block<int32_t>(3), *unknown = block<int32_t>(B + 1);
    uint8_t* gw = block<uint8_t>(B * G);
    double *pi = block<double>(B * S + 1), *sum = block<double>(C + 1);
    int64_t *counts = block<int64_t>(3 * C + 1), *tab = block<int64_t>(B + 2);
    memset(pred, 0, (n + 1) * 4); memset(gt, 0, (n + 1) * 4); memset(pc, 0xff, (B * S + 1) * 4); memset(gc, 0xff, (B * G + 1) * 4); memset(gw, 0, B * G);
    keys[0] = 1; keys[1] = 2; vals[0] = 1; vals[1] = 2; tab[0] = 0; tab[1] = 1; tab[2] = 2; status[0] = 0;
    auto off1 = [](auto* p) { return (decltype(p))((char*)p + 1); };
    auto off4 = [](auto* p) { return (decltype(p))((char*)p + 4); };
#define REFUSED(call) EXPECT((call) == CVLM_E_BADARG, "not refused: %s", #call)
#define REMAP(raw, rgb, B_, dims, off, n_, mp, k, v, tb, nk, out, unk, st) cvlm_debug_pan_remap_host(raw, rgb, B_, dims, off, n_, mp, k, v, tb, nk, out, unk, st)
    EXPECT(REMAP(pred, 0, B, t.dims, t.off, n, t.max_pixels, keys, vals, tab, 2, gt, unknown, status) == 0, "remap: the good call is refused");
    REFUSED(REMAP(nullptr, 0, B, t.dims, t.off, n, t.max_pixels, keys, vals, tab, 2, gt, unknown, status));
    REFUSED(REMAP(pred, 0, B, nullptr, t.off, n, t.max_pixels, keys, vals, tab, 2, gt, unknown, status));
    REFUSED(REMAP(pred, 0, B, t.dims, nullptr, n, t.max_pixels, keys, vals, tab, 2, gt, unknown, status));
    REFUSED(REMAP(pred, 0, B, t.dims, t.off, n, t.max_pixels, nullptr, vals, tab, 2, gt, unknown, status));
    REFUSED(REMAP(pred, 0, B, t.dims, t.off, n, t.max_pixels, keys, nullptr, tab, 2, gt, unknown, status));
    REFUSED(REMAP(pred, 0, B, t.dims, t.off, n, t.max_pixels, keys, vals, nullptr, 2, gt, unknown, status));
    REFUSED(REMAP(pred, 0, B, t.dims, t.off, n, t.max_pixels, keys, vals, tab, 2, nullptr, unknown, status));
    REFUSED(REMAP(pred, 0, B, t.dims, t.off, n, t.max_pixels, keys, vals, tab, 2, gt, nullptr, status));
    REFUSED(REMAP(pred, 0, B, t.dims, t.off, n, t.max_pixels, keys, vals, tab, 2, gt, unknown, nullptr));
    REFUSED(REMAP(off1(pred), 0, B, t.dims, t.off, n, t.max_pixels, keys, vals, tab, 2, gt, unknown, status));
    REFUSED(REMAP(pred, 0, B, t.dims, off4(t.off), n, t.max_pixels, keys, vals, tab, 2, gt, unknown, status));
    REFUSED(REMAP(pred, 0, B, t.dims, t.off, n, t.max_pixels, keys, vals, off4(tab), 2, gt, unknown, status));
    REFUSED(REMAP(pred, 0, B, t.dims, t.off, n, t.max_pixels, keys, vals, tab, 2, off1(gt), unknown, status));
    REFUSED(REMAP(pred, 2, B, t.dims, t.off, n, t.max_pixels, keys, vals, tab, 2, gt, unknown, status));
    REFUSED(REMAP(pred, 0, 0, t.dims, t.off, n, t.max_pixels, keys, vals, tab, 2, gt, unknown, status));
    REFUSED(REMAP(pred, 0, 65536, t.dims, t.off, n, t.max_pixels, keys, vals, tab, 2, gt, unknown, status));
    REFUSED(REMAP(pred, 0, B, t.dims, t.off, 0, t.max_pixels, keys, vals, tab, 2, gt, unknown, status));
    REFUSED(REMAP(pred, 0, B, t.dims, t.off, n, 0, keys, vals, tab, 2, gt, unknown, status));
    REFUSED(REMAP(pred, 0, B, t.dims, t.off, n, ((int64_t)1 << 28) + 1, keys, vals, tab, 2, gt, unknown, status));
    REFUSED(REMAP(pred, 0, B, t.dims, t.off, n, t.max_pixels, keys, vals, tab, 0, gt, unknown, status));
    REFUSED(REMAP(pred, 0, B, t.dims, t.off, n, t.max_pixels, keys, vals, tab, 2, pred, unknown, status));             // out is raw
    REFUSED(REMAP(pred, 0, B, t.dims, t.off, n, t.max_pixels, keys, vals, tab, 2, gt, unknown, unknown + 1));          // status inside unknown
#define PAIR(p, g, B_, G_, S_, dims, off, n_, mp, in, st) cvlm_debug_pan_pair_hist_host(p, g, B_, G_, S_, dims, off, n_, mp, 1, in, st)
    EXPECT(PAIR(pred, gt, B, G, S, t.dims, t.off, n, t.max_pixels, inter, status) == 0, "pair_hist: the good call is refused");
    REFUSED(PAIR(nullptr, gt, B, G, S, t.dims, t.off, n, t.max_pixels, inter, status));
    REFUSED(PAIR(pred, nullptr, B, G, S, t.dims, t.off, n, t.max_pixels, inter, status));
    REFUSED(PAIR(pred, gt, B, G, S, t.dims, t.off, n, t.max_pixels, nullptr, status));
    REFUSED(PAIR(pred, gt, B, G, S, t.dims, t.off, n, t.max_pixels, inter, nullptr));
    REFUSED(PAIR(off1(pred), gt, B, G, S, t.dims, t.off, n, t.max_pixels, inter, status));
    REFUSED(PAIR(pred, gt, B, G, S, t.dims, t.off, n, t.max_pixels, off1(inter), status));
    REFUSED(PAIR(pred, gt, B, 0, S, t.dims, t.off, n, t.max_pixels, inter, status));
    REFUSED(PAIR(pred, gt, B, G, 0, t.dims, t.off, n, t.max_pixels, inter, status));
    REFUSED(PAIR(pred, gt, B, 4097, 4096, t.dims, t.off, n, t.max_pixels, inter, status));
    REFUSED(PAIR(pred, gt, 0, G, S, t.dims, t.off, n, t.max_pixels, inter, status));
    REFUSED(PAIR(pred, gt, B, G, S, t.dims, t.off, n, t.max_pixels, pred, status));                                    // inter is pred
    REFUSED(PAIR(pred, gt, B, G, S, t.dims, t.off, n, t.max_pixels, inter, inter + B * G * S - 1));                     // status inside inter
#define MATCH(in, B_, G_, S_, pc_, gc_, gw_, C_, pm_, pi_, gm_, pa_, ga_) cvlm_debug_pan_match_host(in, B_, G_, S_, pc_, gc_, gw_, C_, pm_, pi_, gm_, pa_, ga_)
    EXPECT(MATCH(inter, B, G, S, pc, gc, gw, C, pm, pi, gm, pa, ga) == 0, "match: the good call is refused");
    REFUSED(MATCH(nullptr, B, G, S, pc, gc, gw, C, pm, pi, gm, pa, ga));
    REFUSED(MATCH(inter, B, G, S, nullptr, gc, gw, C, pm, pi, gm, pa, ga));
    REFUSED(MATCH(inter, B, G, S, pc, nullptr, gw, C, pm, pi, gm, pa, ga));
    REFUSED(MATCH(inter, B, G, S, pc, gc, nullptr, C, pm, pi, gm, pa, ga));
    REFUSED(MATCH(inter, B, G, S, pc, gc, gw, C, nullptr, pi, gm, pa, ga));
    REFUSED(MATCH(inter, B, G, S, pc, gc, gw, C, pm, nullptr, gm, pa, ga));
    REFUSED(MATCH(inter, B, G, S, pc, gc, gw, C, pm, pi, nullptr, pa, ga));
    REFUSED(MATCH(inter, B, G, S, pc, gc, gw, C, pm, pi, gm, nullptr, ga));
    REFUSED(MATCH(inter, B, G, S, pc, gc, gw, C, pm, pi, gm, pa, nullptr));
    REFUSED(MATCH(inter, B, G, S, pc, gc, gw, C, pm, off4(pi), gm, pa, ga));
    REFUSED(MATCH(inter, B, G, S, pc, gc, gw, C, off1(pm), pi, gm, pa, ga));
    REFUSED(MATCH(inter, B, G, S, pc, gc, gw, 0, pm, pi, gm, pa, ga));
    REFUSED(MATCH(inter, B, G, S, pc, gc, gw, 65537, pm, pi, gm, pa, ga));
    REFUSED(MATCH(inter, 65536, G, S, pc, gc, gw, C, pm, pi, gm, pa, ga));
    REFUSED(MATCH(inter, B, 1 << 13, 1 << 12, pc, gc, gw, C, pm, pi, gm, pa, ga));
    REFUSED(MATCH(inter, B, G, S, pc, gc, gw, C, pc, pi, gm, pa, ga));                                                 // pred_match is pred_cat
    REFUSED(MATCH(inter, B, G, S, pc, gc, gw, C, pm, pi, gm, pm, ga));                                                 // two outputs are one
#define ACC(B_, G_, S_, pc_, gc_, pm_, pi_, gm_, C_, counts_, sum_) cvlm_debug_pan_accumulate_host(B_, G_, S_, pc_, gc_, pm_, pi_, gm_, C_, 1, counts_, sum_)
    EXPECT(ACC(B, G, S, pc, gc, pm, pi, gm, C, counts, sum) == 0, "accumulate: the good call is refused");
    REFUSED(ACC(B, G, S, nullptr, gc, pm, pi, gm, C, counts, sum));
    REFUSED(ACC(B, G, S, pc, nullptr, pm, pi, gm, C, counts, sum));
    REFUSED(ACC(B, G, S, pc, gc, nullptr, pi, gm, C, counts, sum));
    REFUSED(ACC(B, G, S, pc, gc, pm, nullptr, gm, C, counts, sum));
    REFUSED(ACC(B, G, S, pc, gc, pm, pi, nullptr, C, counts, sum));
    REFUSED(ACC(B, G, S, pc, gc, pm, pi, gm, C, nullptr, sum));
    REFUSED(ACC(B, G, S, pc, gc, pm, pi, gm, C, counts, nullptr));
    REFUSED(ACC(B, G, S, pc, gc, pm, pi, gm, C, off4(counts), sum));
    REFUSED(ACC(B, G, S, pc, gc, pm, pi, gm, C, counts, off4(sum)));
    REFUSED(ACC(B, G, S, off1(pc), gc, pm, pi, gm, C, counts, sum));
    REFUSED(ACC(0, G, S, pc, gc, pm, pi, gm, C, counts, sum));
    REFUSED(ACC(B, 0, S, pc, gc, pm, pi, gm, C, counts, sum));
    REFUSED(ACC(B, G, S, pc, gc, pm, pi, gm, 0, counts, sum));
    REFUSED(ACC(B, G, S, pc, gc, pm, pi, gm, 65537, counts, sum));
    REFUSED(ACC(B, G, S, pc, gc, pm, pi, gm, C, (int64_t*)pi, sum));                                                   // counts is pred_iou
    REFUSED(ACC(B, G, S, pc, gc, pm, pi, gm, C, counts, (double*)counts + 3 * C - 1));                                 // iou_sum inside counts
    EXPECT(cvlm_debug_pan_lds_cells() == pn_lds_cells() && pn_lds_cells() > 0, "the exported LDS bound is not the header's");
    free(pred); free(gt); free(inter); free(status); free(pc); free(gc); free(pm); free(pa); free(gm); free(ga); free(keys); free(vals);
    free(unknown); free(gw); free(pi); free(sum); free(counts); free(tab);
}

}  // namespace

int main() {
    remap_cases();
    quality_case(1, 1, 1, 1, 0);
    quality_case(1, 2, 2, 3, 0);
    quality_case(7, 21, 62, 61, 0);
    quality_case(7, 9, 11, 133, 1);
    quality_case(7, 9, 11, 4, 2);
    quality_case(9, 40, 45, 7, 0);
    refusals();
    printf(failures ? "pq_host_sanitize: %d FAILED\n" : "pq_host_sanitize: all cases passed\n", failures);
    return failures ? 1 : 0;
}
