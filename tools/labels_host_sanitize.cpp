// Stand-alone check of the cvlm_debug_label_*_host entries for a host sanitizer: their per-thread functions are the
// kernels' (csrc/labels_logic.h, csrc/sized_logic.h), so their indexing is what runs on the device.  Every buffer is a heap block of
// exactly the size the interface states, so that AddressSanitizer sees any access beyond it.  Ragged images -- (1, 1), one row, widths
// around the unit of 64 pixels -- at K = 1, 3 and 65, the planes in one accumulate call and cut into calls of 4, weights NULL, dyadic
// and NaN, +-inf and NaN planes; the maps are held against a plain restatement of the definition (argmax in increasing k, the three
// areas, the published per-query test), the cut calls against the single call byte for byte.  Refused tables -- a size of 0, a slice
// longer than its size, an image beyond the maps -- run through the same exact-size buffers and must leave the fill.  The histogram
// with uint8 and int32 ground truth, both flags, values outside the classes, against plain counting.
// Build and run on the CPU, from the repository root:
//   hipcc -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/labels_host_sanitize.cpp camouflaged-vlm_amd/csrc/labels.hip -o /tmp/labels_host_sanitize && /tmp/labels_host_sanitize
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>                                         // the shared headers' device halves, when hipcc compiles this file
#endif

#include "../include/cvlm.h"
#include "../camouflaged-vlm_amd/csrc/labels_logic.h"

namespace {

uint32_t rng_state = 2323u;
uint32_t rng() { return rng_state = rng_state * 1664525u + 1013904223u; }
int below(int n) { return (int)((rng() >> 8) % (uint32_t)n); }

template <class T> T* block(size_t n) { return (T*)malloc((n ? n : 1) * sizeof(T)); }     // exactly n elements (1 where n is 0)

int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

struct Maps {
    int B, K;
    int64_t n_pix, P;
    float* score; int16_t *winner, *segment; int32_t *areas, *ids, *nseg, *status;
    Maps(int B_, int K_, int64_t n) : B(B_), K(K_), n_pix(n), P((int64_t)B_ * K_) {
        score = block<float>(n); winner = block<int16_t>(n); segment = block<int16_t>(n);
        areas = block<int32_t>(3 * P); ids = block<int32_t>(P); nseg = block<int32_t>(B); status = block<int32_t>(1);
        memset(score, 0x5a, n * 4); memset(winner, 0x5a, n * 2); memset(segment, 0x5a, n * 2);
        memset(areas, 0x5a, 3 * P * 4); memset(ids, 0x5a, P * 4); memset(nseg, 0x5a, B * 4); status[0] = -3;
    }
    ~Maps() { free(score); free(winner); free(segment); free(areas); free(ids); free(nseg); free(status); }
    bool same(const Maps& o) const {
        return !memcmp(score, o.score, n_pix * 4) && !memcmp(winner, o.winner, n_pix * 2) && !memcmp(segment, o.segment, n_pix * 2) &&
               !memcmp(areas, o.areas, 3 * P * 4) && !memcmp(ids, o.ids, P * 4) && !memcmp(nseg, o.nseg, B * 4) && status[0] == o.status[0];
    }
};

// the whole sequence; step > 0: accumulate calls of `step` planes
int run(Maps& m, const float* logits, int Hs, int Ws, const int32_t* dims, const int64_t* off, const float* wts, int level, double thr,
        int64_t max_pixels, int step) {
    int rc = cvlm_debug_label_init_host(m.score, m.winner, m.segment, m.n_pix, m.areas, m.ids, m.B, m.K, m.nseg, m.status);
    const int P = (int)m.P;
    for (int p0 = 0; !rc && p0 < P; p0 += step > 0 ? step : P) {
        const int p1 = step > 0 && p0 + step < P ? p0 + step : P;
        rc = cvlm_debug_label_accumulate_host(logits + (int64_t)p0 * Hs * Ws, p0, p1, Hs, Ws, m.B, m.K, dims, off, wts, level, m.score, m.winner,
                                              m.segment, m.n_pix, max_pixels, m.areas, m.status);
    }
    if (!rc) rc = cvlm_debug_label_finish_host(m.B, m.K, dims, off, &thr, m.winner, m.segment, m.n_pix, max_pixels, m.areas, m.ids, m.nseg, m.status);
    return rc;
}

// the definition, plainly, for one image; the value and the bit come from the shared per-pixel functions
void definition(const float* logits, int Hs, int Ws, int K, int h, int w, const float* wts, int level, double thr, std::vector<int>& winner,
                std::vector<int>& segment, std::vector<int>& orig, std::vector<int>& won, std::vector<int>& kept_area, std::vector<int>& ids) {
    winner.assign((size_t)h * w, -1); segment.assign((size_t)h * w, -1);
    orig.assign(K, 0); won.assign(K, 0); kept_area.assign(K, 0); ids.assign(K, 0);
    std::vector<char> own((size_t)h * w, 0);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const sz_axis ax = sz_axis_of(x, Ws, (double)Ws / w, true), ay = sz_axis_of(y, Hs, (double)Hs / h, false);
            float best = 0.0f;
            int arg = -1;
            bool arg_bit = false;
            for (int k = 0; k < K; ++k) {
                const float v = lb_value(logits + (int64_t)k * Hs * Ws, Ws, ax, ay);
                const bool bit = v * 255.0f >= (float)level;
                orig[k] += bit;
                const float wk = wts ? wts[k] : 1.0f;
                if (std::isnan(wk) || std::isnan(v)) continue;
                const float s = wk * v;
                if (arg < 0 || s > best) { best = s; arg = k; arg_bit = bit; }
            }
            winner[(size_t)y * w + x] = arg;
            own[(size_t)y * w + x] = arg_bit;
            if (arg >= 0) { ++won[arg]; kept_area[arg] += arg_bit; }
        }
    int current = 0;
    for (int k = 0; k < K; ++k) {
        if (!(won[k] > 0 && orig[k] > 0 && kept_area[k] > 0)) continue;
        if ((double)won[k] / (double)orig[k] < thr) continue;
        ids[k] = ++current;
    }
    for (size_t i = 0; i < winner.size(); ++i)
        if (winner[i] >= 0 && own[i] && ids[winner[i]] > 0) segment[i] = winner[i];
}

void maps_case(int K, int weights_kind, int level, double thr) {
    const int sizes[][2] = {{1, 1}, {7, 33}, {1, 64}, {3, 65}, {5, 63}, {9, 131}, {2, 32}};
    const int B = 7, Hs = 12, Ws = 20, P = B * K;
    int32_t* dims = block<int32_t>(2 * B);
    int64_t* off = block<int64_t>(B + 1);
    int64_t max_pixels = 0;
    off[0] = 0;
    for (int b = 0; b < B; ++b) {
        dims[2 * b] = sizes[b][0]; dims[2 * b + 1] = sizes[b][1];
        off[b + 1] = off[b] + (int64_t)sizes[b][0] * sizes[b][1];
        if ((int64_t)sizes[b][0] * sizes[b][1] > max_pixels) max_pixels = (int64_t)sizes[b][0] * sizes[b][1];
    }
    float* logits = block<float>((size_t)P * Hs * Ws);
    for (int p = 0; p < P; ++p) {
        const int kind = below(12);
        for (int i = 0; i < Hs * Ws; ++i) {
            float v = below(3) ? (float)(below(1200) - 600) / 50.0f : (below(2) ? 30.0f : -30.0f);
            if (kind == 0) v = NAN;
            if (kind == 1) v = below(2) ? INFINITY : -INFINITY;
            logits[(size_t)p * Hs * Ws + i] = v;
        }
    }
    float* wts = nullptr;
    if (weights_kind) {
        wts = block<float>(P);
        const float dyadic[] = {1.0f, 0.5f, 2.0f, 0.25f, 1.5f, 0.0f, -1.0f};
        for (int p = 0; p < P; ++p) wts[p] = weights_kind == 2 && below(4) == 0 ? NAN : dyadic[below(7)];
    }
    Maps whole(B, K, off[B]), cut(B, K, off[B]);
    EXPECT(run(whole, logits, Hs, Ws, dims, off, wts, level, thr, max_pixels, 0) == 0, "K %d: the call was refused", K);
    EXPECT(run(cut, logits, Hs, Ws, dims, off, wts, level, thr, max_pixels, 4) == 0, "K %d: a cut call was refused", K);
    EXPECT(whole.status[0] == 0 && whole.same(cut), "K %d weights %d: calls of 4 planes differ from one call", K, weights_kind);
    std::vector<int> winner, segment, orig, won, kept_area, ids;
    for (int b = 0; b < B; ++b) {
        const int h = sizes[b][0], w = sizes[b][1];
        definition(logits + (int64_t)b * K * Hs * Ws, Hs, Ws, K, h, w, wts ? wts + b * K : nullptr, level, thr, winner, segment, orig, won, kept_area, ids);
        bool ok = true;
        for (int i = 0; i < h * w; ++i) ok = ok && whole.winner[off[b] + i] == winner[i] && whole.segment[off[b] + i] == segment[i];
        int n = 0;
        for (int k = 0; k < K; ++k) {
            const int64_t p = (int64_t)b * K + k;
            ok = ok && whole.areas[p] == orig[k] && whole.areas[P + p] == won[k] && whole.areas[2 * P + p] == kept_area[k] && whole.ids[p] == ids[k];
            n += ids[k] > 0;
        }
        EXPECT(ok && whole.nseg[b] == n, "K %d weights %d level %d: image %d differs from the definition", K, weights_kind, level, b);
    }
    // the lookup into an exact-size map
    int32_t* table = block<int32_t>(P);
    int32_t* out = block<int32_t>(off[B]);
    for (int p = 0; p < P; ++p) table[p] = 1000 + p;
    EXPECT(cvlm_debug_label_lookup_host(whole.segment, B, K, dims, off, off[B], max_pixels, table, -7, out, whole.status) == 0, "lookup refused");
    bool ok = whole.status[0] == 0;
    for (int b = 0; b < B; ++b)
        for (int64_t i = off[b]; i < off[b + 1]; ++i) ok = ok && out[i] == (whole.segment[i] < 0 ? -7 : 1000 + b * K + whole.segment[i]);
    EXPECT(ok, "K %d: the lookup differs", K);
    // refused tables: image 2 of size 0, image 3's slice one longer, the last image beyond the maps -- each leaves its image at the fill
    for (int kind = 0; kind < 3; ++kind) {
        int32_t* d2 = block<int32_t>(2 * B);
        int64_t* o2 = block<int64_t>(B + 1);
        memcpy(d2, dims, 2 * B * 4); memcpy(o2, off, (B + 1) * 8);
        int64_t n = off[B];
        int bad = 2;
        if (kind == 0) d2[4] = 0;
        if (kind == 1) { bad = 3; for (int b = 4; b <= B; ++b) o2[b] += 1; n += 1; }
        if (kind == 2) { bad = B - 1; n -= 1; }
        Maps r(B, K, n);
        EXPECT(run(r, logits, Hs, Ws, d2, o2, wts, level, thr, max_pixels, 4) == 0, "refusal case %d: BADARG", kind);
        bool fill = r.status[0] == 1 && r.nseg[bad] == 0;
        for (int64_t i = o2[bad]; i < o2[bad + 1] && i < n; ++i) fill = fill && r.winner[i] == -1 && r.segment[i] == -1 && r.score[i] == 0.0f;
        for (int k = 0; k < K; ++k) fill = fill && r.areas[bad * K + k] == 0 && r.areas[P + bad * K + k] == 0 && r.ids[bad * K + k] == 0;
        const int other = bad == 0 ? 1 : 0;
        fill = fill && !memcmp(r.winner + o2[other], whole.winner + off[other], (size_t)(off[other + 1] - off[other]) * 2);
        EXPECT(fill, "K %d refusal case %d: image %d is not at the fill or its neighbour is not whole", K, kind, bad);
        free(d2); free(o2);
    }
    free(table); free(out); free(wts); free(logits); free(dims); free(off);
}

template <class G>
void hist_case(int C, int64_t n, int ignore, int reduce) {
    int32_t* pred = block<int32_t>(n);
    G* gt = block<G>(n);
    for (int64_t i = 0; i < n; ++i) {
        gt[i] = (G)(below(8) == 0 ? 255 : below(C + 2));
        pred[i] = below(3) ? (int32_t)gt[i] : below(C + 3) - 1;
    }
    int64_t* totals = block<int64_t>(3 * (size_t)C);
    std::vector<int64_t> want(3 * (size_t)C, 0);
    for (int round = 0; round < 2; ++round) {                        // the second call accumulates
        EXPECT(cvlm_debug_label_iou_hist_host(pred, gt, sizeof(G) == 1, n, C, ignore, reduce, round == 0, totals) == 0, "histogram refused");
        for (int64_t i = 0; i < n; ++i) {
            int g = (int)gt[i];
            if (reduce) { if (g == 0) g = 255; g -= 1; if (g == 254) g = 255; }
            if (g == ignore) continue;
            const int p = pred[i];
            if (p >= 0 && p < C) { ++want[C + p]; if (p == g) ++want[p]; }
            if (g >= 0 && g < C) ++want[2 * C + g];
        }
        EXPECT(!memcmp(totals, want.data(), 3 * (size_t)C * 8), "C %d n %lld: the histogram differs in round %d", C, (long long)n, round);
    }
    free(pred); free(gt); free(totals);
}

}  // namespace

int main() {
    for (int K : {1, 3, 65})
        for (int weights_kind = 0; weights_kind < 3; ++weights_kind) {
            maps_case(K, weights_kind, 128, 0.8);
            maps_case(K, weights_kind, 1, 0.5);
        }
    maps_case(5, 1, 255, 1.0);
    for (int C : {1, 3, 150, 4097})
        for (int64_t n : {(int64_t)1, (int64_t)63, (int64_t)1000}) {
            hist_case<uint8_t>(C, n, 255, 0);
            hist_case<uint8_t>(C, n, 255, 1);
            hist_case<int32_t>(C, n, 0, 0);
            hist_case<int32_t>(C, n, 255, 1);
        }
    printf(failures ? "%d check(s) FAILED\n" : "label host entries: every check passed (%d failures)\n", failures);
    return failures ? 1 : 0;
}
