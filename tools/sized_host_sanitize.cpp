// Stand-alone check of cvlm_debug_mask_pack_sized_host and cvlm_debug_mask_rle_host_w for a host sanitizer: the
// entries' per-thread functions are the kernels' (csrc/sized_logic.h, csrc/rle_logic.h), so their indexing is what runs on the
// device.  Every buffer is a heap block of exactly the size the interface states, so that AddressSanitizer sees any access beyond it;
// the bits are held against a plain pixel loop over the same taps, the counts against a plain pixel loop over the unpadded plane.
// Build and run on the CPU, from the repository root:
//   hipcc -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/sized_host_sanitize.cpp camouflaged-vlm_amd/csrc/sized.hip camouflaged-vlm_amd/csrc/rle.hip \
//         -o /tmp/sized_host_sanitize && /tmp/sized_host_sanitize
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/cvlm.h"

namespace {

uint32_t rng_state = 12345u;
uint32_t rng() { return rng_state = rng_state * 1664525u + 1013904223u; }

// cv::resize(INTER_LINEAR)'s taps of one output coordinate, as oracle/metrics_oracle.py states them
void taps(int d, int n_src, int n_dst, bool column, int& i0, int& i1, float& w1) {
    float f = (float)(((double)d + 0.5) * ((double)n_src / (double)n_dst) - 0.5);
    const int i = (int)std::floor(f);
    f -= (float)i;
    if (column) {
        i0 = i;
        if (i < 0) { i0 = 0; f = 0.f; }
        if (i0 >= n_src - 1) { i0 = n_src - 1; f = 0.f; }
        i1 = i0 + 1 < n_src ? i0 + 1 : n_src - 1;
    } else {
        i0 = i < 0 ? 0 : (i > n_src - 1 ? n_src - 1 : i);
        i1 = i + 1 < 0 ? 0 : (i + 1 > n_src - 1 ? n_src - 1 : i + 1);
    }
    w1 = f;
}

bool loop_pixel(const float* src, int Hs, int Ws, int h, int w, int y, int x, int level) {
    int x0, x1, y0, y1;
    float fx, fy;
    taps(x, Ws, w, true, x0, x1, fx);
    taps(y, Hs, h, false, y0, y1, fy);
    auto sig = [](float v) { return 1.0f / (1.0f + expf(-v)); };
    volatile float a = sig(src[y0 * Ws + x0]) * (1.f - fx), b = sig(src[y0 * Ws + x1]) * fx;          // volatile: no contraction
    volatile float c = sig(src[y1 * Ws + x0]) * (1.f - fx), d = sig(src[y1 * Ws + x1]) * fx;
    volatile float t0 = a + b, t1 = c + d;
    volatile float u0 = t0 * (1.f - fy), u1 = t1 * fy;
    volatile float v = u0 + u1;
    return v * 255.0f >= (float)level;
}

// one call over P planes of the given sizes; bad_plane >= 0: that plane's slice is four bytes short and must be refused
int check_pack(int Hs, int Ws, const std::vector<std::pair<int, int>>& sizes, int level, int bad_plane, bool with_stats) {
    const int P = (int)sizes.size();
    float* logits = (float*)malloc(sizeof(float) * (size_t)P * Hs * Ws);
    for (int64_t i = 0; i < (int64_t)P * Hs * Ws; ++i) logits[i] = ((int)(rng() >> 8) % 2001 - 1000) / 250.0f;
    int32_t* dims = (int32_t*)malloc(sizeof(int32_t) * 2 * P);
    int64_t* offsets = (int64_t*)malloc(sizeof(int64_t) * (P + 1));
    offsets[0] = 0;
    int64_t max_words = 1;
    for (int p = 0; p < P; ++p) {
        dims[2 * p] = sizes[p].first;
        dims[2 * p + 1] = sizes[p].second;
        const int64_t words = (int64_t)sizes[p].first * ((sizes[p].second + 31) / 32);
        max_words = words > max_words ? words : max_words;
        offsets[p + 1] = offsets[p] + 4 * words - (p == bad_plane ? 4 : 0);
    }
    const int64_t nbytes = offsets[P];
    uint8_t* bits = (uint8_t*)malloc((size_t)nbytes);
    for (int64_t i = 0; i < nbytes; ++i) bits[i] = 0xA5;
    int32_t* area = with_stats ? (int32_t*)malloc(sizeof(int32_t) * P) : nullptr;
    int32_t* box = with_stats ? (int32_t*)malloc(sizeof(int32_t) * 4 * P) : nullptr;
    int32_t* status = (int32_t*)malloc(sizeof(int32_t));
    int bad = cvlm_debug_mask_pack_sized_host(logits, P, Hs, Ws, dims, offsets, level, bits, nbytes, max_words, area, box, status) != 0;
    bad |= status[0] != (bad_plane >= 0 ? 1 : 0);
    int64_t set = 0;
    for (int p = 0; p < P; ++p) {
        const int h = sizes[p].first, w = sizes[p].second, ws = (w + 31) / 32;
        const uint8_t* plane = bits + offsets[p];
        if (p == bad_plane) {
            for (int64_t i = offsets[p]; i < offsets[p + 1]; ++i) bad |= bits[i] != 0xA5;
            if (with_stats) bad |= area[p] != 0 || box[4 * p] != -1;
            continue;
        }
        int n = 0, x0 = w, y0 = h, x1 = -1, y1 = -1;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < 32 * ws; ++x) {
                const bool got = (plane[(int64_t)y * 4 * ws + (x >> 3)] >> (7 - (x & 7))) & 1;
                const bool want = x < w && loop_pixel(logits + (int64_t)p * Hs * Ws, Hs, Ws, h, w, y, x, level);
                bad |= got != want;
                if (got) { ++n; x0 = x < x0 ? x : x0; y0 = y < y0 ? y : y0; x1 = x > x1 ? x : x1; y1 = y > y1 ? y : y1; }
            }
        set += n;
        if (with_stats) {
            bad |= area[p] != n;
            if (n) bad |= box[4 * p] != x0 || box[4 * p + 1] != y0 || box[4 * p + 2] != x1 || box[4 * p + 3] != y1;
            else bad |= box[4 * p] != -1 || box[4 * p + 3] != -1;
        }
    }
    printf("%s  pack: %d planes of %d x %d, level %d, refused plane %d, %s: %lld bytes, %lld set\n", bad ? "FAIL" : "ok  ", P, Hs, Ws, level,
           bad_plane, with_stats ? "area and box" : "bits only", (long long)nbytes, (long long)set);
    free(status); free(box); free(area); free(bits); free(offsets); free(dims); free(logits);
    return bad;
}

int check_rle(int P, int H, int Wt, int density_percent, int shorten_last) {
    const int W = 32 * ((Wt + 31) / 32);
    const int64_t plane_bytes = (int64_t)H * W / 8;
    uint8_t* bits = (uint8_t*)malloc((size_t)(P * plane_bytes));
    for (int64_t i = 0; i < P * plane_bytes; ++i) {                   // the pad bits too: they must not matter
        uint8_t b = 0;
        for (int k = 0; k < 8; ++k) b = (uint8_t)(b << 1 | ((int)(rng() >> 8) % 100 < density_percent));
        bits[i] = b;
    }
    auto loop_counts = [&](const uint8_t* plane) {
        std::vector<int32_t> c;
        int value = 0, run = 0;
        for (int x = 0; x < Wt; ++x)
            for (int y = 0; y < H; ++y) {
                const int64_t i = (int64_t)y * W + x;
                const int v = (plane[i >> 3] >> (7 - (i & 7))) & 1;
                if (v != value) { c.push_back(run); value = v; run = 0; }
                ++run;
            }
        c.push_back(run);
        return c;
    };
    int32_t* n_runs = (int32_t*)malloc(sizeof(int32_t) * P);
    int bad = cvlm_debug_mask_rle_host_w((const uint32_t*)bits, P, H, W, Wt, n_runs, nullptr, nullptr, 0, nullptr) != 0;
    int64_t* offsets = (int64_t*)malloc(sizeof(int64_t) * (P + 1));
    offsets[0] = 0;
    for (int p = 0; p < P; ++p) offsets[p + 1] = offsets[p] + n_runs[p] - (p == P - 1 ? shorten_last : 0);
    const int64_t total = offsets[P];
    int32_t* counts = (int32_t*)malloc(sizeof(int32_t) * (size_t)total);
    int32_t* status = (int32_t*)malloc(sizeof(int32_t));
    bad |= cvlm_debug_mask_rle_host_w((const uint32_t*)bits, P, H, W, Wt, n_runs, offsets, counts, total, status) != 0;
    bad |= status[0] != (shorten_last ? 1 : 0);
    for (int p = 0; p < P; ++p) {
        const std::vector<int32_t> want = loop_counts(bits + p * plane_bytes);
        bad |= (int)want.size() != n_runs[p];
        for (int64_t k = 0; k < offsets[p + 1] - offsets[p] && k < (int64_t)want.size(); ++k) bad |= counts[offsets[p] + k] != want[(size_t)k];
    }
    printf("%s  rle:  P = %d, %d x %d in rows of %d, density %d %%, last slice %d short: %lld counts\n", bad ? "FAIL" : "ok  ", P, H, Wt, W,
           density_percent, shorten_last, (long long)total);
    free(status); free(counts); free(offsets); free(n_runs); free(bits);
    return bad;
}

}  // namespace

int main() {
    int bad = 0;
    const std::vector<std::pair<int, int>> ragged = {{1, 1}, {70, 33}, {5, 65}, {33, 31}, {1, 32}, {97, 131}, {2, 64}};
    for (int level : {1, 128, 254, 255}) bad |= check_pack(24, 40, ragged, level, -1, true);
    bad |= check_pack(24, 40, ragged, 128, -1, false);
    bad |= check_pack(24, 40, ragged, 128, 2, true);                  // a slice that is not its size's length: refused, untouched
    bad |= check_pack(24, 40, ragged, 128, 6, false);
    bad |= check_pack(1, 40, {{33, 97}, {1, 1}}, 128, -1, true);
    bad |= check_pack(24, 1, {{33, 33}, {2, 2}}, 128, -1, true);
    bad |= check_pack(64, 96, {{64, 96}, {213, 320}}, 128, -1, true); // the identity size and an enlargement
    const int shapes[][2] = {{1, 1}, {1, 31}, {8, 33}, {33, 31}, {32, 63}, {33, 65}, {65, 97}, {130, 517}, {32, 64}};
    for (const auto& s : shapes)
        for (int density : {0, 1, 50, 99, 100}) bad |= check_rle(3, s[0], s[1], density, 0);
    bad |= check_rle(3, 33, 65, 50, 1);                               // an undersized slot: the dropped stores must not happen
    bad |= check_rle(2, 65, 97, 50, 40);
    printf(bad ? "FAILED\n" : "all equal to the pixel loops\n");
    return bad;
}
