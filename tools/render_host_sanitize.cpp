// Stand-alone check of cvlm_debug_render_host for a host sanitizer: the entry's per-pixel functions are the kernel's
// (csrc/render_logic.h), so their indexing is what runs on the device.  Every buffer is a heap block of exactly the size the interface
// states, so that AddressSanitizer sees any access beyond it: ragged image sizes whose last bytes end the image buffer, sized planes with
// every pad bit dirty, a levels map that ends its buffer, label maps whose border pixels' neighbours would lie outside it.  The bytes are
// held against a per-pixel loop written out plainly; then every refusal -- a size that is none, offsets off their boundary, backwards or
// beyond the buffer, layer ranges, kinds, flags, sources, slices and table rows -- at the first, a middle and the last position, and in
// place, through the same exact-size buffers.
// Build and run on the CPU, from the repository root:
//   hipcc -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/render_host_sanitize.cpp camouflaged-vlm_amd/csrc/render.hip -o /tmp/render_host_sanitize && /tmp/render_host_sanitize
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/cvlm.h"

#pragma clang fp contract(off)

namespace {

uint32_t rng_state = 3131u;
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

uint8_t blend(uint8_t c, uint8_t col, float a) {
    const float b = 1.0f - a;
    const float p = (float)c * b;
    const float q = (float)col * a;
    const float v = nearbyintf(p + q);
    return (uint8_t)(v < 0.0f ? 0.0f : v > 255.0f ? 255.0f : v);
}

struct Scene {
    std::vector<int32_t> dims, layer_off, labels;
    std::vector<int64_t> img_off, layers;
    std::vector<uint8_t> img, bits, levels, rgb;
    std::vector<float> alpha;
    int B = 0, L = 0, T = 0;
    int64_t max_pixels = 1;
};

int add_rows(Scene& s, int n, float a_fixed) {
    const int first = s.T;
    for (int k = 0; k < n; ++k) {
        for (int ch = 0; ch < 3; ++ch) s.rgb.push_back((uint8_t)below(256));
        const int r = below(6);
        s.alpha.push_back(a_fixed >= 0.0f ? a_fixed : r == 0 ? 0.0f : r == 1 ? 1.0f : below(1000) / 1000.0f);
    }
    s.T += n;
    return first;
}

Scene make_scene() {
    Scene s;
    const int sizes[][2] = {{1, 1}, {2, 3}, {7, 5}, {3, 31}, {2, 32}, {5, 33}, {4, 37}, {3, 65}, {9, 130}, {1, 97}};
    s.B = (int)(sizeof(sizes) / sizeof(sizes[0]));
    s.img_off.push_back(0);
    s.layer_off.push_back(0);
    add_rows(s, 1, 0.25f);                                            // a row that belongs to no layer
    for (int b = 0; b < s.B; ++b) {
        const int h = sizes[b][0], w = sizes[b][1], ws = (w + 31) / 32;
        s.dims.push_back(h); s.dims.push_back(w);
        if ((int64_t)h * w > s.max_pixels) s.max_pixels = (int64_t)h * w;
        for (int i = 0; i < 3 * h * w; ++i) s.img.push_back((uint8_t)below(256));
        while (s.img.size() % 4) s.img.push_back(0xEE);
        s.img_off.push_back((int64_t)s.img.size());
        const int n_layers = b == 1 ? 0 : 1 + below(5);
        for (int l = 0; l < n_layers; ++l) {
            const int kind = (b + l) % 3;
            if (kind == 0) {
                const int64_t src = (int64_t)s.bits.size();
                for (int y = 0; y < h; ++y)
                    for (int c = 0; c < ws; ++c) {
                        uint32_t word = 0;                            // bit i = pixel 32 c + i; every pad bit 1
                        for (int i = 0; i < 32; ++i) word |= (uint32_t)(32 * c + i >= w || below(2)) << i;
                        for (int k = 0; k < 4; ++k) {                 // numpy.packbits' order: pixel i -> bit 7 - (i & 7) of byte i >> 3
                            uint8_t byte = 0;
                            for (int i = 0; i < 8; ++i) byte |= (uint8_t)(((word >> (8 * k + i)) & 1u) << (7 - i));
                            s.bits.push_back(byte);
                        }
                    }
                const int64_t row[] = {0 | (int64_t)(below(2) ? 2 : 0) << 8, src, add_rows(s, 1, -1.0f), 1};
                s.layers.insert(s.layers.end(), row, row + 4);
            } else if (kind == 1) {
                const int64_t src = (int64_t)s.levels.size();
                for (int i = 0; i < h * w; ++i) s.levels.push_back((uint8_t)below(256));
                const int64_t row[] = {1, src, add_rows(s, 256, -1.0f), 256};
                s.layers.insert(s.layers.end(), row, row + 4);
            } else {
                const int64_t src = (int64_t)s.labels.size();
                const int n = 1 + below(5);
                for (int i = 0; i < h * w; ++i) {
                    const int r = below(12);
                    s.labels.push_back(r == 0 ? -1 : r == 1 ? n : r == 2 ? std::numeric_limits<int32_t>::max() : below(n));
                }
                const int64_t row[] = {2 | (int64_t)below(2) << 8, src, add_rows(s, n, -1.0f), n};
                s.layers.insert(s.layers.end(), row, row + 4);
            }
        }
        s.L += n_layers;
        s.layer_off.push_back(s.L);
    }
    return s;
}

// the contract read plainly: expected[] holds what the call must leave in out (0xA5 where it writes nothing)
void reference(const Scene& s, const std::vector<bool>& image_refused, const std::vector<bool>& layer_skipped, std::vector<uint8_t>& out,
               int& status) {
    status = 0;
    for (int b = 0; b < s.B; ++b) {
        if (image_refused[(size_t)b]) { status |= 1; continue; }
        const int h = s.dims[2 * (size_t)b], w = s.dims[2 * (size_t)b + 1], ws = (w + 31) / 32;
        uint8_t* px = out.data() + s.img_off[(size_t)b];
        memcpy(px, s.img.data() + s.img_off[(size_t)b], (size_t)3 * h * w);
        for (int l = s.layer_off[(size_t)b]; l < s.layer_off[(size_t)b + 1]; ++l) {
            if (layer_skipped[(size_t)l]) { status |= 2; continue; }
            const int64_t* row = &s.layers[4 * (size_t)l];
            const int kind = (int)(row[0] & 0xff), flags = (int)(row[0] >> 8);
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    int64_t t = -1;
                    const int64_t p = (int64_t)y * w + x;
                    if (kind == 0) {
                        const uint8_t byte = s.bits[(size_t)(row[1] + 4 * ((int64_t)y * ws) + x / 8)];
                        const bool on = ((byte >> (7 - (x & 7))) & 1) != 0;
                        if (on != ((flags & 2) != 0)) t = row[2];
                    } else if (kind == 1) {
                        t = row[2] + s.levels[(size_t)(row[1] + p)];
                    } else {
                        const int32_t* m = &s.labels[(size_t)row[1]];
                        const int32_t id = m[p];
                        bool edge = (x > 0 && m[p - 1] != id) || (x < w - 1 && m[p + 1] != id) || (y > 0 && m[p - w] != id) ||
                                    (y < h - 1 && m[p + w] != id);
                        if (id >= 0 && id < row[3] && (!(flags & 1) || edge)) t = row[2] + id;
                    }
                    if (t < 0) continue;
                    const float a = s.alpha[(size_t)t];
                    if (!(a >= 0.0f && a <= 1.0f)) { status |= 4; continue; }
                    for (int ch = 0; ch < 3; ++ch) px[3 * p + ch] = blend(px[3 * p + ch], s.rgb[3 * (size_t)t + ch], a);
                }
        }
    }
}

int calls = 0;

// one call through exact-size heap blocks -> the bytes of out and the status
int run(const Scene& s, bool in_place, std::vector<uint8_t>& got, int& status, bool null_sources = false) {
    uint8_t* img = exact(s.img);
    int64_t* img_off = exact(s.img_off);
    int32_t* dims = exact(s.dims);
    int32_t* layer_off = exact(s.layer_off);
    int64_t* layers = exact(s.layers);
    uint8_t* bits = null_sources ? nullptr : exact(s.bits);
    uint8_t* levels = null_sources ? nullptr : exact(s.levels);
    int32_t* labels = null_sources ? nullptr : exact(s.labels);
    uint8_t* rgb = exact(s.rgb);
    float* alpha = exact(s.alpha);
    uint8_t* out = in_place ? img : (uint8_t*)malloc(s.img.size());
    if (!in_place) memset(out, 0xA5, s.img.size());
    int32_t* st = (int32_t*)malloc(4);
    st[0] = -1;
    const int rc = cvlm_debug_render_host(img, (int64_t)s.img.size(), img_off, dims, s.B, s.max_pixels, layer_off, layers, s.L, bits,
                                          (int64_t)s.bits.size(), levels, (int64_t)s.levels.size(), labels, (int64_t)s.labels.size(), rgb,
                                          alpha, s.T, out, st);
    ++calls;
    got.assign(out, out + s.img.size());
    status = st[0];
    if (!in_place) free(out);
    free(img); free(img_off); free(dims); free(layer_off); free(layers); free(bits); free(levels); free(labels); free(rgb); free(alpha); free(st);
    return rc;
}

void check(const Scene& s, const std::vector<bool>& image_refused, const std::vector<bool>& layer_skipped, int line, bool null_sources = false) {
    for (int in_place = 0; in_place < 2; ++in_place) {
        std::vector<uint8_t> want = in_place ? s.img : std::vector<uint8_t>(s.img.size(), 0xA5), got;
        int want_status = 0, status = 0;
        reference(s, image_refused, layer_skipped, want, want_status);
        const int rc = run(s, in_place != 0, got, status, null_sources);
        if (rc != 0 || status != want_status || got != want) {
            ++failures;
            printf("FAILED case of line %d (in place %d): rc %d, status %d for %d, bytes %s\n", line, in_place, rc, status, want_status,
                   got == want ? "equal" : "differ");
        }
    }
}

}  // namespace

int main() {
    const Scene s = make_scene();
    const std::vector<bool> no_image((size_t)s.B, false), no_layer((size_t)s.L, false);
    check(s, no_image, no_layer, __LINE__);
    {                                                                 // no sources at all: every layer is skipped
        check(s, no_image, std::vector<bool>((size_t)s.L, true), __LINE__, true);
    }
    {                                                                 // L = 0: a copy
        Scene t = s;
        t.L = 0; t.layers.clear();
        t.layer_off.assign((size_t)s.B + 1, 0);
        check(t, no_image, std::vector<bool>(), __LINE__);
    }
    const int last_b = s.B - 1, mid_b = s.B / 2;
    for (int b : {0, mid_b, last_b}) {                                // images refused whole
        std::vector<bool> refused = no_image;
        refused[(size_t)b] = true;
        for (int what = 0; what < 6; ++what) {
            Scene t = s;
            std::vector<bool> r = refused;
            if (what == 0) t.dims[2 * (size_t)b] = 0;
            if (what == 1) t.dims[2 * (size_t)b + 1] = 16385;
            if (what == 2) t.dims[2 * (size_t)b] = -3;
            if (what == 3) {                                          // the slice's start off a multiple of 4: the image before it ends there
                if (b == 0) continue;
                t.img_off[(size_t)b] += 2;
                r[(size_t)b - 1] = true;
            }
            if (what == 4) {                                          // the slice's end beyond the buffer (the last) or its pad (the others)
                t.img_off[(size_t)b + 1] += 4;
                if (b < last_b) r[(size_t)b + 1] = true;
            }
            if (what == 5) {                                          // a layer range that leaves [0, L] or runs backwards
                if (b == 0) t.layer_off[0] = -1;
                else if (b == last_b) t.layer_off[(size_t)b + 1] = s.L + 1;
                else continue;                                        // a middle offset is the next image's too: the last one, below
            }
            check(t, r, no_layer, __LINE__);
        }
    }
    if (s.layer_off[(size_t)last_b] >= 1) {                           // the last image's range runs backwards
        Scene t = s;
        std::vector<bool> r = no_image;
        r[(size_t)last_b] = true;
        t.layer_off[(size_t)s.B] = s.layer_off[(size_t)last_b] - 1;
        check(t, r, no_layer, __LINE__);
    }
    for (int l : {0, s.L / 2, s.L - 1}) {                             // layers skipped as if absent
        std::vector<bool> skipped = no_layer;
        skipped[(size_t)l] = true;
        const int kind = (int)(s.layers[4 * (size_t)l] & 0xff);
        const int64_t huge = (int64_t)1 << 62;
        const int64_t words[] = {3, -1, (int64_t)kind | 4 << 8, (int64_t)kind | (kind == 0 ? 1 : 2) << 8, (int64_t)1 << 40};
        for (int64_t word : words) {
            Scene t = s;
            t.layers[4 * (size_t)l] = word;
            check(t, no_image, skipped, __LINE__);
        }
        const int64_t full = kind == 0 ? (int64_t)s.bits.size() : kind == 1 ? (int64_t)s.levels.size() : (int64_t)s.labels.size();
        const int64_t srcs[] = {-4, full, full + 4, huge, kind == 0 ? s.layers[4 * (size_t)l + 1] + 2 : -1};
        for (int64_t src : srcs) {
            Scene t = s;
            t.layers[4 * (size_t)l + 1] = src;
            check(t, no_image, skipped, __LINE__);
        }
        const int64_t firsts[] = {-1, (int64_t)s.T, (int64_t)s.T + 1, huge};
        for (int64_t first : firsts) {
            Scene t = s;
            t.layers[4 * (size_t)l + 2] = first;
            if (first == s.T && kind == 2) t.layers[4 * (size_t)l + 3] = 1;
            check(t, no_image, skipped, __LINE__);
        }
        const int64_t rows[] = {-1, (int64_t)s.T + 1, huge, kind == 2 ? -2 : 2, kind == 2 ? -3 : 255};
        for (int64_t n : rows) {
            Scene t = s;
            t.layers[4 * (size_t)l + 3] = n;
            check(t, no_image, skipped, __LINE__);
        }
    }
    {                                                                 // a slice that ends exactly at its buffer's end is taken: the last of each kind
        for (int kind = 0; kind < 3; ++kind)
            for (int l = s.L - 1; l >= 0; --l)
                if ((s.layers[4 * (size_t)l] & 0xff) == kind) {
                    Scene t = s;
                    t.layers[4 * (size_t)l + 1] += kind == 0 ? 4 : 1; // and one step further it is not
                    std::vector<bool> skipped = no_layer;
                    skipped[(size_t)l] = true;
                    bool is_last = true;
                    for (int m = l + 1; m < s.L; ++m) is_last = is_last && (s.layers[4 * (size_t)m] & 0xff) != kind;
                    if (is_last) check(t, no_image, skipped, __LINE__);
                    break;
                }
    }
    for (float bad : {std::numeric_limits<float>::quiet_NaN(), -0.5f, 1.5f, std::numeric_limits<float>::infinity()}) {
        Scene t = s;                                                  // table rows that paint nothing: the reference counts them on use
        for (int k = 0; k < s.T; k += 3) t.alpha[(size_t)k] = bad;
        check(t, no_image, no_layer, __LINE__);
    }
    {                                                                 // refused arguments: nothing is read, nothing written
        std::vector<uint8_t> got;
        int status = 0;
        Scene t = s;
        t.B = 0;
        EXPECT(run(t, false, got, status) == CVLM_E_BADARG && status == -1);
        t = s; t.T = 0;
        EXPECT(run(t, false, got, status) == CVLM_E_BADARG && status == -1);
        t = s; t.L = -1;
        EXPECT(run(t, false, got, status) == CVLM_E_BADARG && status == -1);
        t = s; t.max_pixels = 0;
        EXPECT(run(t, true, got, status) == CVLM_E_BADARG && status == -1 && got == s.img);
    }
    if (failures) {
        printf("render_host_sanitize: %d FAILURES in %d calls\n", failures, calls);
        return 1;
    }
    printf("render_host_sanitize: %d calls, every refusal at three positions, in place and apart: ok\n", calls);
    return 0;
}
