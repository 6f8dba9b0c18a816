// Stand-alone check of cvlm_debug_mask_rle_host for a host sanitizer: the entry's per-thread functions are the
// kernels' (csrc/rle_logic.h), so their indexing is what runs on the device.  Every buffer is a heap block of exactly the size the
// interface states, so that AddressSanitizer sees any access beyond it; the counts are held against a plain pixel loop.  Build and
// run on the CPU, from the repository root:
//   hipcc -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/rle_host_sanitize.cpp camouflaged-vlm_amd/csrc/rle.hip -o /tmp/rle_host_sanitize && /tmp/rle_host_sanitize
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/cvlm.h"

namespace {

uint32_t rng_state = 12345u;
uint32_t rng() { return rng_state = rng_state * 1664525u + 1013904223u; }

// pixel (y, x) of a plane in numpy.packbits' order
bool pixel(const uint8_t* plane, int W, int y, int x) {
    const int64_t i = (int64_t)y * W + x;
    return (plane[i >> 3] >> (7 - (i & 7))) & 1;
}

std::vector<int32_t> loop_counts(const uint8_t* plane, int H, int W) {
    std::vector<int32_t> c;
    int value = 0, run = 0;
    for (int x = 0; x < W; ++x)
        for (int y = 0; y < H; ++y) {
            const int v = pixel(plane, W, y, x);
            if (v != value) { c.push_back(run); value = v; run = 0; }
            ++run;
        }
    c.push_back(run);
    return c;
}

int check(int P, int H, int W, int density_percent, int shorten_last) {
    const int64_t plane_bytes = (int64_t)H * W / 8;
    uint8_t* bits = (uint8_t*)malloc((size_t)(P * plane_bytes));
    for (int64_t i = 0; i < P * plane_bytes; ++i) {
        uint8_t b = 0;
        for (int k = 0; k < 8; ++k) b = (uint8_t)(b << 1 | ((int)(rng() >> 8) % 100 < density_percent));
        bits[i] = b;
    }
    int32_t* n_runs = (int32_t*)malloc(sizeof(int32_t) * P);
    int bad = cvlm_debug_mask_rle_host((const uint32_t*)bits, P, H, W, n_runs, nullptr, nullptr, 0, nullptr) != 0;
    int64_t* offsets = (int64_t*)malloc(sizeof(int64_t) * (P + 1));
    offsets[0] = 0;
    for (int p = 0; p < P; ++p) offsets[p + 1] = offsets[p] + n_runs[p] - (p == P - 1 ? shorten_last : 0);
    const int64_t total = offsets[P];
    int32_t* counts = (int32_t*)malloc(sizeof(int32_t) * (size_t)total);
    int32_t* status = (int32_t*)malloc(sizeof(int32_t));
    bad |= cvlm_debug_mask_rle_host((const uint32_t*)bits, P, H, W, n_runs, offsets, counts, total, status) != 0;
    bad |= status[0] != (shorten_last ? 1 : 0);
    for (int p = 0; p < P; ++p) {
        const std::vector<int32_t> want = loop_counts(bits + p * plane_bytes, H, W);
        bad |= (int)want.size() != n_runs[p];
        for (int64_t k = 0; k < offsets[p + 1] - offsets[p] && k < (int64_t)want.size(); ++k) bad |= counts[offsets[p] + k] != want[(size_t)k];
    }
    printf("%s  P = %d, %d x %d, density %d %%, last slice %d short: %lld counts\n", bad ? "FAIL" : "ok  ", P, H, W, density_percent,
           shorten_last, (long long)total);
    free(status); free(counts); free(offsets); free(n_runs); free(bits);
    return bad;
}

}  // namespace

int main() {
    int bad = 0;
    const int shapes[][2] = {{1, 32}, {1, 64}, {8, 64}, {31, 64}, {32, 64}, {33, 64}, {65, 96}, {130, 544}, {256, 1024}};
    for (const auto& s : shapes)
        for (int density : {0, 1, 50, 99, 100}) bad |= check(3, s[0], s[1], density, 0);
    bad |= check(3, 33, 64, 50, 1);                                   // an undersized slot: the dropped stores must not happen
    bad |= check(2, 65, 96, 50, 40);
    printf(bad ? "FAILED\n" : "all equal to the pixel loop\n");
    return bad;
}
