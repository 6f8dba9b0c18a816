// Stand-alone check of cvlm_debug_mask_thin_sized_host for a host sanitizer: the entry runs the kernels' own word
// function (csrc/thin_logic.h), so its indexing is what runs on the device.  Every buffer is a heap block of exactly the size the
// interface states, so that AddressSanitizer sees any access beyond it; the sizes are ragged, the pad bits dirty, a refused plane sits
// at the first, a middle and the last position, every CVLM_E_BADARG and CVLM_E_WORKSPACE is tried, and the result is held against a
// per-pixel loop written from the definition.
// Build and run on the CPU, from the repository root:
//   hipcc -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/thin_host_sanitize.cpp camouflaged-vlm_amd/csrc/thin.hip -o /tmp/thin_host_sanitize && /tmp/thin_host_sanitize
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../include/cvlm.h"

namespace {

uint32_t rng_state = 2026u;
uint32_t rng() { return rng_state = rng_state * 1664525u + 1013904223u; }

typedef std::vector<uint8_t> Plane;                                   // h * w bytes, 0 or 1

int at(const Plane& x, int h, int w, int y, int xx) { return y >= 0 && y < h && xx >= 0 && xx < w ? x[(size_t)y * w + xx] : 0; }

// one subiteration, pixel by pixel, from the definition -> true if a pixel was cleared
bool subiteration(Plane& x, int h, int w, bool second) {
    Plane out = x;
    bool cleared = false;
    for (int y = 0; y < h; ++y)
        for (int c = 0; c < w; ++c) {
            if (!x[(size_t)y * w + c]) continue;
            int v[10];
            v[1] = at(x, h, w, y, c + 1); v[2] = at(x, h, w, y - 1, c + 1); v[3] = at(x, h, w, y - 1, c); v[4] = at(x, h, w, y - 1, c - 1);
            v[5] = at(x, h, w, y, c - 1); v[6] = at(x, h, w, y + 1, c - 1); v[7] = at(x, h, w, y + 1, c); v[8] = at(x, h, w, y + 1, c + 1);
            v[9] = v[1];
            int xh = 0, n1 = 0, n2 = 0;
            for (int i = 1; i <= 4; ++i) {
                xh += !v[2 * i - 1] && (v[2 * i] || v[2 * i + 1]);
                n1 += v[2 * i - 1] || v[2 * i];
                n2 += v[2 * i] || v[2 * i + 1];
            }
            const int low = n1 < n2 ? n1 : n2;
            const bool g3 = second ? !((v[6] || v[7] || !v[4]) && v[5]) : !((v[2] || v[3] || !v[8]) && v[1]);
            if (xh == 1 && low >= 2 && low <= 3 && g3) {
                out[(size_t)y * w + c] = 0;
                cleared = true;
            }
        }
    x = out;
    return cleared;
}

int thin(Plane& x, int h, int w, int max_iter) {
    int it = 0;
    while (max_iter == 0 || it < max_iter) {
        const bool a = subiteration(x, h, w, false), b = subiteration(x, h, w, true);
        if (!a && !b) break;
        ++it;
    }
    return it;
}

enum Refusal { NONE, SHORT_SLICE, ODD_OFFSET, PAST_THE_END, ITER_NEGATIVE, ITER_HUGE, HEIGHT_ZERO, WIDTH_HUGE };

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

// one call over planes of the given sizes and limits; plane `bad_plane` is doctored as `how` says and must be refused
int check_thin(const std::vector<std::pair<int, int>>& sizes, const std::vector<int>& limits, int density_percent, int bad_plane, Refusal how,
               bool with_stats, int mode, int steps) {
    const int P = (int)sizes.size();
    int32_t* dims = (int32_t*)malloc(sizeof(int32_t) * 2 * P);
    int32_t* max_iter = (int32_t*)malloc(sizeof(int32_t) * P);
    int64_t* offsets = (int64_t*)malloc(sizeof(int64_t) * (P + 1));
    std::vector<int64_t> true_off((size_t)P + 1, 0);
    int64_t max_words = 1;
    for (int p = 0; p < P; ++p) {
        dims[2 * p] = sizes[p].first;
        dims[2 * p + 1] = sizes[p].second;
        max_iter[p] = limits[p];
        const int64_t words = (int64_t)sizes[p].first * ((sizes[p].second + 31) / 32);
        max_words = words > max_words ? words : max_words;
        true_off[p + 1] = true_off[p] + 4 * words;
    }
    const int64_t nbytes = true_off[P];
    for (int p = 0; p <= P; ++p) offsets[p] = true_off[p];
    // what is refused besides bad_plane: a doctored offset is shared with the plane before it
    std::vector<int> refused((size_t)P, 0), untouched((size_t)P, 0);
    if (bad_plane >= 0) {
        refused[bad_plane] = 1;
        if (how == SHORT_SLICE && bad_plane + 1 < P) { offsets[bad_plane + 1] -= 4; refused[bad_plane + 1] = 1; }
        if (how == SHORT_SLICE && bad_plane + 1 == P) { offsets[bad_plane] += 4; refused[bad_plane - 1] = 1; }      // the last plane: short at its start
        if (how == ODD_OFFSET) { offsets[bad_plane] += 2; untouched[bad_plane] = 1; if (bad_plane > 0) refused[bad_plane - 1] = untouched[bad_plane - 1] = 1; }
        if (how == PAST_THE_END) { offsets[P] += 4; refused[bad_plane] = 0; refused[P - 1] = untouched[P - 1] = 1; }
        if (how == ITER_NEGATIVE) max_iter[bad_plane] = -1;
        if (how == ITER_HUGE) max_iter[bad_plane] = (1 << 30) + 1;
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
    const int64_t need = cvlm_mask_thin_workspace_bytes(nbytes, P, steps);
    if (need < nbytes) FAIL("workspace_bytes %lld", (long long)need);
    uint8_t* workspace = (uint8_t*)aligned_alloc(16, (size_t)need);
    uint8_t* out = (uint8_t*)malloc((size_t)nbytes);
    memset(out, 0xA5, (size_t)nbytes);
    int32_t* area = with_stats ? (int32_t*)malloc(sizeof(int32_t) * P) : nullptr;
    int32_t* box = with_stats ? (int32_t*)malloc(sizeof(int32_t) * 4 * P) : nullptr;
    int32_t* iters = (int32_t*)malloc(sizeof(int32_t) * P);
    int32_t* done = (int32_t*)malloc(sizeof(int32_t) * P);
    int32_t* status = (int32_t*)malloc(sizeof(int32_t));
    status[0] = 77;
    const int rc = cvlm_debug_mask_thin_sized_host(bits, nbytes, offsets, dims, max_iter, P, max_words, mode, steps, workspace, need, out, area,
                                                   box, iters, done, status);
    if (rc != 0) FAIL("rc %d", rc);
    if (status[0] != (bad_plane >= 0 ? 1 : 0)) FAIL("status %d", status[0]);
    for (int p = 0; p < P; ++p) {
        const int h = sizes[p].first, w = sizes[p].second, ws = (w + 31) / 32;
        const uint8_t* got = out + true_off[p];
        if (refused[p]) {
            for (int64_t i = 0; i < (int64_t)4 * h * ws; ++i)
                if (got[i] != (untouched[p] ? 0xA5 : 0)) FAIL("plane %d: a refused slice holds %d", p, got[i]);
            if (iters[p] != 0 || done[p] != 0 || (with_stats && (area[p] != 0 || box[4 * p] != -1 || box[4 * p + 3] != -1))) FAIL("plane %d: refused outputs", p);
            continue;
        }
        Plane want = planes[p];
        const int n = thin(want, h, w, limits[p]);
        if (iters[p] != n || done[p] != 1) FAIL("plane %d: iters %d, want %d, done %d", p, iters[p], n, done[p]);
        int cnt = 0, x0 = -1, y0 = -1, x1 = -1, y1 = -1;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < 32 * ws; ++x) {
                const int bit = (got[(int64_t)y * 4 * ws + (x >> 3)] >> (7 - (x & 7))) & 1;
                if (bit != (x < w ? want[(size_t)y * w + x] : 0)) FAIL("plane %d (%d x %d): pixel (%d, %d) is %d", p, h, w, y, x, bit);
                if (bit) {
                    ++cnt;
                    x0 = x0 < 0 || x < x0 ? x : x0; y0 = y0 < 0 ? y : y0;
                    x1 = x > x1 ? x : x1; y1 = y;
                }
            }
        if (with_stats && (area[p] != cnt || box[4 * p] != x0 || box[4 * p + 1] != y0 || box[4 * p + 2] != x1 || box[4 * p + 3] != y1))
            FAIL("plane %d: area %d (%d), box %d %d %d %d (%d %d %d %d)", p, area[p], cnt, box[4 * p], box[4 * p + 1], box[4 * p + 2],
                 box[4 * p + 3], x0, y0, x1, y1);
    }
    free(dims); free(max_iter); free(offsets); free(bits); free(workspace); free(out); free(area); free(box); free(iters); free(done); free(status);
    return 0;
}

// every CVLM_E_BADARG and CVLM_E_WORKSPACE on two small planes
int check_badargs() {
    const int P = 2;
    int32_t dims[4] = {5, 40, 3, 7};
    int64_t offsets[3] = {0, 40, 52};
    int32_t max_iter[2] = {0, 1};
    const int64_t nbytes = 52, max_words = 10;
    const int steps = 2;
    const int64_t need = cvlm_mask_thin_workspace_bytes(nbytes, P, steps);
    if (need != 64 + 16) FAIL("workspace_bytes %lld", (long long)need);
    if (cvlm_mask_thin_workspace_bytes(3, 1, 1) != -1 || cvlm_mask_thin_workspace_bytes(8, 0, 1) != -1 || cvlm_mask_thin_workspace_bytes(8, 65536, 1) != -1 ||
        cvlm_mask_thin_workspace_bytes(8, 1, -1) != -1 || cvlm_mask_thin_workspace_bytes(8, 1, 1025) != -1)
        FAIL("workspace_bytes takes arguments out of range");
    if (cvlm_mask_thin_resident(1024, 1024) != 1 || cvlm_mask_thin_resident(1143, 1024) != 0 || cvlm_mask_thin_resident(0, 4) != 0 ||
        cvlm_mask_thin_resident(4, 16385) != 0)
        FAIL("cvlm_mask_thin_resident");
    uint8_t* block = (uint8_t*)aligned_alloc(16, 64 + (size_t)need + 64);             // bits, workspace, out_bits: 16-byte aligned each
    memset(block, 0, 64 + (size_t)need + 64);
    uint8_t *bits = block, *ws = block + 64, *out = block + 64 + need;
    int32_t area[2], box[8], iters[2], done[2], status[1];
    struct Args {
        const uint8_t* bits; int64_t n; const int64_t* off; const int32_t* dims; const int32_t* mi; int32_t P; int64_t mw; int32_t mode, steps;
        void* ws; int64_t wsb; uint8_t* out; int32_t *area, *box, *iters, *done, *status;
    };
    const Args good = {bits, nbytes, offsets, dims, max_iter, P, max_words, 0, steps, ws, need, out, area, box, iters, done, status};
    auto call = [](const Args& a) {
        return cvlm_debug_mask_thin_sized_host(a.bits, a.n, a.off, a.dims, a.mi, a.P, a.mw, a.mode, a.steps, a.ws, a.wsb, a.out, a.area, a.box,
                                               a.iters, a.done, a.status);
    };
    if (call(good) != 0) FAIL("the good call fails");
    std::vector<Args> bad;
    Args a;
#define BAD(stmt) a = good; stmt; bad.push_back(a)
    BAD(a.bits = nullptr); BAD(a.off = nullptr); BAD(a.dims = nullptr); BAD(a.mi = nullptr); BAD(a.ws = nullptr); BAD(a.out = nullptr);
    BAD(a.iters = nullptr); BAD(a.done = nullptr); BAD(a.status = nullptr); BAD(a.area = nullptr); BAD(a.box = nullptr);
    BAD(a.bits = bits + 2); BAD(a.dims = (const int32_t*)((const uint8_t*)dims + 2)); BAD(a.mi = (const int32_t*)((const uint8_t*)max_iter + 2));
    BAD(a.out = out + 2); BAD(a.area = (int32_t*)((uint8_t*)area + 2)); BAD(a.box = (int32_t*)((uint8_t*)box + 2));
    BAD(a.iters = (int32_t*)((uint8_t*)iters + 2)); BAD(a.done = (int32_t*)((uint8_t*)done + 2)); BAD(a.status = (int32_t*)((uint8_t*)status + 2));
    BAD(a.off = (const int64_t*)((const uint8_t*)offsets + 4)); BAD(a.ws = ws + 8);
    BAD(a.P = 0); BAD(a.P = 65536); BAD(a.n = 3); BAD(a.mw = 0); BAD(a.mw = (int64_t)16384 * 512 + 1); BAD(a.mode = -1); BAD(a.mode = 2);
    BAD(a.steps = -1); BAD(a.steps = 1025); BAD(a.mode = 1; a.steps = 0); BAD(a.mw = (int64_t)16384 * 512; a.steps = 0);
    BAD(a.out = bits); BAD(a.out = bits + nbytes - 4); BAD(a.ws = bits); BAD(a.out = ws); BAD(a.out = ws + need - 4);
    BAD(a.status = (int32_t*)out); BAD(a.status = (int32_t*)ws); BAD(a.out = (uint8_t*)dims); BAD(a.iters = done); BAD(a.area = box + 1);
    BAD(a.done = (int32_t*)max_iter); BAD(a.box = (int32_t*)out); BAD(a.status = iters + 1);
#undef BAD
    for (size_t i = 0; i < bad.size(); ++i)
        if (call(bad[i]) != CVLM_E_BADARG) FAIL("bad call %zu is taken", i);
    a = good; a.wsb = need - 16;
    if (call(a) != CVLM_E_WORKSPACE) FAIL("a short workspace is taken");
    a = good; a.wsb = 0;
    if (call(a) != CVLM_E_WORKSPACE) FAIL("no workspace is taken");
    a = good; a.area = nullptr; a.box = nullptr;
    if (call(a) != 0) FAIL("the call without areas and boxes fails");
    free(block);
    return 0;
}

}  // namespace

int main() {
    const std::vector<std::pair<int, int>> ragged = {{1, 1}, {70, 33}, {5, 65}, {33, 31}, {1, 32}, {97, 131}, {2, 64}};
    int calls = 0;
    for (int density : {0, 30, 50, 90, 98, 100}) {
        if (check_thin(ragged, {0, 0, 0, 0, 0, 0, 0}, density, -1, NONE, true, 0, 64)) return 1;
        if (check_thin(ragged, {1, 2, 1, 3, 1, 1, 2}, density, -1, NONE, false, 1, 1)) return 1;
        calls += 2;
    }
    for (int bad_plane : {0, 3, 6})
        for (Refusal how : {SHORT_SLICE, ODD_OFFSET, PAST_THE_END, ITER_NEGATIVE, ITER_HUGE, HEIGHT_ZERO, WIDTH_HUGE}) {
            if (check_thin(ragged, {0, 1, 0, 2, 0, 0, 1}, 90, bad_plane, how, true, 0, 3)) {
                fprintf(stderr, "refusal %d at plane %d\n", (int)how, bad_plane);
                return 1;
            }
            ++calls;
        }
    if (check_thin({{200, 300}}, {0}, 100, -1, NONE, true, 0, 0)) return 1;               // 100 iterations, 101 pixels
    if (check_badargs()) return 1;
    printf("thin_host_sanitize: %d calls and every refused argument: ok\n", calls + 1);
    return 0;
}
