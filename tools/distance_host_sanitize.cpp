// Stand-alone check of cvlm_debug_mask_distance_sized_host and cvlm_debug_mask_surface_totals_host for a host sanitizer:
// the entries run the kernels' per-thread functions (csrc/distance_logic.h), so their indexing is what runs on the device.  Every
// buffer is a heap block of exactly the size the interface states, so that AddressSanitizer sees any access beyond it.  The maps are
// held against the definition -- the minimum over every set pixel, cut at the reach -- and the totals against a plain loop over the
// map.  Ragged sizes, dirty pad bits, each kind of refused plane at the first, a middle and the last position, refused pairs, and every
// CVLM_E_BADARG of both entries.
// Build and run on the CPU, from the repository root:
//   hipcc -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/distance_host_sanitize.cpp camouflaged-vlm_amd/csrc/distance.hip -o /tmp/distance_host_sanitize && /tmp/distance_host_sanitize
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/cvlm.h"

namespace {

constexpr int32_t FAR = 0x7fffffff;
uint32_t rng_state = 2027u;
uint32_t rng() { return rng_state = rng_state * 1664525u + 1013904223u; }

template <typename T>
T* block(size_t n) { return (T*)malloc(n ? n * sizeof(T) : 1); }      // exact size: no slack behind the last element

bool pixel(const uint8_t* plane, int ws, int y, int x) { return (plane[(int64_t)y * 4 * ws + (x >> 3)] >> (7 - (x & 7))) & 1; }

int32_t defined(const uint8_t* plane, int h, int w, int y, int x, int R) {
    const int ws = (w + 31) / 32;
    int64_t best = -1;
    for (int yy = 0; yy < h; ++yy)
        for (int xx = 0; xx < w; ++xx)
            if (pixel(plane, ws, yy, xx)) {
                const int64_t d = (int64_t)(y - yy) * (y - yy) + (int64_t)(x - xx) * (x - xx);
                if (best < 0 || d < best) best = d;
            }
    return best < 0 || (R && best > (int64_t)R * R) ? FAR : (int32_t)best;
}

enum Refusal { NONE, HEIGHT_ZERO, WIDTH_HUGE, WRONG_SIZE, REACH_NEGATIVE, REACH_HUGE, PIX_SHORT };
const int SIZES[7][2] = {{1, 1}, {20, 33}, {5, 65}, {33, 31}, {1, 32}, {17, 70}, {2, 64}};

// one call on the seven planes with plane `at` refused in the way `how` -> the number of wrong entries
int distance_case(Refusal how, int at, bool dirty) {
    const int P = 7;
    int64_t off[P + 1] = {0}, pix[P + 1] = {0};
    int32_t dims[2 * P], reach[P];
    int64_t max_words = 0;
    for (int p = 0; p < P; ++p) {
        const int h = SIZES[p][0], w = SIZES[p][1], ws = (w + 31) / 32;
        dims[2 * p] = h; dims[2 * p + 1] = w;
        reach[p] = p % 3 == 0 ? 0 : p % 3 == 1 ? 3 : 40;
        off[p + 1] = off[p] + 4 * h * ws;
        pix[p + 1] = pix[p] + h * w;
        if ((int64_t)h * ws > max_words) max_words = (int64_t)h * ws;
    }
    uint8_t* bits = block<uint8_t>(off[P]);
    for (int p = 0; p < P; ++p) {
        const int h = SIZES[p][0], w = SIZES[p][1], ws = (w + 31) / 32;
        const uint32_t density = p == 4 ? 0u : p == 1 ? 40u : 900u;   // per 1024: an empty plane, a sparse one, dense ones
        uint8_t* plane = bits + off[p];
        memset(plane, 0, (size_t)(off[p + 1] - off[p]));
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < 32 * ws; ++x)
                if (x < w ? rng() % 1024u < density : dirty) plane[(int64_t)y * 4 * ws + (x >> 3)] |= (uint8_t)(0x80 >> (x & 7));
    }
    int64_t* offsets = block<int64_t>(P + 1);
    int64_t* pix_offsets = block<int64_t>(P + 1);
    memcpy(offsets, off, sizeof off);
    memcpy(pix_offsets, pix, sizeof pix);
    int32_t* d = block<int32_t>(2 * P);
    int32_t* r = block<int32_t>(P);
    memcpy(d, dims, sizeof dims);
    memcpy(r, reach, sizeof reach);
    bool both = false;                                                // PIX_SHORT moves a seam: the neighbour before it is refused too
    switch (how) {
        case HEIGHT_ZERO: d[2 * at] = 0; break;
        case WIDTH_HUGE: d[2 * at + 1] = 16385; break;
        case WRONG_SIZE: d[2 * at] += 1; break;
        case REACH_NEGATIVE: r[at] = -1; break;
        case REACH_HUGE: r[at] = 23171; break;
        case PIX_SHORT: if (at > 0) { pix_offsets[at] += 1; both = true; } else pix_offsets[0] = -1; break;
        case NONE: break;
    }
    const int64_t n_pix = pix[P], ws_bytes = (2 * n_pix + 15) / 16 * 16;
    void* ws = aligned_alloc(16, (size_t)ws_bytes);
    int32_t* out = block<int32_t>(n_pix);
    for (int64_t i = 0; i < n_pix; ++i) out[i] = -7;
    int32_t* status = block<int32_t>(1);
    const int rc = cvlm_debug_mask_distance_sized_host(bits, off[P], offsets, d, r, P, max_words, pix_offsets, n_pix, ws, ws_bytes, out, status);
    int bad = rc != 0;
    bad += status[0] != (how != NONE);
    for (int p = 0; p < P; ++p) {
        const int h = SIZES[p][0], w = SIZES[p][1];
        const bool refused = how != NONE && (p == at || (both && p == at - 1));
        const bool untouched = how == PIX_SHORT && at == 0 && p == 0;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const int32_t got = out[pix[p] + (int64_t)y * w + x];
                const int32_t want = untouched ? -7 : refused ? FAR : defined(bits + off[p], h, w, y, x, reach[p]);
                bad += got != want;
            }
    }
    free(bits); free(offsets); free(pix_offsets); free(d); free(r); free(ws); free(out); free(status);
    return bad;
}

// the totals of pairs of the same planes against maps made by the distance entry; pair 2 is refused in the way `how`
int totals_case(int how) {
    const int P = 3, h = 9, w = 40, ws = 2, T = 3, N = 4;
    int64_t off[P + 1], pix[P + 1];
    int32_t dims[2 * P], reach[P] = {0, 0, 5};
    for (int p = 0; p <= P; ++p) { off[p] = (int64_t)p * 4 * h * ws; pix[p] = (int64_t)p * h * w; }
    for (int p = 0; p < P; ++p) { dims[2 * p] = h; dims[2 * p + 1] = w; }
    uint8_t* bits = block<uint8_t>(off[P]);
    for (int64_t i = 0; i < off[P]; ++i) bits[i] = i < off[1] ? (uint8_t)(rng() & rng()) : i < off[2] ? 0 : (uint8_t)(rng() & rng() & rng());
    int64_t* offsets = block<int64_t>(P + 1);
    int64_t* pix_offsets = block<int64_t>(P + 1);
    int32_t* d = block<int32_t>(2 * P);
    int32_t* r = block<int32_t>(P);
    memcpy(offsets, off, sizeof off); memcpy(pix_offsets, pix, sizeof pix); memcpy(d, dims, sizeof dims); memcpy(r, reach, sizeof reach);
    const int64_t n_pix = pix[P], ws_bytes = (2 * n_pix + 15) / 16 * 16;
    void* dws = aligned_alloc(16, (size_t)ws_bytes);
    int32_t* map = block<int32_t>(n_pix);
    int32_t* status = block<int32_t>(1);
    int bad = cvlm_debug_mask_distance_sized_host(bits, off[P], offsets, d, r, P, h * ws, pix_offsets, n_pix, dws, ws_bytes, map, status) != 0;
    int32_t* pairs = block<int32_t>(2 * N);
    int32_t* radii = block<int32_t>(N * T);
    const int32_t pr[2 * N] = {0, 2, 1, 0, 2, 0, 2, 1};
    memcpy(pairs, pr, sizeof pr);
    for (int i = 0; i < N * T; ++i) radii[i] = i % T == 0 ? 0 : i % T == 1 ? 2 : 23170;
    int32_t* bd = block<int32_t>(2 * P);
    memcpy(bd, dims, sizeof dims);
    if (how == 1) pairs[4] = 3;
    if (how == 2) pairs[5] = -1;
    if (how == 3) radii[2 * T + 1] = 23171;
    if (how == 4) bd[1] = 39;                                         // map 0 is another size: pairs 1 and 2 name it
    const int64_t sws_bytes = cvlm_mask_surface_workspace_bytes(N);
    void* sws = aligned_alloc(16, (size_t)sws_bytes);
    int32_t* n = block<int32_t>(N); int32_t* far = block<int32_t>(N); int32_t* within = block<int32_t>(N * T); int32_t* mx = block<int32_t>(N);
    int64_t* s2 = block<int64_t>(N);
    double* sd = block<double>(N);
    bad += cvlm_debug_mask_surface_totals_host(bits, off[P], offsets, d, P, map, pix_offsets, n_pix, bd, P, pairs, N, radii, T, h * ws, sws,
                                               sws_bytes, n, far, within, mx, s2, sd, status) != 0;
    bad += status[0] != (how != 0);
    for (int i = 0; i < N; ++i) {
        const bool refused = (how >= 1 && how <= 3 && i == 2) || (how == 4 && (i == 1 || i == 2));
        int wn = 0, wfar = 0, wmx = -1, ww[T] = {0, 0, 0};
        int64_t ws2 = 0;
        double wsd = 0.0;
        if (refused) {
            wn = wfar = wmx = -1; ws2 = -1; ww[0] = ww[1] = ww[2] = -1;
        } else {
            const uint8_t* plane = bits + off[pr[2 * i]];
            const int32_t* m = map + pix[pr[2 * i + 1]];
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    if (!pixel(plane, ws, y, x)) continue;
                    ++wn;
                    const int32_t v = m[y * w + x];
                    if (v == FAR) { ++wfar; continue; }
                    for (int k = 0; k < T; ++k) ww[k] += (int64_t)v <= (int64_t)radii[i * T + k] * radii[i * T + k];
                    if (v > wmx) wmx = v;
                    ws2 += v;
                    wsd += std::sqrt((double)v);
                }
        }
        bad += n[i] != wn || far[i] != wfar || mx[i] != wmx || s2[i] != ws2 || sd[i] != wsd;
        for (int k = 0; k < T; ++k) bad += within[i * T + k] != ww[k];
    }
    // CVLM_E_BADARG of the totals entry, on these sound buffers
    if (how == 0) {
        auto call = [&](const uint8_t* a, int32_t Pa, int64_t NN, int32_t TT, int64_t mw, void* w_, int64_t wb, int32_t* n_, double* sd_) {
            return cvlm_debug_mask_surface_totals_host(a, off[P], offsets, d, Pa, map, pix_offsets, n_pix, bd, P, pairs, NN, radii, TT, mw, w_, wb,
                                                       n_, far, within, mx, s2, sd_, status);
        };
        bad += call(nullptr, P, N, T, h * ws, sws, sws_bytes, n, sd) != CVLM_E_BADARG;
        bad += call(bits, 0, N, T, h * ws, sws, sws_bytes, n, sd) != CVLM_E_BADARG;
        bad += call(bits, 65536, N, T, h * ws, sws, sws_bytes, n, sd) != CVLM_E_BADARG;
        bad += call(bits, P, 0, T, h * ws, sws, sws_bytes, n, sd) != CVLM_E_BADARG;
        bad += call(bits, P, ((int64_t)1 << 24) + 1, T, h * ws, sws, sws_bytes, n, sd) != CVLM_E_BADARG;
        bad += call(bits, P, N, 0, h * ws, sws, sws_bytes, n, sd) != CVLM_E_BADARG;
        bad += call(bits, P, N, 9, h * ws, sws, sws_bytes, n, sd) != CVLM_E_BADARG;
        bad += call(bits, P, N, T, 0, sws, sws_bytes, n, sd) != CVLM_E_BADARG;
        bad += call(bits, P, N, T, h * ws, (uint8_t*)sws + 8, sws_bytes, n, sd) != CVLM_E_BADARG;
        bad += call(bits, P, N, T, h * ws, sws, sws_bytes - 16, n, sd) != CVLM_E_WORKSPACE;
        bad += call(bits, P, N, T, h * ws, sws, sws_bytes, far, sd) != CVLM_E_BADARG;                 // two outputs that meet
        bad += call(bits, P, N, T, h * ws, sws, sws_bytes, n, (double*)s2) != CVLM_E_BADARG;
        bad += call(bits, P, N, T, h * ws, sws, sws_bytes, (int32_t*)((uint8_t*)n + 2), sd) != CVLM_E_BADARG;
    }
    free(bits); free(offsets); free(pix_offsets); free(d); free(r); free(dws); free(map); free(status); free(pairs); free(radii); free(bd);
    free(sws); free(n); free(far); free(within); free(mx); free(s2); free(sd);
    return bad;
}

// CVLM_E_BADARG of the distance entry
int distance_badargs() {
    const int h = 3, w = 40, ws = 2;
    int64_t* offsets = block<int64_t>(2);
    int64_t* pix = block<int64_t>(2);
    offsets[0] = 0; offsets[1] = 4 * h * ws; pix[0] = 0; pix[1] = h * w;
    int32_t* dims = block<int32_t>(2);
    dims[0] = h; dims[1] = w;
    int32_t* reach = block<int32_t>(1);
    reach[0] = 0;
    uint8_t* bits = block<uint8_t>(4 * h * ws);
    memset(bits, 0x5a, 4 * h * ws);
    const int64_t n_pix = h * w, wb = (2 * n_pix + 15) / 16 * 16;
    void* wsp = aligned_alloc(16, (size_t)wb);
    int32_t* out = block<int32_t>(n_pix);
    int32_t* status = block<int32_t>(1);
    auto call = [&](const uint8_t* b, int64_t nb, int32_t P, int64_t mw, int64_t np, void* w_, int64_t wb_, int32_t* o, int32_t* s) {
        return cvlm_debug_mask_distance_sized_host(b, nb, offsets, dims, reach, P, mw, pix, np, w_, wb_, o, s);
    };
    int bad = call(bits, 4 * h * ws, 1, h * ws, n_pix, wsp, wb, out, status) != 0;
    bad += call(nullptr, 4 * h * ws, 1, h * ws, n_pix, wsp, wb, out, status) != CVLM_E_BADARG;
    bad += call(bits + 2, 4 * h * ws, 1, h * ws, n_pix, wsp, wb, out, status) != CVLM_E_BADARG;
    bad += call(bits, 3, 1, h * ws, n_pix, wsp, wb, out, status) != CVLM_E_BADARG;
    bad += call(bits, 4 * h * ws, 0, h * ws, n_pix, wsp, wb, out, status) != CVLM_E_BADARG;
    bad += call(bits, 4 * h * ws, 65536, h * ws, n_pix, wsp, wb, out, status) != CVLM_E_BADARG;
    bad += call(bits, 4 * h * ws, 1, 0, n_pix, wsp, wb, out, status) != CVLM_E_BADARG;
    bad += call(bits, 4 * h * ws, 1, 16384 * 512 + 1, n_pix, wsp, wb, out, status) != CVLM_E_BADARG;
    bad += call(bits, 4 * h * ws, 1, h * ws, 0, wsp, wb, out, status) != CVLM_E_BADARG;
    bad += call(bits, 4 * h * ws, 1, h * ws, n_pix, nullptr, wb, out, status) != CVLM_E_BADARG;
    bad += call(bits, 4 * h * ws, 1, h * ws, n_pix, (uint8_t*)wsp + 4, wb, out, status) != CVLM_E_BADARG;
    bad += call(bits, 4 * h * ws, 1, h * ws, n_pix, wsp, wb - 16, out, status) != CVLM_E_WORKSPACE;
    bad += call(bits, 4 * h * ws, 1, h * ws, n_pix, wsp, wb, (int32_t*)wsp, status) != CVLM_E_BADARG;     // the output meets the workspace
    bad += call(bits, 4 * h * ws, 1, h * ws, n_pix, wsp, wb, (int32_t*)bits, status) != CVLM_E_BADARG;    // ... the input
    bad += call(bits, 4 * h * ws, 1, h * ws, n_pix, wsp, wb, out, out) != CVLM_E_BADARG;                  // ... the status
    bad += call(bits, 4 * h * ws, 1, h * ws, n_pix, wsp, wb, out, nullptr) != CVLM_E_BADARG;
    free(offsets); free(pix); free(dims); free(reach); free(bits); free(wsp); free(out); free(status);
    return bad;
}

}  // namespace

int main() {
    int bad = 0, cases = 0;
    for (int dirty = 0; dirty < 2; ++dirty) {
        bad += distance_case(NONE, 0, dirty != 0);
        ++cases;
        for (int how = HEIGHT_ZERO; how <= PIX_SHORT; ++how)
            for (int at : {0, 3, 6}) {
                bad += distance_case((Refusal)how, at, dirty != 0);
                ++cases;
            }
    }
    for (int how = 0; how <= 4; ++how) {
        bad += totals_case(how);
        ++cases;
    }
    bad += distance_badargs();
    printf("distance_host_sanitize: %d cases, %d wrong\n", cases, bad);
    return bad != 0;
}
