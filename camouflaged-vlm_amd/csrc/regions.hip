// Instances of sized planes (include/cvlm.h: cvlm_mask_regions_sized, cvlm_region_alpha): every sized plane split into
// its connected regions, the M largest as sized planes of their own, and the stage-2 alpha of one region.  The labelling is §14's --
// union-find seeded from the horizontal runs of 32-pixel words (components_logic.h, included) -- run per plane through pointers taken
// from the tables of the sized layout (§19), on any mix of sizes in one call.  The per-thread logic that is new -- the cleaned word,
// the table row, the ranks of a word's runs, the gate -- is regions_logic.h, shared with the sequential host entries at the end of
// this file.  All integers but the alpha.
//
// rg_init_kernel     status = 0, n_regions = 0 (it is the counter of the root lists).
// rg_seed_kernel     a thread per word: the word without its pad bits goes to plane (p, 0) of out_bits, which holds the cleaned input
//                    until the last pass overwrites it, and every run of it becomes a region of its own (cc_seed_word).  The same
//                    grid zeroes the M slices of a plane that is refused.
// rg_join_kernel     the neighbour rule (cc_join_word) on the cleaned plane.
// rg_flatten_kernel  components.hip's pass 3: every run start pointed at its root, the roots listed, areas and boxes summed per wave
//                    first.
// rg_select_kernel   one workgroup per plane: n_regions, then M rounds of a block-wide maximum over the roots that count; behind them
//                    the area slot of every root is overwritten with its rank in the table, -1 outside it.
// rg_route_kernel    a thread per word: the ranks of the word's runs are read once (rg_ranks), then the M words of the M output planes
//                    are built in registers and stored whole -- no atomics on out_bits, every word of every slot written once.
// No thread waits for another workgroup: the find and union loops lower a label on every iteration (components_logic.h).
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/cvlm.h"
#include "common.h"
#include "regions_logic.h"

namespace {

// Plane p of the call as every kernel sees it.  ok: sized_logic.h's check of the slice and no more words than the grid covers.
struct rg_plane { int h, w, ws, words; int64_t off, end; bool ok; };
__host__ __device__ inline rg_plane rg_plane_of(int p, const int64_t* offsets, const int32_t* dims, int64_t nbytes, int64_t max_words) {
    rg_plane g;
    g.h = dims[2 * p]; g.w = dims[2 * p + 1];
    g.off = offsets[p]; g.end = offsets[p + 1];
    g.ok = sz_plane_ok(g.h, g.w, g.off, g.end, nbytes);
    g.ws = g.ok ? sz_words_per_row(g.w) : 1;
    g.words = g.ok ? g.h * g.ws : 0;
    if (g.words > max_words) g.ok = false;
    return g;
}
// The plane's workspace.  slot = 0: every plane of the call is in flight, plane p at 112 bytes per byte before it; otherwise the
// planes of a round lie in slots of `slot` bytes, the largest plane's.
__host__ __device__ inline rg_ws rg_ws_of(void* workspace, int64_t slot, int p, int p0, const rg_plane& g) {
    char* base = (char*)workspace + (slot == 0 ? (RG_WS_PER_WORD / 4) * g.off : (int64_t)(p - p0) * slot);
    return rg_workspace(base, g.words);
}

__global__ __launch_bounds__(256) void rg_init_kernel(int P, int* __restrict__ n_regions, int* __restrict__ status) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p == 0) status[0] = 0;
    if (p < P) n_regions[p] = 0;
}

// bits and out_bits never share a byte (rg_bad); out_bits is read back by the passes below, so it is not __restrict__ there
__global__ __launch_bounds__(256) void rg_seed_kernel(const uint8_t* __restrict__ bits, int64_t nbytes, const int64_t* __restrict__ offsets,
                                                      const int* __restrict__ dims, int p0, int64_t max_words, int M, void* workspace,
                                                      int64_t slot, uint8_t* out_bits, int* __restrict__ status) {
    const int p = p0 + blockIdx.y;
    const rg_plane g = rg_plane_of(p, offsets, dims, nbytes, max_words);
    if (!g.ok) {                                                      // the same for every thread of the plane
        if (th_slice_ok(g.off, g.end, nbytes)) {
            uint32_t* z = (uint32_t*)(out_bits + (int64_t)M * g.off);
            const int64_t n = ((int64_t)M * (g.end - g.off)) >> 2;
            for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) z[i] = 0u;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, 1);
        return;
    }
    const int wi = blockIdx.x * 256 + threadIdx.x;
    if (wi >= g.words) return;
    const rg_ws ws = rg_ws_of(workspace, slot, p, p0, g);
    uint32_t* clean = (uint32_t*)(out_bits + rg_out_plane(g.off, g.end, M, 0));
    clean[wi] = rg_clean_word(((const uint32_t*)(bits + g.off))[wi], wi % g.ws, g.w);
    cc_seed_word(clean, wi, g.ws, ws.parent, ws.area, ws.box);
}

__global__ __launch_bounds__(256) void rg_join_kernel(int64_t nbytes, const int64_t* __restrict__ offsets, const int* __restrict__ dims, int p0,
                                                      int64_t max_words, int M, int connectivity, void* workspace, int64_t slot,
                                                      const uint8_t* __restrict__ out_bits) {
    const int p = p0 + blockIdx.y;
    const rg_plane g = rg_plane_of(p, offsets, dims, nbytes, max_words);
    const int wi = blockIdx.x * 256 + threadIdx.x;
    if (!g.ok || wi >= g.words) return;
    const rg_ws ws = rg_ws_of(workspace, slot, p, p0, g);
    cc_join_word((const uint32_t*)(out_bits + rg_out_plane(g.off, g.end, M, 0)), wi, g.ws, connectivity, ws.parent);
}

// components.hip's flatten pass (cc_flatten_body) on a plane of the tables: the lanes of a wave hold consecutive words, neighbouring
// lanes whose runs share a root are summed in registers first and the last lane of each group issues the five atomics.  Every lane of
// a workgroup that has a word stays in the loop until its wave has no run left, so ballots and shuffles see the whole wave.
__global__ __launch_bounds__(256) void rg_flatten_kernel(int64_t nbytes, const int64_t* __restrict__ offsets, const int* __restrict__ dims, int p0,
                                                         int64_t max_words, int M, void* workspace, int64_t slot,
                                                         const uint8_t* __restrict__ out_bits, int* __restrict__ n_regions) {
    const int p = p0 + blockIdx.y;
    const rg_plane g = rg_plane_of(p, offsets, dims, nbytes, max_words);
    if (!g.ok || (int64_t)blockIdx.x * 256 >= g.words) return;        // the same for every thread of the workgroup
    const rg_ws ws = rg_ws_of(workspace, slot, p, p0, g);
    const uint32_t* clean = (const uint32_t*)(out_bits + rg_out_plane(g.off, g.end, M, 0));
    const int wi = blockIdx.x * 256 + threadIdx.x;
    const uint32_t w = wi < g.words ? cc_unpack(clean[wi]) : 0u;
    const int wc = wi < g.words ? wi : 0;                             // past the plane's end: no run, and no index to overflow
    const int y = wc / g.ws, xw = (wc - y * g.ws) * 32, base = wc * 32;
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    int* counter = n_regions + p;
    uint32_t rest = w;
    while (__any(rest != 0u)) {
        int key = -1, me = -1, len = 0, x0 = 0, x1 = 0;
        if (rest) {
            int s, e;
            cc_next_run(w, rest, s, e);
            me = base + s;
            const int root = cc_find(ws.parent, me);
            if (root != me) { ws.parent[me >> 1] = root; key = root; }
            len = e - s; x0 = xw + s; x1 = xw + e - 1;
        }
        const bool is_root = me >= 0 && key < 0;
        const unsigned long long roots = __ballot(is_root);
        if (roots) {
            int at = 0;
            if (lane == __builtin_ctzll(roots)) at = atomicAdd(counter, __builtin_popcountll(roots));
            at = __shfl(at, __builtin_ctzll(roots), 64);
            if (is_root) ws.list[at + __builtin_popcountll(roots & below)] = me;
        }
        const int key_prev = __shfl_up(key, 1, 64);
        const unsigned long long heads = __ballot(lane == 0 || key != key_prev);
        const int first = 63 - __builtin_clzll(heads & (below | (1ull << lane)));
        int y0 = y, y1 = y;
        for (int d = 1; d < 64 && __any(lane - d >= first); d <<= 1) {
            const int o_len = __shfl_up(len, d, 64), o_x0 = __shfl_up(x0, d, 64), o_x1 = __shfl_up(x1, d, 64);
            const int o_y0 = __shfl_up(y0, d, 64), o_y1 = __shfl_up(y1, d, 64);
            if (lane - d >= first) {
                len += o_len; x0 = min(x0, o_x0); x1 = max(x1, o_x1); y0 = min(y0, o_y0); y1 = max(y1, o_y1);
            }
        }
        const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
        if (key >= 0 && last) {
            const int k = key >> 1;
            atomicAdd(ws.area + k, len);
            atomicMin(&ws.box[k].x0, x0); atomicMin(&ws.box[k].y0, y0);
            atomicMax(&ws.box[k].x1, x1); atomicMax(&ws.box[k].y1, y1);
        }
    }
}

__device__ __forceinline__ uint64_t rg_max(uint64_t a, uint64_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint64_t rg_wave_max(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
        const uint64_t other = ((uint64_t)hi << 32) | lo;
        v = other > v ? other : v;
    }
    return v;
}

// One workgroup per plane of the round.  The list of a plane has at most one root per two padded pixels, what ws.list holds.
__global__ __launch_bounds__(256) void rg_select_kernel(int64_t nbytes, const int64_t* __restrict__ offsets, const int* __restrict__ dims, int p0,
                                                        int64_t max_words, int M, int min_area, void* workspace, int64_t slot,
                                                        int* __restrict__ n_regions, int* __restrict__ regions) {
    __shared__ uint64_t red[4];
    __shared__ int win[RG_MAXM];
    const int p = p0 + blockIdx.x;
    const rg_plane g = rg_plane_of(p, offsets, dims, nbytes, max_words);
    int* rows = regions + (int64_t)p * M * 6;
    if (!g.ok) {                                                      // refused: no region, filler rows (n_regions is 0 from the init)
        if (threadIdx.x < M) rg_write_row(rows + 6 * threadIdx.x, 0, nullptr, 1, 1);
        return;
    }
    const rg_ws ws = rg_ws_of(workspace, slot, p, p0, g);
    const int n = n_regions[p];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int c[1] = {0};
    for (int i = threadIdx.x; i < n; i += 256) c[0] += rg_counts(ws.area[ws.list[i] >> 1], min_area) ? 1 : 0;
    if (mb_block_sum(c)) n_regions[p] = c[0];                         // behind its barrier every thread has read n
    uint64_t prev = ~0ull;
    for (int m = 0; m < M; ++m) {
        uint64_t best = 0;
        for (int i = threadIdx.x; i < n; i += 256) {
            const int seed = ws.list[i], a = ws.area[seed >> 1];
            const uint64_t key = cc_rank_key(a, seed);
            if (key < prev && key > best && rg_counts(a, min_area)) best = key;
        }
        best = rg_wave_max(best);
        __syncthreads();                                              // the previous round's reads of red are done
        if (lane == 0) red[wave] = best;
        __syncthreads();
        best = rg_max(rg_max(red[0], red[1]), rg_max(red[2], red[3]));
        if (threadIdx.x == 0) {
            rg_write_row(rows + 6 * m, best, ws.box, g.ws, g.w);
            win[m] = best ? cc_key_seed(best) : -1;
        }
        prev = best;                                                  // 0 once the list is exhausted: nothing is below it
    }
    __syncthreads();                                                  // every read of an area is done, win is written
    for (int i = threadIdx.x; i < n; i += 256) ws.area[ws.list[i] >> 1] = -1;
    __syncthreads();                                                  // the -1 of a winner lands before its rank
    if (threadIdx.x < M && win[threadIdx.x] >= 0) ws.area[win[threadIdx.x] >> 1] = threadIdx.x;
}

__global__ __launch_bounds__(256) void rg_route_kernel(int64_t nbytes, const int64_t* __restrict__ offsets, const int* __restrict__ dims, int p0,
                                                       int64_t max_words, int M, const void* workspace, int64_t slot, uint8_t* out_bits) {
    const int p = p0 + blockIdx.y;
    const rg_plane g = rg_plane_of(p, offsets, dims, nbytes, max_words);
    const int wi = blockIdx.x * 256 + threadIdx.x;
    if (!g.ok || wi >= g.words) return;
    const rg_ws ws = rg_ws_of(const_cast<void*>(workspace), slot, p, p0, g);
    const uint32_t w = cc_unpack(((const uint32_t*)(out_bits + rg_out_plane(g.off, g.end, M, 0)))[wi]);      // read before slot 0 is stored
    uint64_t lo = 0, hi = 0;
    const uint64_t present = w ? rg_ranks(w, wi * 32, ws.parent, ws.area, lo, hi) : 0;
    for (int m = 0; m < M; ++m) {
        const uint32_t v = (present >> m) & 1 ? rg_rank_word(w, lo, hi, m) : 0u;
        ((uint32_t*)(out_bits + rg_out_plane(g.off, g.end, M, m)))[wi] = cc_pack(v);
    }
}

// ---- cvlm_region_alpha ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rg_alpha_kernel(const uint8_t* __restrict__ bits, int64_t nbytes, const int64_t* __restrict__ offsets,
                                                       const int* __restrict__ dims, int Q, const float* __restrict__ alpha, int N, int R,
                                                       const int* __restrict__ src, float* __restrict__ out, int* __restrict__ status) {
    const int64_t RR = (int64_t)R * R;
    for (int q = blockIdx.y; q < Q; q += gridDim.y) {
        const int h = dims[2 * q], w = dims[2 * q + 1], s = src[q];
        const int64_t off = offsets[q], end = offsets[q + 1];
        const bool ok = sz_plane_ok(h, w, off, end, nbytes) && s >= 0 && s < N;      // the same for every thread of the plane
        if (!ok && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, 1);
        const uint32_t* plane = (const uint32_t*)(bits + (ok ? off : 0));
        const float* a = alpha + (ok ? s : 0) * RR;
        float* o = out + q * RR;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < RR; i += (int64_t)gridDim.x * 256) {
            const int oy = (int)(i / R), ox = (int)(i - (int64_t)oy * R);
            o[i] = ok ? a[i] * rg_gate(plane, h, w, R, oy, ox) : 0.0f;
        }
    }
}

__global__ void rg_status_kernel(int* __restrict__ status) { status[0] = 0; }

// what both region entries refuse, workspace aside
bool rg_bad(const uint8_t* bits, int64_t nbytes, const int64_t* offsets, const int32_t* dims, int32_t P, int64_t max_words, int32_t connectivity,
            int32_t M, int32_t min_area, const int32_t* n_regions, const int32_t* regions, const uint8_t* out_bits, const int32_t* status) {
    if (!bits || !offsets || !dims || !n_regions || !regions || !out_bits || !status) return true;
    if (mb_misaligned(4, bits, dims, n_regions, regions, out_bits, status) || mb_misaligned(8, offsets)) return true;
    if (P < 1 || P > 65535 || nbytes < 4 || nbytes > ((int64_t)1 << 46) || max_words < 1 || max_words > (int64_t)SZ_MAX_SIDE * (SZ_MAX_SIDE / 32))
        return true;
    if ((connectivity != 4 && connectivity != 8) || M < 1 || M > RG_MAXM || min_area < 0) return true;
    const uint64_t n4 = 4 * (uint64_t)P;
    const void* in[3] = {bits, offsets, dims};
    const uint64_t in_bytes[3] = {(uint64_t)nbytes, 8 * ((uint64_t)P + 1), 2 * n4};
    const void* out[4] = {n_regions, regions, out_bits, status};
    const uint64_t out_bytes[4] = {n4, 6 * n4 * (uint64_t)M, (uint64_t)nbytes * (uint64_t)M, 4};
    for (int o = 0; o < 4; ++o) {
        for (int i = 0; i < 3; ++i)
            if (mb_ranges_meet(out[o], out_bytes[o], in[i], in_bytes[i])) return true;
        for (int q = o + 1; q < 4; ++q)
            if (mb_ranges_meet(out[o], out_bytes[o], out[q], out_bytes[q])) return true;
    }
    return false;
}

int64_t rg_ws_all(int64_t nbytes) { return (RG_WS_PER_WORD / 4) * ((nbytes + 3) & ~(int64_t)3); }

bool rg_alpha_bad(const uint8_t* bits, int64_t nbytes, const int64_t* offsets, const int32_t* dims, int32_t Q, const float* alpha, int32_t N,
                  int32_t R, const int32_t* src, const float* out, const int32_t* status) {
    if (!bits || !offsets || !dims || !alpha || !src || !out || !status) return true;
    if (mb_misaligned(4, bits, dims, alpha, src, out, status) || mb_misaligned(8, offsets)) return true;
    return Q < 1 || Q > (1 << 24) || N < 1 || R < 1 || R > SZ_MAX_SIDE || nbytes < 4;
}

}  // namespace

extern "C" {

int64_t cvlm_mask_regions_workspace_bytes(int64_t n_bytes, int32_t P, int64_t max_words) {
    if (n_bytes < 4 || n_bytes > ((int64_t)1 << 46) || P < 1 || P > 65535 || max_words < 1 || max_words > (int64_t)SZ_MAX_SIDE * (SZ_MAX_SIDE / 32))
        return CVLM_E_BADARG;
    return std::max(rg_ws_all(n_bytes), RG_WS_PER_WORD * max_words);
}

int cvlm_mask_regions_sized(const uint8_t* bits, int64_t n_bytes, const int64_t* offsets, const int32_t* dims, int32_t P, int64_t max_words,
                            int32_t connectivity, int32_t M, int32_t min_area, void* workspace, int64_t ws_bytes, int32_t* n_regions,
                            int32_t* regions, uint8_t* out_bits, int32_t* status, void* stream) {
    if (rg_bad(bits, n_bytes, offsets, dims, P, max_words, connectivity, M, min_area, n_regions, regions, out_bits, status)) return CVLM_E_BADARG;
    const int64_t one = RG_WS_PER_WORD * max_words;
    if (mb_bad_workspace(workspace, ws_bytes, one)) return CVLM_E_BADARG;
    if (mb_ranges_meet(workspace, (uint64_t)ws_bytes, bits, (uint64_t)n_bytes) ||
        mb_ranges_meet(workspace, (uint64_t)ws_bytes, out_bits, (uint64_t)n_bytes * (uint64_t)M))
        return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    // everything in flight where the workspace holds it, the planes packed as the bits are; otherwise rounds of whole slots
    const bool all = ws_bytes >= rg_ws_all(n_bytes);
    const int64_t slot = all ? 0 : one;
    const int fit = all ? P : mb_fit(P, ws_bytes, one);
    const int gx = (int)((max_words + 255) / 256);
    const int* d = (const int*)dims;
    hipLaunchKernelGGL(rg_init_kernel, dim3((P + 255) / 256), dim3(256), 0, st, (int)P, (int*)n_regions, (int*)status);
    CVLM_CHECK_LAUNCH();
    for (int p0 = 0; p0 < P; p0 += fit) {
        const int np = std::min(fit, P - p0);
        hipLaunchKernelGGL(rg_seed_kernel, dim3(gx, np), dim3(256), 0, st, bits, n_bytes, offsets, d, p0, max_words, (int)M, workspace, slot,
                           out_bits, (int*)status);
        CVLM_CHECK_LAUNCH();
        hipLaunchKernelGGL(rg_join_kernel, dim3(gx, np), dim3(256), 0, st, n_bytes, offsets, d, p0, max_words, (int)M, (int)connectivity,
                           workspace, slot, (const uint8_t*)out_bits);
        CVLM_CHECK_LAUNCH();
        hipLaunchKernelGGL(rg_flatten_kernel, dim3(gx, np), dim3(256), 0, st, n_bytes, offsets, d, p0, max_words, (int)M, workspace, slot,
                           (const uint8_t*)out_bits, (int*)n_regions);
        CVLM_CHECK_LAUNCH();
        hipLaunchKernelGGL(rg_select_kernel, dim3(np), dim3(256), 0, st, n_bytes, offsets, d, p0, max_words, (int)M, (int)min_area, workspace,
                           slot, (int*)n_regions, (int*)regions);
        CVLM_CHECK_LAUNCH();
        hipLaunchKernelGGL(rg_route_kernel, dim3(gx, np), dim3(256), 0, st, n_bytes, offsets, d, p0, max_words, (int)M, (const void*)workspace,
                           slot, out_bits);
        CVLM_CHECK_LAUNCH();
    }
    return 0;
}

// The same passes on host memory, plane by plane and word by word, through the functions of components_logic.h and regions_logic.h.
int cvlm_debug_mask_regions_sized_host(const uint8_t* bits, int64_t n_bytes, const int64_t* offsets, const int32_t* dims, int32_t P,
                                       int64_t max_words, int32_t connectivity, int32_t M, int32_t min_area, int32_t* n_regions, int32_t* regions,
                                       uint8_t* out_bits, int32_t* status) {
    if (rg_bad(bits, n_bytes, offsets, dims, P, max_words, connectivity, M, min_area, n_regions, regions, out_bits, status)) return CVLM_E_BADARG;
    std::vector<char> mem;
    status[0] = 0;
    for (int p = 0; p < P; ++p) {
        const rg_plane g = rg_plane_of(p, offsets, dims, n_bytes, max_words);
        int32_t* rows = regions + (int64_t)p * M * 6;
        n_regions[p] = 0;
        if (!g.ok) {
            if (th_slice_ok(g.off, g.end, n_bytes)) memset(out_bits + (int64_t)M * g.off, 0, (size_t)((int64_t)M * (g.end - g.off)));
            status[0] |= 1;
            for (int m = 0; m < M; ++m) rg_write_row(rows + 6 * m, 0, nullptr, 1, 1);
            continue;
        }
        mem.resize((size_t)(RG_WS_PER_WORD * g.words) + 16);
        const rg_ws ws = rg_workspace(mem.data() + (16 - ((uintptr_t)mem.data() & 15)) % 16, g.words);
        uint32_t* clean = (uint32_t*)(out_bits + rg_out_plane(g.off, g.end, M, 0));
        const uint32_t* src = (const uint32_t*)(bits + g.off);
        for (int wi = 0; wi < g.words; ++wi) {
            clean[wi] = rg_clean_word(src[wi], wi % g.ws, g.w);
            cc_seed_word(clean, wi, g.ws, ws.parent, ws.area, ws.box);
        }
        for (int wi = 0; wi < g.words; ++wi) cc_join_word(clean, wi, g.ws, connectivity, ws.parent);
        int n = 0;
        for (int wi = 0; wi < g.words; ++wi) {
            const uint32_t w = cc_unpack(clean[wi]);
            for (uint32_t rest = w; rest;) {
                int s, e;
                cc_next_run(w, rest, s, e);
                const int me = wi * 32 + s, root = cc_find(ws.parent, me);
                if (root == me) { ws.list[n++] = me; continue; }
                ws.parent[me >> 1] = root;
                const cc_box b = ws.box[me >> 1];
                cc_box& r = ws.box[root >> 1];
                ws.area[root >> 1] += e - s;
                r.x0 = std::min(r.x0, b.x0); r.y0 = std::min(r.y0, b.y0); r.x1 = std::max(r.x1, b.x1); r.y1 = std::max(r.y1, b.y1);
            }
        }
        int c = 0;
        for (int i = 0; i < n; ++i) c += rg_counts(ws.area[ws.list[i] >> 1], min_area) ? 1 : 0;
        n_regions[p] = c;
        int win[RG_MAXM];
        uint64_t prev = ~0ull;
        for (int m = 0; m < M; ++m) {
            uint64_t best = 0;
            for (int i = 0; i < n; ++i) {
                const int seed = ws.list[i], a = ws.area[seed >> 1];
                const uint64_t key = cc_rank_key(a, seed);
                if (key < prev && key > best && rg_counts(a, min_area)) best = key;
            }
            rg_write_row(rows + 6 * m, best, ws.box, g.ws, g.w);
            win[m] = best ? cc_key_seed(best) : -1;
            prev = best;
        }
        for (int i = 0; i < n; ++i) ws.area[ws.list[i] >> 1] = -1;
        for (int m = 0; m < M; ++m)
            if (win[m] >= 0) ws.area[win[m] >> 1] = m;
        for (int wi = 0; wi < g.words; ++wi) {
            const uint32_t w = cc_unpack(clean[wi]);
            uint64_t lo = 0, hi = 0;
            const uint64_t present = w ? rg_ranks(w, wi * 32, ws.parent, ws.area, lo, hi) : 0;
            for (int m = 0; m < M; ++m) {
                const uint32_t v = (present >> m) & 1 ? rg_rank_word(w, lo, hi, m) : 0u;
                ((uint32_t*)(out_bits + rg_out_plane(g.off, g.end, M, m)))[wi] = cc_pack(v);
            }
        }
    }
    return 0;
}

int cvlm_region_alpha(const uint8_t* bits, int64_t n_bytes, const int64_t* offsets, const int32_t* dims, int32_t Q, const float* alpha, int32_t N,
                      int32_t R, const int32_t* src, float* out, int32_t* status, void* stream) {
    if (rg_alpha_bad(bits, n_bytes, offsets, dims, Q, alpha, N, R, src, out, status)) return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rg_status_kernel, dim3(1), dim3(1), 0, st, (int*)status);
    CVLM_CHECK_LAUNCH();
    const int64_t RR = (int64_t)R * R;
    const int gx = (int)std::min<int64_t>((RR + 255) / 256, 64);
    hipLaunchKernelGGL(rg_alpha_kernel, dim3(gx, std::min(Q, 65535)), dim3(256), 0, st, bits, n_bytes, offsets, (const int*)dims, (int)Q, alpha,
                       (int)N, (int)R, (const int*)src, out, (int*)status);
    CVLM_CHECK_LAUNCH();
    return 0;
}

// The same rg_gate on host memory, pixel by pixel.
int cvlm_debug_region_alpha_host(const uint8_t* bits, int64_t n_bytes, const int64_t* offsets, const int32_t* dims, int32_t Q, const float* alpha,
                                 int32_t N, int32_t R, const int32_t* src, float* out, int32_t* status) {
    if (rg_alpha_bad(bits, n_bytes, offsets, dims, Q, alpha, N, R, src, out, status)) return CVLM_E_BADARG;
    status[0] = 0;
    const int64_t RR = (int64_t)R * R;
    for (int q = 0; q < Q; ++q) {
        const int h = dims[2 * q], w = dims[2 * q + 1], s = src[q];
        const int64_t off = offsets[q], end = offsets[q + 1];
        const bool ok = sz_plane_ok(h, w, off, end, n_bytes) && s >= 0 && s < N;
        if (!ok) status[0] |= 1;
        for (int64_t i = 0; i < RR; ++i)
            out[q * RR + i] = ok ? alpha[s * RR + i] * rg_gate((const uint32_t*)(bits + off), h, w, R, (int)(i / R), (int)(i % R)) : 0.0f;
    }
    return 0;
}

}  // extern "C"
