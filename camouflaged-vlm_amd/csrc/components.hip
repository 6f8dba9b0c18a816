// Connected components of packed masks (include/cvlm.h: cvlm_mask_components): label equivalence with union-find
// (Komura 2015; Playne & Hawick 2018), seeded from the horizontal runs of 32-pixel words instead of from pixels.  The per-thread
// logic -- runs of a word, neighbour rule, find, union, kept-word filter -- is components_logic.h, shared with the sequential host
// entry at the end of this file.  One thread per word in every pass but the selection; no thread ever waits for another workgroup:
// every find / union loop lowers a label on each iteration.  All results are integer sums, minima, maxima and counts.
// Holes (cvlm_mask_holes) are the same passes on the clear pixels at the dual connectivity: the hl_ kernels below.
#include <algorithm>
#include <vector>

#include "../../include/cvlm.h"
#include "common.h"
#include "components_logic.h"

namespace {

constexpr int CC_MAXM = 64;

// Workspace of one plane: four arrays of HW / 2 entries, one entry per possible run start (components_logic.h) -- 14 bytes per pixel.
struct PlaneWs { int* parent; int* list; int* area; cc_box* box; };
__host__ __device__ inline int64_t plane_ws_bytes(int64_t HW) { return 14 * HW; }
__host__ __device__ inline PlaneWs plane_ws(void* workspace, int64_t slot, int64_t HW) {
    char* b = (char*)workspace + slot * plane_ws_bytes(HW);         // HW % 32 == 0: every array starts on a 64-byte multiple
    return PlaneWs{(int*)b, (int*)(b + 2 * HW), (int*)(b + 4 * HW), (cc_box*)(b + 6 * HW)};
}

// n_comp = 0 (it is the counter of the root lists), kept_area = 0, kept_box = -1 for all P planes
__global__ __launch_bounds__(256) void cc_init_kernel(int* __restrict__ n_comp, int* __restrict__ kept_area, int* __restrict__ kept_box, int P) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < P) n_comp[p] = 0;
    mb_init_planes(nullptr, kept_area, kept_box, P);
}

// pass 1: plane blockIdx.y of the round, one word per thread
__global__ __launch_bounds__(256) void cc_seed_kernel(const uint32_t* __restrict__ bits, int words, int wpr, void* workspace) {
    const int wi = blockIdx.x * 256 + threadIdx.x;
    if (wi >= words) return;
    const PlaneWs ws = plane_ws(workspace, blockIdx.y, (int64_t)words * 32);
    cc_seed_word(bits + (int64_t)blockIdx.y * words, wi, wpr, ws.parent, ws.area, ws.box);
}

// pass 2
__global__ __launch_bounds__(256) void cc_join_kernel(const uint32_t* __restrict__ bits, int words, int wpr, int connectivity, void* workspace) {
    const int wi = blockIdx.x * 256 + threadIdx.x;
    if (wi >= words) return;
    const PlaneWs ws = plane_ws(workspace, blockIdx.y, (int64_t)words * 32);
    cc_join_word(bits + (int64_t)blockIdx.y * words, wi, wpr, connectivity, ws.parent);
}

// pass 3: every run start is pointed at its root; a root appends itself to the plane's list (one counter add per wave and step), every
// other run adds its length and box to its root's.  The lanes of a wave hold consecutive words: neighbouring lanes whose runs share a
// root are summed in registers first (a segmented scan over equal neighbours), and the last lane of each such group issues the five
// atomics -- a region that fills the plane costs five atomics per wave and step, not per word.  Every lane stays in the loop until
// the wave has no run left, so ballots and shuffles always see the whole wave.
// FLIP = CC_SET: the set pixels (cvlm_mask_components); CC_CLEAR: the clear ones (cvlm_mask_holes), through the same scan.
template <uint32_t FLIP>
__device__ __forceinline__ void cc_flatten_body(const uint32_t* __restrict__ bits, int words, int wpr, void* workspace, int* __restrict__ n_comp) {
    const int wi = blockIdx.x * 256 + threadIdx.x;
    const PlaneWs ws = plane_ws(workspace, blockIdx.y, (int64_t)words * 32);
    const uint32_t w = wi < words ? cc_fetch(bits + (int64_t)blockIdx.y * words, wi, FLIP) : 0u;
    const int wc = wi < words ? wi : 0;                             // past the plane's end: no run, and no index to overflow
    const int y = wc / wpr, xw = (wc - y * wpr) * 32, base = wc * 32;
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    int* counter = n_comp + blockIdx.y;
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
        // groups of neighbouring lanes with one root: head = the first lane of a group, `first` = my group's head lane
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
__global__ __launch_bounds__(256) void cc_flatten_kernel(const uint32_t* __restrict__ bits, int words, int wpr, void* workspace,
                                                         int* __restrict__ n_comp) {
    cc_flatten_body<CC_SET>(bits, words, wpr, workspace, n_comp);
}

__device__ __forceinline__ uint64_t max_u64(uint64_t a, uint64_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
        const uint64_t other = ((uint64_t)hi << 32) | lo;
        v = other > v ? other : v;
    }
    return v;
}

// pass 4: one workgroup per plane.  n_kept = the regions of at least min_area pixels; then M rounds of a block-wide maximum of
// cc_rank_key over the root list, each strictly below the previous winner (the scheme of cvlm_topk_select_wide): row m of the table.
__global__ __launch_bounds__(256) void cc_select_kernel(int words, void* workspace, const int* __restrict__ n_comp, int M, int min_area,
                                                        int* __restrict__ comps, int* __restrict__ n_kept) {
    __shared__ uint64_t red[4];
    const PlaneWs ws = plane_ws(workspace, blockIdx.x, (int64_t)words * 32);
    const int n = n_comp[blockIdx.x];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (n_kept) {
        int c[1] = {0};
        for (int i = threadIdx.x; i < n; i += 256) c[0] += ws.area[ws.list[i] >> 1] >= min_area ? 1 : 0;
        if (mb_block_sum(c)) n_kept[blockIdx.x] = c[0];
    }
    uint64_t prev = ~0ull;
    for (int m = 0; m < M; ++m) {
        uint64_t best = 0;
        for (int i = threadIdx.x; i < n; i += 256) {
            const int seed = ws.list[i];
            const uint64_t key = cc_rank_key(ws.area[seed >> 1], seed);
            if (key < prev && key > best) best = key;
        }
        best = wave_max_u64(best);
        __syncthreads();                                            // the previous round's reads of red are done
        if (lane == 0) red[wave] = best;
        __syncthreads();
        best = max_u64(max_u64(red[0], red[1]), max_u64(red[2], red[3]));
        if (threadIdx.x == 0) {
            int* row = comps + ((int64_t)blockIdx.x * M + m) * 6;
            if (best) {
                const int seed = cc_key_seed(best);
                const cc_box b = ws.box[seed >> 1];
                row[0] = (int)(best >> 32); row[1] = b.x0; row[2] = b.y0; row[3] = b.x1; row[4] = b.y1; row[5] = seed;
            } else {
                row[0] = 0; row[1] = row[2] = row[3] = row[4] = row[5] = -1;
            }
        }
        prev = best;                                                // 0 once the list is exhausted: nothing is below it
    }
}

// pass 5: the plane without its regions below min_area, whole words in the stored order, and its area and box reduced per workgroup
// as cvlm_mask_pack reduces them: five atomics per workgroup that kept a pixel.
__global__ __launch_bounds__(256) void cc_keep_kernel(const uint32_t* __restrict__ bits, int words, int wpr, const void* workspace, int min_area,
                                                      uint32_t* __restrict__ kept_bits, int* __restrict__ kept_area, int* __restrict__ kept_box) {
    const int wi = blockIdx.x * 256 + threadIdx.x;
    const PlaneWs ws = plane_ws(const_cast<void*>(workspace), blockIdx.y, (int64_t)words * 32);
    mb_stats stats;
    if (wi < words) {
        const int64_t at = (int64_t)blockIdx.y * words + wi;
        const uint32_t w = cc_unpack(bits[at]);
        const uint32_t kept = w ? cc_keep_word(w, wi * 32, ws.parent, ws.area, min_area) : 0u;
        kept_bits[at] = cc_pack(kept);
        if (kept) mb_word(stats, kept, wi % wpr, wi / wpr);
    }
    mb_block_commit(stats, kept_area, kept_box, blockIdx.y);
}

// ---- holes (cvlm_mask_holes): the passes above on the CLEAR pixels, at the dual connectivity -----------------------------
// n_filled = 0, filled_area = 0 for all P planes; n_holes is written by the flatten pass's counter and then by the selection
__global__ __launch_bounds__(256) void hl_init_kernel(int* __restrict__ n_holes, int* __restrict__ n_filled, int* __restrict__ filled_area, int P) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    n_holes[p] = 0;
    if (n_filled) { n_filled[p] = 0; filled_area[p] = 0; }
}

__global__ __launch_bounds__(256) void hl_seed_kernel(const uint32_t* __restrict__ bits, int words, int wpr, void* workspace) {
    const int wi = blockIdx.x * 256 + threadIdx.x;
    if (wi >= words) return;
    const PlaneWs ws = plane_ws(workspace, blockIdx.y, (int64_t)words * 32);
    cc_seed_word(bits + (int64_t)blockIdx.y * words, wi, wpr, ws.parent, ws.area, ws.box, CC_CLEAR);
}

// background_connectivity: the dual of the caller's
__global__ __launch_bounds__(256) void hl_join_kernel(const uint32_t* __restrict__ bits, int words, int wpr, int background_connectivity,
                                                      void* workspace) {
    const int wi = blockIdx.x * 256 + threadIdx.x;
    if (wi >= words) return;
    const PlaneWs ws = plane_ws(workspace, blockIdx.y, (int64_t)words * 32);
    cc_join_word(bits + (int64_t)blockIdx.y * words, wi, wpr, background_connectivity, ws.parent, CC_CLEAR);
}

// n_regions: the counter of the list of background roots, the border's region(s) among them
__global__ __launch_bounds__(256) void hl_flatten_kernel(const uint32_t* __restrict__ bits, int words, int wpr, void* workspace,
                                                         int* __restrict__ n_regions) {
    cc_flatten_body<CC_CLEAR>(bits, words, wpr, workspace, n_regions);
}

// pass 4: one workgroup per plane.  n_holes arrives as the length of the list of background roots and leaves as the number of those
// whose box misses the border; n_filled = the holes below fill_below; then cc_select_kernel's rounds over the holes alone.
__global__ __launch_bounds__(256) void hl_select_kernel(int words, int wpr, void* workspace, int* __restrict__ n_holes, int M, int fill_below,
                                                        int* __restrict__ holes, int* __restrict__ n_filled) {
    __shared__ uint64_t red[4];
    const PlaneWs ws = plane_ws(workspace, blockIdx.x, (int64_t)words * 32);
    const int H = words / wpr, W = wpr * 32;
    const int n = n_holes[blockIdx.x];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int cf[2] = {0, 0};                                             // the holes, and those of them below fill_below
    for (int i = threadIdx.x; i < n; i += 256) {
        const int k = ws.list[i] >> 1;
        if (cc_box_inside(ws.box[k], H, W)) { ++cf[0]; cf[1] += ws.area[k] < fill_below ? 1 : 0; }
    }
    if (mb_block_sum(cf)) {                                         // behind its barrier every thread has read n
        n_holes[blockIdx.x] = cf[0];
        if (n_filled) n_filled[blockIdx.x] = cf[1];
    }
    uint64_t prev = ~0ull;
    for (int m = 0; m < M; ++m) {
        uint64_t best = 0;
        for (int i = threadIdx.x; i < n; i += 256) {
            const int seed = ws.list[i];
            const uint64_t key = cc_rank_key(ws.area[seed >> 1], seed);
            if (key < prev && key > best && cc_box_inside(ws.box[seed >> 1], H, W)) best = key;
        }
        best = wave_max_u64(best);
        __syncthreads();
        if (lane == 0) red[wave] = best;
        __syncthreads();
        best = max_u64(max_u64(red[0], red[1]), max_u64(red[2], red[3]));
        if (threadIdx.x == 0) {
            int* row = holes + ((int64_t)blockIdx.x * M + m) * 6;
            if (best) {
                const int seed = cc_key_seed(best);
                const cc_box b = ws.box[seed >> 1];
                row[0] = (int)(best >> 32); row[1] = b.x0; row[2] = b.y0; row[3] = b.x1; row[4] = b.y1; row[5] = seed;
            } else {
                row[0] = 0; row[1] = row[2] = row[3] = row[4] = row[5] = -1;
            }
        }
        prev = best;
    }
}

// pass 5: the plane with its holes below fill_below set, whole words in the stored order; its area reduced per workgroup to one atomic
__global__ __launch_bounds__(256) void hl_fill_kernel(const uint32_t* __restrict__ bits, int words, int wpr, const void* workspace, int fill_below,
                                                      uint32_t* __restrict__ filled_bits, int* __restrict__ filled_area) {
    const int wi = blockIdx.x * 256 + threadIdx.x;
    const PlaneWs ws = plane_ws(const_cast<void*>(workspace), blockIdx.y, (int64_t)words * 32);
    int cnt[1] = {0};
    if (wi < words) {
        const int64_t at = (int64_t)blockIdx.y * words + wi;
        const uint32_t set = cc_unpack(bits[at]);
        const uint32_t filled = ~set ? set | cc_fill_word(~set, wi * 32, ws.parent, ws.area, ws.box, words / wpr, wpr * 32, fill_below) : set;
        filled_bits[at] = cc_pack(filled);
        cnt[0] = __popc(filled);
    }
    if (mb_block_sum(cnt) && cnt[0]) atomicAdd(&filled_area[blockIdx.y], cnt[0]);
}

// what both hole entries refuse, workspace aside
bool hl_bad_request(const uint32_t* bits, int32_t P, int32_t H, int32_t W, int32_t connectivity, int32_t M, int32_t fill_below,
                    const int32_t* n_holes, const int32_t* holes, const int32_t* n_filled, const uint32_t* filled_bits, const int32_t* filled_area) {
    if (!bits || !n_holes || mb_misaligned(4, bits, filled_bits) || mb_bad_planes(P, H, W)) return true;
    if ((connectivity != 4 && connectivity != 8) || M < 0 || M > CC_MAXM || (M > 0) != (holes != nullptr) || fill_below < 0) return true;
    const bool fill = fill_below > 0;
    return fill != (n_filled != nullptr) || fill != (filled_bits != nullptr) || fill != (filled_area != nullptr);
}

// what both entries refuse, workspace aside
bool cc_bad_request(const uint32_t* bits, int32_t P, int32_t H, int32_t W, int32_t connectivity, int32_t M, int32_t min_area,
                    const int32_t* n_comp, const int32_t* comps, const int32_t* n_kept, const uint32_t* kept_bits, const int32_t* kept_area,
                    const int32_t* kept_box) {
    if (!bits || !n_comp || mb_misaligned(4, bits, kept_bits) || mb_bad_planes(P, H, W)) return true;
    if ((connectivity != 4 && connectivity != 8) || M < 0 || M > CC_MAXM || (M > 0) != (comps != nullptr) || min_area < 0) return true;
    const bool keep = min_area > 0;
    return keep != (n_kept != nullptr) || keep != (kept_bits != nullptr) || keep != (kept_area != nullptr) || keep != (kept_box != nullptr);
}

// Passes 1 to 3 of one plane on host memory, word by word, through the functions of components_logic.h -> the length of ws.list
int host_label_plane(const uint32_t* src, int words, int wpr, int connectivity, const PlaneWs& ws, uint32_t flip) {
    for (int wi = 0; wi < words; ++wi) cc_seed_word(src, wi, wpr, ws.parent, ws.area, ws.box, flip);
    for (int wi = 0; wi < words; ++wi) cc_join_word(src, wi, wpr, connectivity, ws.parent, flip);
    int n = 0;
    for (int wi = 0; wi < words; ++wi) {
        const uint32_t w = cc_fetch(src, wi, flip);
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
    return n;
}

}  // namespace

extern "C" {

int64_t cvlm_mask_components_workspace_bytes(int32_t P, int32_t H, int32_t W) {
    if (mb_bad_planes(P, H, W)) return -1;
    return plane_ws_bytes((int64_t)H * W) * P;
}

int cvlm_mask_components(const uint32_t* bits, int32_t P, int32_t H, int32_t W, int32_t connectivity, int32_t M, int32_t min_area,
                         void* workspace, int64_t workspace_bytes, int32_t* n_comp, int32_t* comps, int32_t* n_kept, uint32_t* kept_bits,
                         int32_t* kept_area, int32_t* kept_box, void* stream) {
    if (cc_bad_request(bits, P, H, W, connectivity, M, min_area, n_comp, comps, n_kept, kept_bits, kept_area, kept_box)) return CVLM_E_BADARG;
    const int64_t HW = (int64_t)H * W;
    if (mb_bad_workspace(workspace, workspace_bytes, plane_ws_bytes(HW))) return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int words = (int)(HW / 32), wpr = W / 32;
    const int gx = (words + 255) / 256;
    const int fit = mb_fit(P, workspace_bytes, plane_ws_bytes(HW));
    hipLaunchKernelGGL(cc_init_kernel, dim3((P + 255) / 256), dim3(256), 0, st, (int*)n_comp, (int*)kept_area, (int*)kept_box, (int)P);
    CVLM_CHECK_LAUNCH();
    for (int p0 = 0; p0 < P; p0 += fit) {
        const int np = std::min(fit, P - p0);
        const uint32_t* src = bits + (int64_t)p0 * words;
        hipLaunchKernelGGL(cc_seed_kernel, dim3(gx, np), dim3(256), 0, st, src, words, wpr, workspace);
        CVLM_CHECK_LAUNCH();
        hipLaunchKernelGGL(cc_join_kernel, dim3(gx, np), dim3(256), 0, st, src, words, wpr, (int)connectivity, workspace);
        CVLM_CHECK_LAUNCH();
        hipLaunchKernelGGL(cc_flatten_kernel, dim3(gx, np), dim3(256), 0, st, src, words, wpr, workspace, (int*)n_comp + p0);
        CVLM_CHECK_LAUNCH();
        if (M > 0 || min_area > 0) {
            hipLaunchKernelGGL(cc_select_kernel, dim3(np), dim3(256), 0, st, words, workspace, (const int*)n_comp + p0, (int)M, (int)min_area,
                               comps ? (int*)comps + (int64_t)p0 * M * 6 : (int*)nullptr, n_kept ? (int*)n_kept + p0 : (int*)nullptr);
            CVLM_CHECK_LAUNCH();
        }
        if (min_area > 0) {
            hipLaunchKernelGGL(cc_keep_kernel, dim3(gx, np), dim3(256), 0, st, src, words, wpr, (const void*)workspace, (int)min_area,
                               kept_bits + (int64_t)p0 * words, (int*)kept_area + p0, (int*)kept_box + 4 * (int64_t)p0);
            CVLM_CHECK_LAUNCH();
        }
    }
    return 0;
}

// The same passes on host memory, plane by plane and word by word, through the functions of components_logic.h.
int cvlm_debug_mask_components_host(const uint32_t* bits, int32_t P, int32_t H, int32_t W, int32_t connectivity, int32_t M, int32_t min_area,
                                    int32_t* n_comp, int32_t* comps, int32_t* n_kept, uint32_t* kept_bits, int32_t* kept_area,
                                    int32_t* kept_box) {
    if (cc_bad_request(bits, P, H, W, connectivity, M, min_area, n_comp, comps, n_kept, kept_bits, kept_area, kept_box)) return CVLM_E_BADARG;
    const int64_t HW = (int64_t)H * W;
    const int words = (int)(HW / 32), wpr = W / 32;
    std::vector<char> mem((size_t)plane_ws_bytes(HW));
    const PlaneWs ws = plane_ws(mem.data(), 0, HW);
    for (int p = 0; p < P; ++p) {
        const uint32_t* src = bits + (int64_t)p * words;
        const int n = host_label_plane(src, words, wpr, connectivity, ws, CC_SET);
        n_comp[p] = n;
        if (n_kept) {
            int c = 0;
            for (int i = 0; i < n; ++i) c += ws.area[ws.list[i] >> 1] >= min_area ? 1 : 0;
            n_kept[p] = c;
        }
        uint64_t prev = ~0ull;
        for (int m = 0; m < M; ++m) {
            uint64_t best = 0;
            for (int i = 0; i < n; ++i) {
                const uint64_t key = cc_rank_key(ws.area[ws.list[i] >> 1], ws.list[i]);
                if (key < prev && key > best) best = key;
            }
            int* row = comps + ((int64_t)p * M + m) * 6;
            if (best) {
                const int seed = cc_key_seed(best);
                const cc_box b = ws.box[seed >> 1];
                row[0] = (int)(best >> 32); row[1] = b.x0; row[2] = b.y0; row[3] = b.x1; row[4] = b.y1; row[5] = seed;
            } else {
                row[0] = 0; row[1] = row[2] = row[3] = row[4] = row[5] = -1;
            }
            prev = best;
        }
        if (min_area > 0) {
            mb_stats stats;
            for (int wi = 0; wi < words; ++wi) {
                const uint32_t w = cc_unpack(src[wi]);
                const uint32_t kept = w ? cc_keep_word(w, wi * 32, ws.parent, ws.area, min_area) : 0u;
                kept_bits[(int64_t)p * words + wi] = cc_pack(kept);
                if (kept) mb_word(stats, kept, wi % wpr, wi / wpr);
            }
            mb_init(kept_area, kept_box, p);
            mb_store(stats, kept_area, kept_box, p);
        }
    }
    return 0;
}

int64_t cvlm_mask_holes_workspace_bytes(int32_t P, int32_t H, int32_t W) { return cvlm_mask_components_workspace_bytes(P, H, W); }

int cvlm_mask_holes(const uint32_t* bits, int32_t P, int32_t H, int32_t W, int32_t connectivity, int32_t M, int32_t fill_below,
                    void* workspace, int64_t workspace_bytes, int32_t* n_holes, int32_t* holes, int32_t* n_filled,
                    uint32_t* filled_bits, int32_t* filled_area, void* stream) {
    if (hl_bad_request(bits, P, H, W, connectivity, M, fill_below, n_holes, holes, n_filled, filled_bits, filled_area)) return CVLM_E_BADARG;
    const int64_t HW = (int64_t)H * W;
    if (mb_bad_workspace(workspace, workspace_bytes, plane_ws_bytes(HW))) return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int words = (int)(HW / 32), wpr = W / 32;
    const int gx = (words + 255) / 256;
    const int fit = mb_fit(P, workspace_bytes, plane_ws_bytes(HW));
    hipLaunchKernelGGL(hl_init_kernel, dim3((P + 255) / 256), dim3(256), 0, st, (int*)n_holes, (int*)n_filled, (int*)filled_area, (int)P);
    CVLM_CHECK_LAUNCH();
    for (int p0 = 0; p0 < P; p0 += fit) {
        const int np = std::min(fit, P - p0);
        const uint32_t* src = bits + (int64_t)p0 * words;
        hipLaunchKernelGGL(hl_seed_kernel, dim3(gx, np), dim3(256), 0, st, src, words, wpr, workspace);
        CVLM_CHECK_LAUNCH();
        hipLaunchKernelGGL(hl_join_kernel, dim3(gx, np), dim3(256), 0, st, src, words, wpr, cc_dual(connectivity), workspace);
        CVLM_CHECK_LAUNCH();
        hipLaunchKernelGGL(hl_flatten_kernel, dim3(gx, np), dim3(256), 0, st, src, words, wpr, workspace, (int*)n_holes + p0);
        CVLM_CHECK_LAUNCH();
        hipLaunchKernelGGL(hl_select_kernel, dim3(np), dim3(256), 0, st, words, wpr, workspace, (int*)n_holes + p0, (int)M, (int)fill_below,
                           holes ? (int*)holes + (int64_t)p0 * M * 6 : (int*)nullptr, n_filled ? (int*)n_filled + p0 : (int*)nullptr);
        CVLM_CHECK_LAUNCH();
        if (fill_below > 0) {
            hipLaunchKernelGGL(hl_fill_kernel, dim3(gx, np), dim3(256), 0, st, src, words, wpr, (const void*)workspace, (int)fill_below,
                               filled_bits + (int64_t)p0 * words, (int*)filled_area + p0);
            CVLM_CHECK_LAUNCH();
        }
    }
    return 0;
}

// The same passes on host memory, as cvlm_debug_mask_components_host runs them.
int cvlm_debug_mask_holes_host(const uint32_t* bits, int32_t P, int32_t H, int32_t W, int32_t connectivity, int32_t M, int32_t fill_below,
                               int32_t* n_holes, int32_t* holes, int32_t* n_filled, uint32_t* filled_bits, int32_t* filled_area) {
    if (hl_bad_request(bits, P, H, W, connectivity, M, fill_below, n_holes, holes, n_filled, filled_bits, filled_area)) return CVLM_E_BADARG;
    const int64_t HW = (int64_t)H * W;
    const int words = (int)(HW / 32), wpr = W / 32;
    std::vector<char> mem((size_t)plane_ws_bytes(HW));
    const PlaneWs ws = plane_ws(mem.data(), 0, HW);
    for (int p = 0; p < P; ++p) {
        const uint32_t* src = bits + (int64_t)p * words;
        const int n = host_label_plane(src, words, wpr, cc_dual(connectivity), ws, CC_CLEAR);
        int c = 0, f = 0;
        for (int i = 0; i < n; ++i) {
            const int k = ws.list[i] >> 1;
            if (cc_box_inside(ws.box[k], H, W)) { ++c; f += ws.area[k] < fill_below ? 1 : 0; }
        }
        n_holes[p] = c;
        if (n_filled) n_filled[p] = f;
        uint64_t prev = ~0ull;
        for (int m = 0; m < M; ++m) {
            uint64_t best = 0;
            for (int i = 0; i < n; ++i) {
                const int seed = ws.list[i];
                const uint64_t key = cc_rank_key(ws.area[seed >> 1], seed);
                if (key < prev && key > best && cc_box_inside(ws.box[seed >> 1], H, W)) best = key;
            }
            int* row = holes + ((int64_t)p * M + m) * 6;
            if (best) {
                const int seed = cc_key_seed(best);
                const cc_box b = ws.box[seed >> 1];
                row[0] = (int)(best >> 32); row[1] = b.x0; row[2] = b.y0; row[3] = b.x1; row[4] = b.y1; row[5] = seed;
            } else {
                row[0] = 0; row[1] = row[2] = row[3] = row[4] = row[5] = -1;
            }
            prev = best;
        }
        if (fill_below > 0) {
            int a = 0;
            for (int wi = 0; wi < words; ++wi) {
                const uint32_t set = cc_unpack(src[wi]);
                const uint32_t filled = ~set ? set | cc_fill_word(~set, wi * 32, ws.parent, ws.area, ws.box, H, W, fill_below) : set;
                filled_bits[(int64_t)p * words + wi] = cc_pack(filled);
                a += __builtin_popcount(filled);
            }
            filled_area[p] = a;
        }
    }
    return 0;
}

}  // extern "C"
