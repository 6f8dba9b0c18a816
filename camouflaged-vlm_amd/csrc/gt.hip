// COCO annotations on the device (include/cvlm.h: cvlm_mask_rle_decode, cvlm_mask_inter_sized): run counts -> sized
// planes, the inverse of rle.hip at the sizes of sized.hip, and the intersections of pairs of sized planes.  The per-thread logic --
// the checks of a plane and of a pair, the stream bit of a boundary, the prefix XOR of a stream word, the fetch of 32 rows of a pixel
// column, the masked word of an intersection -- is gt_logic.h, shared with the sequential host entries at the end of this file.
// Decoding is three launches per round of planes behind a memset: toggle the boundaries into the stream (one workgroup per plane),
// prefix-XOR the stream (one workgroup per plane), transpose it into the rows.  All results are integers; no thread waits for another
// workgroup.
// COCO polygons (cvlm_mask_poly_decode) feed the same stream: the front walks a polygon's edges with the published
// rleFrPoly's arithmetic (poly_logic.h) and toggles the boundary positions it finds; the prefix pass and the transposition are the
// decoder's own, and a plane's further polygons are ORed in by one more launch.
#include <algorithm>
#include <vector>

#include "../../include/cvlm.h"
#include "common.h"
#include "gt_logic.h"
#include "poly_logic.h"

namespace {

constexpr int GD_SCAN = 1024;                                         // threads of the one workgroup per plane of the two stream passes
// The tile of one workgroup of the transpose: GD_TW word columns x GD_TH rows.  Per block of 32 rows the 32 GD_TW fetched words of the
// tile's pixel columns lie in LDS, 33 apart per word column: the 16 word columns a wave gathers at once then start in 16 banks.
constexpr int GD_TW = 16, GD_TH = 128, GD_LD = GD_TW * 33;
constexpr int GI_SPAN = 2048;                                         // words of a pair per workgroup and step of the intersection

// status = 0; area = 0, box = -1
__global__ __launch_bounds__(256) void gd_init_kernel(int* __restrict__ area, int* __restrict__ box, int P, int* __restrict__ status) {
    mb_init_planes(status, area, box, P);
}

// One workgroup per plane of the round, slot blockIdx.x of the zeroed workspace.  Every check of the plane, then its counts in slabs
// of GD_SCAN with a carried 64-bit prefix sum: boundary k <= n - 2 toggles stream bit e_k where 0 <= e_k < h w, by an integer XOR that
// commutes and cancels equal positions.  The walk ends at the first slab that holds a negative count or carries the sum beyond h w:
// the carry stays below 2^42.  The verdict (slot word 0 = 1: the plane is whole) is the last thing written; a refused plane ORs 1
// into status and leaves the verdict 0.
__global__ __launch_bounds__(GD_SCAN) void gd_toggle_kernel(const int32_t* __restrict__ counts, int64_t total,
                                                            const int64_t* __restrict__ run_offsets, const int* __restrict__ dims,
                                                            const int64_t* __restrict__ bit_offsets, int64_t nbytes, int64_t max_pixels,
                                                            int p0, uint32_t* __restrict__ ws, int64_t ws_stride, int* __restrict__ status) {
    __shared__ long long s_sum[2][GD_SCAN / 64];
    __shared__ int s_neg[2][GD_SCAN / 64];
    const int p = p0 + blockIdx.x;
    uint32_t* slot = ws + (int64_t)blockIdx.x * ws_stride;
    const int h = dims[2 * p], w = dims[2 * p + 1];
    const int64_t off = run_offsets[p], end = run_offsets[p + 1];
    if (!gd_shape_ok(h, w, max_pixels) || !sz_plane_ok(h, w, bit_offsets[p], bit_offsets[p + 1], nbytes) || !gd_slice_ok(off, end, total)) {
        if (threadIdx.x == 0) atomicOr(status, 1);                    // the same for every thread: no count is read, nothing is toggled
        return;
    }
    const int hw = h * w;                                             // <= 2^28
    const int64_t n = end - off;
    uint32_t* stream = slot + GT_WS_HEAD;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long carry = 0;
    int neg = 0;
    for (int64_t k0 = 0, slab = 0; k0 < n; k0 += GD_SCAN, slab ^= 1) {
        const int64_t k = k0 + threadIdx.x;
        const int c = k < n ? counts[off + k] : 0;
        long long sum = c;                                            // inclusive over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long a = __shfl_up(sum, o, 64);
            if (lane >= o) sum += a;
        }
        const int wave_neg = __ballot(c < 0) != 0ull;
        if (lane == 63) { s_sum[slab][wave] = sum; s_neg[slab][wave] = wave_neg; }
        __syncthreads();
        long long before = carry, all = carry;
#pragma unroll
        for (int v = 0; v < GD_SCAN / 64; ++v) {
            const long long a = s_sum[slab][v];
            if (v < wave) before += a;
            all += a;
            neg |= s_neg[slab][v];
        }
        int word;
        uint32_t bit;
        if (k < n - 1 && !neg && gd_toggle(before + sum, hw, word, bit)) atomicXor(&stream[word], bit);
        carry = all;
        if (neg || carry > hw) break;                                 // the same for every thread
    }
    if (threadIdx.x == 0) {
        if (!neg && carry == hw) slot[0] = 1u;
        else atomicOr(status, 1);
    }
}

// One workgroup per plane of the round: the inclusive prefix XOR of the stream, in place.  Inside a word by shifts (gd_prefix_word),
// across the words by the parity of their popcounts: one ballot per wave, the waves' parities through LDS, double-buffered by the
// slab's parity (one barrier per slab), a carry between slabs.  A refused plane (verdict 0) is left alone.
__global__ __launch_bounds__(GD_SCAN) void gd_prefix_kernel(const int* __restrict__ dims, int p0, uint32_t* __restrict__ ws,
                                                            int64_t ws_stride) {
    __shared__ uint32_t s_par[2][GD_SCAN / 64];
    uint32_t* slot = ws + (int64_t)blockIdx.x * ws_stride;
    if (slot[0] == 0u) return;                                        // the whole workgroup; verdict 1: the size passed gd_shape_ok
    const int p = p0 + blockIdx.x;
    const int words = (int)gd_stream_words((int64_t)dims[2 * p] * dims[2 * p + 1]);
    uint32_t* stream = slot + GT_WS_HEAD;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0u;
    for (int k0 = 0, slab = 0; k0 < words; k0 += GD_SCAN, slab ^= 1) {
        const int k = k0 + threadIdx.x;
        const uint32_t w = k < words ? stream[k] : 0u;
        const unsigned long long odd = __ballot(__popc(w) & 1);
        const uint32_t below = (uint32_t)__popcll(odd & ((1ull << lane) - 1ull)) & 1u;
        if (lane == 0) s_par[slab][wave] = (uint32_t)__popcll(odd) & 1u;
        __syncthreads();
        uint32_t before = carry, all = carry;
#pragma unroll
        for (int v = 0; v < GD_SCAN / 64; ++v) {
            const uint32_t a = s_par[slab][v];
            if (v < wave) before ^= a;
            all ^= a;
        }
        if (k < words) stream[k] = gd_prefix_word(w, before ^ below);
        carry = all;
    }
}

// Plane blockIdx.y of the round; workgroup g takes the tiles g, g + gridDim.x, ... of its plane (the grid is sized by the largest plane
// the workspace admits).  A tile stages, per pixel column and block of 32 rows, the 32 stream bits from x h + y on (gd_fetch: two
// stream words), then every thread gathers whole words of rows -- 16 consecutive word columns of a row per 16 lanes -- and stores them;
// the columns at or beyond w stay clear.  The table check comes before any store; a plane the toggle pass refused gets zero words.
template <bool STATS>
__global__ __launch_bounds__(256) void gd_transpose_kernel(const int* __restrict__ dims, const int64_t* __restrict__ bit_offsets,
                                                           uint8_t* __restrict__ bits, int64_t nbytes, int p0,
                                                           const uint32_t* __restrict__ ws, int64_t ws_stride, int* __restrict__ area,
                                                           int* __restrict__ box) {
    __shared__ uint32_t s_v[GD_TH / 32 * GD_LD];
    const int p = p0 + blockIdx.y;
    const int h = dims[2 * p], w = dims[2 * p + 1];
    const int64_t off = bit_offsets[p];
    if (!sz_plane_ok(h, w, off, bit_offsets[p + 1], nbytes)) return;  // the same for every thread; the toggle pass has set status
    const uint32_t* slot = ws + (int64_t)blockIdx.y * ws_stride;
    const bool good = slot[0] != 0u;
    const uint32_t* stream = slot + GT_WS_HEAD;
    const int wsr = sz_words_per_row(w), col_tiles = (wsr + GD_TW - 1) / GD_TW, row_tiles = (h + GD_TH - 1) / GD_TH;
    const int tiles = col_tiles * row_tiles;                          // <= 32 * 128
    const int64_t swords = gd_stream_words((int64_t)h * w);           // read only where good: then h w <= max_pixels
    uint32_t* dst = (uint32_t*)(bits + off);
    mb_stats stats;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int tr = t / col_tiles, tc = t - tr * col_tiles;
        const int c0 = tc * GD_TW, y0 = tr * GD_TH;
        const int rows = min(GD_TH, h - y0);                          // >= 1
        if (good) {
#pragma unroll 1
            for (int i = 0; i < GD_TH / 32 * GD_TW * 32 / 256; ++i) {
                const int o = i * 256 + threadIdx.x;
                const int xl = o & (GD_TW * 32 - 1), rb = o / (GD_TW * 32);
                const int x = 32 * c0 + xl;
                if (x < w && 32 * rb < rows) s_v[rb * GD_LD + xl + (xl >> 5)] = gd_fetch(stream, swords, x * h + y0 + 32 * rb);
            }
            __syncthreads();
        }
#pragma unroll 1
        for (int i = 0; i < GD_TH * GD_TW / 256; ++i) {
            const int o = i * 256 + threadIdx.x;
            const int cl = o & (GD_TW - 1), r = o / GD_TW, c = c0 + cl;
            if (c >= wsr || r >= rows) continue;
            const uint32_t m = good ? gd_row_word(s_v + (r >> 5) * GD_LD + cl * 33, 1, c, w, r & 31) : 0u;
            dst[sz_word_of(y0 + r, 32 * c, wsr)] = cc_pack(m);
            if (STATS && m) mb_word(stats, m, c, y0 + r);
        }
        if (good) __syncthreads();                                    // the next tile stages into the same words
    }
    if (STATS) mb_block_commit(stats, area, box, p);
}

// The transposition on the host: the stream of a plane of h x w (NULL: a refused plane, zero words) -> its rows at dst, area and box
// where they are asked for (initialised by the caller; an empty plane leaves them alone)
void gd_rows_host(const uint32_t* stream, int64_t swords, int h, int w, uint32_t* dst, int32_t* area, int32_t* box) {
    const int wsr = sz_words_per_row(w);
    mb_stats stats;
    uint32_t v[32];
    for (int c = 0; c < wsr; ++c)
        for (int y0 = 0; y0 < h; y0 += 32) {
            if (stream)
                for (int i = 0; i < std::min(32, w - 32 * c); ++i) v[i] = gd_fetch(stream, swords, (32 * c + i) * h + y0);
            for (int r = 0; r < std::min(32, h - y0); ++r) {
                const uint32_t m = stream ? gd_row_word(v, 1, c, w, r) : 0u;
                dst[sz_word_of(y0 + r, 32 * c, wsr)] = cc_pack(m);
                if (m) mb_word(stats, m, c, y0 + r);
            }
        }
    if (area) mb_store(stats, area, box, 0);
}

// The prefix pass on the host: the inclusive prefix XOR of the stream `cur` of `words` words, stored to `out` or (or_in) ORed into it.
// out may be cur itself.
void gd_prefix_host(const uint32_t* cur, int64_t words, uint32_t* out, bool or_in) {
    uint32_t before = 0u;
    for (int64_t k = 0; k < words; ++k) {
        const uint32_t c = cur[k], m = gd_prefix_word(c, before);
        out[k] = or_in ? out[k] | m : m;
        before ^= (uint32_t)__builtin_popcount(c) & 1u;
    }
}

// The last launch of a round of n planes of either decoder, behind gd_prefix_kernel (and the polygons' layers): the streams in the
// round's slots -> the rows of the planes p0 .. p0 + n - 1, with area and box where the call asks for them.
int gd_rows_round(const int32_t* dims, const int64_t* bit_offsets, uint8_t* bits, int64_t bits_bytes, int p0, int n, int64_t max_pixels,
                  const uint32_t* ws, int64_t ws_stride, int32_t* area, int32_t* box, hipStream_t st) {
    // workgroups per plane: one per 16384 pixels of the largest plane the slot admits, about 8192 in all and at most 256; they walk
    // their plane's tiles in strides
    const int64_t by_work = (max_pixels + 16383) / 16384, want = (8192 + n - 1) / n;
    const int gx = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(by_work, want), 256));
    if (area)
        hipLaunchKernelGGL(gd_transpose_kernel<true>, dim3(gx, n), dim3(256), 0, st, (const int*)dims, bit_offsets, bits, bits_bytes, p0, ws,
                           ws_stride, (int*)area, (int*)box);
    else
        hipLaunchKernelGGL(gd_transpose_kernel<false>, dim3(gx, n), dim3(256), 0, st, (const int*)dims, bit_offsets, bits, bits_bytes, p0, ws,
                           ws_stride, (int*)nullptr, (int*)nullptr);
    CVLM_CHECK_LAUNCH();
    return 0;
}

// what both decode entries refuse
bool gd_bad(const int32_t* counts, int64_t total, const int64_t* run_offsets, const int32_t* dims, const int64_t* bit_offsets, int32_t P,
            int64_t max_pixels, const uint8_t* bits, int64_t nbytes, const int32_t* area, const int32_t* box, const int32_t* status) {
    if (!counts || !run_offsets || !dims || !bit_offsets || !bits || !status || (area == nullptr) != (box == nullptr)) return true;
    if (mb_misaligned(4, counts, dims, bits, area, box, status) || mb_misaligned(8, run_offsets, bit_offsets)) return true;
    return P < 1 || P > 65535 || total < 1 || nbytes < 4 || max_pixels < 1 || max_pixels > GT_MAX_PIXELS;
}

// ---- polygons ----------------------------------------------------------------------------------------------------------------
// One polygon, xy[off, end), by the whole workgroup of GD_SCAN threads: every check first -- the slice, every coordinate, and the walk
// points of all edges summed in 64 bits (at most 65535 edges of fewer than 2^20 points each) --, and only then the walk, in slabs of
// GD_SCAN edges whose scaled vertices are staged in LDS: a wave per edge, round-robin, the lanes striding over the edge's points.
// Each lane forms its point and the point before it -- for d = 0 the last point of the previous edge; the very first point of the
// sequence has none -- and toggles the pair's boundary position, if it has one, by an integer XOR that commutes and cancels equal
// positions.  -> false, the same for every thread: the polygon is refused and nothing was toggled.  s_sum / s_bad: GD_SCAN / 64
// words of LDS each, s_x / s_y: GD_SCAN + 2 each, all free again on return.  s_span, where given: two words of LDS the caller has set
// to (INT_MAX, -1); behind the caller's next barrier they hold the first and the last stream word the polygon toggled.
__device__ bool gp_polygon(const double* __restrict__ xy, int64_t total, int64_t off, int64_t end, int h, int w, uint32_t* stream,
                           long long* s_sum, int* s_bad, int* s_x, int* s_y, int* s_span) {
    if (!pl_slice_ok(off, end, total)) return false;
    const int k = (int)((end - off) >> 1);
    const double* v = xy + off;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long pts = 0;
    int bad = 0;
    for (int j = threadIdx.x; j < k; j += GD_SCAN) {
        const int jn = j + 1 < k ? j + 1 : 0;
        const double x0 = v[2 * j], y0 = v[2 * j + 1], x1 = v[2 * jn], y1 = v[2 * jn + 1];
        if (!pl_coord_ok(x0) || !pl_coord_ok(y0) || !pl_coord_ok(x1) || !pl_coord_ok(y1)) bad = 1;      // nothing of it becomes an int
        else pts += pl_edge_of(pl_scale(x0), pl_scale(y0), pl_scale(x1), pl_scale(y1)).n;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pts += __shfl_xor(pts, o, 64);
    const int wave_bad = __ballot(bad) != 0ull;
    if (lane == 0) { s_sum[wave] = pts; s_bad[wave] = wave_bad; }
    __syncthreads();
    pts = 0;
    bad = 0;
#pragma unroll
    for (int i = 0; i < GD_SCAN / 64; ++i) { pts += s_sum[i]; bad |= s_bad[i]; }
    __syncthreads();                                                  // the LDS words may be written again
    if (bad || pts > PL_MAX_POINTS) return false;
    const int hw = h * w;
    int lo = 0x7fffffff, hi = -1;                                     // the stream words this thread toggles
    for (int j0 = 0; j0 < k; j0 += GD_SCAN) {                         // slabs of GD_SCAN edges, their scaled vertices staged in LDS
        for (int i = threadIdx.x; i < GD_SCAN + 2; i += GD_SCAN) {    // slot i: vertex j0 - 1 + i; vertex k is vertex 0 again
            const int j = j0 - 1 + i;
            if (j >= 0 && j <= k) {
                const int jj = j < k ? j : 0;
                s_x[i] = pl_scale(v[2 * jj]);
                s_y[i] = pl_scale(v[2 * jj + 1]);
            }
        }
        __syncthreads();
        const int m = min(GD_SCAN, k - j0);
        for (int i = wave; i < m; i += GD_SCAN / 64) {
            const pl_edge e = pl_edge_of(s_x[i + 1], s_y[i + 1], s_x[i + 2], s_y[i + 2]);
            int lu = 0, lv = 0;                                       // the last point of the edge before this one
            if (j0 + i > 0) {
                const pl_edge b = pl_edge_of(s_x[i], s_y[i], s_x[i + 1], s_y[i + 1]);
                pl_point(b, b.n - 1, lu, lv);
            }
            for (int d = lane; d < e.n; d += 64) {
                int u, t, up = lu, tp = lv;
                pl_point(e, d, u, t);
                if (d > 0) pl_point(e, d - 1, up, tp);
                else if (j0 + i == 0) continue;
                int64_t pos;
                int word;
                uint32_t bit;
                if (pl_candidate(up, tp, u, t, h, w, pos) && gd_toggle(pos, hw, word, bit)) {
                    atomicXor(&stream[word], bit);
                    lo = min(lo, word);
                    hi = max(hi, word);
                }
            }
        }
        __syncthreads();                                              // the next slab stages into the same words
    }
    if (s_span) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o, 64)); hi = max(hi, __shfl_xor(hi, o, 64)); }
        if (lane == 0 && hi >= 0) { atomicMin(&s_span[0], lo); atomicMax(&s_span[1], hi); }
    }
    return true;
}

// One workgroup per plane of the round, slot blockIdx.x of the zeroed accumulator streams: every check of the plane and of its list
// of polygons, then its FIRST polygon into the stream.  layered: cvlm_mask_poly_decode runs gp_layers_kernel behind this one (Q > P);
// without it a plane of several polygons is refused -- the call then holds a plane of none as well.  The verdict (slot word 0 = 1: whole
// so far) is the last thing written; a refused plane ORs 1 into status and leaves the verdict 0.
__global__ __launch_bounds__(GD_SCAN) void gp_toggle_kernel(const double* __restrict__ xy, int64_t total, const int64_t* __restrict__ poly_offsets,
                                                            const int* __restrict__ plane_polys, int Q, const int* __restrict__ dims,
                                                            const int64_t* __restrict__ bit_offsets, int64_t nbytes, int64_t max_pixels,
                                                            int layered, int p0, uint32_t* __restrict__ ws, int64_t ws_stride,
                                                            int* __restrict__ status) {
    __shared__ long long s_sum[GD_SCAN / 64];
    __shared__ int s_bad[GD_SCAN / 64], s_x[GD_SCAN + 2], s_y[GD_SCAN + 2];
    const int p = p0 + blockIdx.x;
    uint32_t* slot = ws + (int64_t)blockIdx.x * ws_stride;
    const int h = dims[2 * p], w = dims[2 * p + 1];
    const int q0 = plane_polys[p], q1 = plane_polys[p + 1];
    bool good = gd_shape_ok(h, w, max_pixels) && sz_plane_ok(h, w, bit_offsets[p], bit_offsets[p + 1], nbytes) && pl_polys_ok(q0, q1, Q) &&
                (layered || q1 - q0 == 1);
    good = good && gp_polygon(xy, total, poly_offsets[q0], poly_offsets[q0 + 1], h, w, slot + GT_WS_HEAD, s_sum, s_bad, s_x, s_y, nullptr);
    if (threadIdx.x == 0) {                                           // good is the same for every thread
        if (good) slot[0] = 1u;
        else atomicOr(status, 1);
    }
}

// One workgroup per plane of the round, behind gp_toggle_kernel and gd_prefix_kernel: the plane's polygons 1, 2, ... one after the other.
// Each is toggled into the plane's second stream `cur` (zero on entry), whose prefix XOR -- gd_prefix_kernel's pass -- is ORed into the
// accumulator word by word while cur is cleared again: acc |= cur, cur = 0, the union.  cur is toggled by atomics, which the L2 runs;
// so it is read back by loads of device scope, behind a device-wide fence and the barrier.  The pass starts at the slab of the first
// word the polygon toggled and ends behind the last one as soon as the parity carried on is even: every word outside is zero in cur
// and stays zero under the prefix XOR.  A refused polygon refuses the plane: the verdict goes back to 0 and status gets its 1.  A
// plane of one polygon, or one already refused, leaves at once.
__global__ __launch_bounds__(GD_SCAN) void gp_layers_kernel(const double* __restrict__ xy, int64_t total, const int64_t* __restrict__ poly_offsets,
                                                            const int* __restrict__ plane_polys, const int* __restrict__ dims, int p0,
                                                            uint32_t* __restrict__ ws, uint32_t* __restrict__ cur_ws, int64_t ws_stride,
                                                            int* __restrict__ status) {
    __shared__ long long s_sum[GD_SCAN / 64];
    __shared__ int s_bad[GD_SCAN / 64], s_x[GD_SCAN + 2], s_y[GD_SCAN + 2], s_span[2];
    __shared__ uint32_t s_par[2][GD_SCAN / 64];
    uint32_t* slot = ws + (int64_t)blockIdx.x * ws_stride;
    if (slot[0] == 0u) return;                                        // the whole workgroup; verdict 1: size and list passed their checks
    const int p = p0 + blockIdx.x;
    const int q0 = plane_polys[p], q1 = plane_polys[p + 1];
    if (q1 - q0 < 2) return;
    const int h = dims[2 * p], w = dims[2 * p + 1];
    const int words = (int)gd_stream_words((int64_t)h * w);
    uint32_t* acc = slot + GT_WS_HEAD;
    uint32_t* cur = cur_ws + (int64_t)blockIdx.x * ws_stride + GT_WS_HEAD;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int q = q0 + 1; q < q1; ++q) {
        if (threadIdx.x == 0) { s_span[0] = 0x7fffffff; s_span[1] = -1; }      // gp_polygon's barriers lie between this and its walk
        if (!gp_polygon(xy, total, poly_offsets[q], poly_offsets[q + 1], h, w, cur, s_sum, s_bad, s_x, s_y, s_span)) {
            if (threadIdx.x == 0) { slot[0] = 0u; atomicOr(status, 1); }
            return;                                                   // the same for every thread
        }
        __threadfence();
        __syncthreads();                                              // every toggle of the polygon has reached the L2
        const int first = s_span[0], last = s_span[1];                // last < 0: the polygon toggled nothing
        uint32_t carry = 0u;
        for (int k0 = last < 0 ? words : first / GD_SCAN * GD_SCAN, slab = 0; k0 < words; k0 += GD_SCAN, slab ^= 1) {
            const int k = k0 + threadIdx.x;
            const uint32_t c = k < words ? __hip_atomic_load(&cur[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
            const unsigned long long odd = __ballot(__popc(c) & 1);
            const uint32_t below = (uint32_t)__popcll(odd & ((1ull << lane) - 1ull)) & 1u;
            if (lane == 0) s_par[slab][wave] = (uint32_t)__popcll(odd) & 1u;
            __syncthreads();
            uint32_t before = carry, all = carry;
#pragma unroll
            for (int i = 0; i < GD_SCAN / 64; ++i) {
                const uint32_t a = s_par[slab][i];
                if (i < wave) before ^= a;
                all ^= a;
            }
            if (k < words) {
                const uint32_t m = gd_prefix_word(c, before ^ below);
                if (m) acc[k] |= m;                                   // word k is this thread's in every layer
                if (c) cur[k] = 0u;
            }
            carry = all;
            if (k0 + GD_SCAN > last && !(carry & 1u)) break;          // the same for every thread: nothing but zeros from here on
        }
        __threadfence();
        __syncthreads();                                              // cur is clear, s_span read, before the next polygon
    }
}

// what both polygon entries refuse
bool gp_bad(const double* xy, int64_t total, const int64_t* poly_offsets, const int32_t* plane_polys, const int32_t* dims,
            const int64_t* bit_offsets, int32_t P, int32_t Q, int64_t max_pixels, const uint8_t* bits, int64_t nbytes, const int32_t* area,
            const int32_t* box, const int32_t* status) {
    if (!xy || !poly_offsets || !plane_polys || !dims || !bit_offsets || !bits || !status || (area == nullptr) != (box == nullptr)) return true;
    if (mb_misaligned(4, plane_polys, dims, bits, area, box, status) || mb_misaligned(8, xy, poly_offsets, bit_offsets)) return true;
    if (P < 1 || P > 65535 || Q < 1 || (int64_t)Q > (int64_t)P * PL_MAX_POLYS) return true;
    return total < 1 || nbytes < 4 || max_pixels < 1 || max_pixels > GT_MAX_PIXELS;
}

// ---- intersections ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gi_init_kernel(int* __restrict__ inter, int N, int* __restrict__ status) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) status[0] = 0;
    if (i < N) inter[i] = 0;
}

// Pair blockIdx.x; workgroup blockIdx.y of it takes the word spans blockIdx.y, + gridDim.y, ... of GI_SPAN words.  A refused pair
// reads no plane: its first workgroup stores -1 and ORs 1 into status, the others leave.  Whole-word loads of both planes, the last
// word of a row masked to the columns below w, a wave reduction and at most one integer atomic per workgroup.
__global__ __launch_bounds__(256) void gi_inter_kernel(const uint8_t* __restrict__ a_bits, int64_t a_bytes, const int64_t* __restrict__ a_off,
                                                       const int* __restrict__ a_dims, int Pa, const uint8_t* __restrict__ b_bits,
                                                       int64_t b_bytes, const int64_t* __restrict__ b_off, const int* __restrict__ b_dims,
                                                       int Pb, const int* __restrict__ pairs, int* __restrict__ inter,
                                                       int* __restrict__ status) {
    const int i = blockIdx.x;
    const int a = pairs[2 * i], b = pairs[2 * i + 1];
    if (!gi_pair_ok(a, b, Pa, Pb, a_dims, a_off, a_bytes, b_dims, b_off, b_bytes)) {    // the same for every thread of the pair
        if (blockIdx.y == 0 && threadIdx.x == 0) { inter[i] = -1; atomicOr(status, 1); }
        return;
    }
    const int h = a_dims[2 * a], w = a_dims[2 * a + 1];
    const int wsr = sz_words_per_row(w), words = h * wsr;             // <= 2^23
    const uint32_t* pa = (const uint32_t*)(a_bits + a_off[a]);
    const uint32_t* pb = (const uint32_t*)(b_bits + b_off[b]);
    int n[1] = {0};
    for (int s0 = blockIdx.y * GI_SPAN; s0 < words; s0 += gridDim.y * GI_SPAN) {
#pragma unroll
        for (int k = 0; k < GI_SPAN / 256; ++k) {
            const int wi = s0 + k * 256 + threadIdx.x;
            if (wi < words) n[0] += gi_word(pa[wi], pb[wi], wi % wsr, w);
        }
    }
    if (mb_block_sum(n) && n[0]) atomicAdd(&inter[i], n[0]);
}

// what both intersection entries refuse
bool gi_bad(const uint8_t* a_bits, int64_t a_bytes, const int64_t* a_off, const int32_t* a_dims, int32_t Pa, const uint8_t* b_bits,
            int64_t b_bytes, const int64_t* b_off, const int32_t* b_dims, int32_t Pb, const int32_t* pairs, int32_t N, int64_t max_words,
            const int32_t* inter, const int32_t* status) {
    if (!a_bits || !a_off || !a_dims || !b_bits || !b_off || !b_dims || !pairs || !inter || !status) return true;
    if (mb_misaligned(4, a_bits, a_dims, b_bits, b_dims, pairs, inter, status) || mb_misaligned(8, a_off, b_off)) return true;
    if (Pa < 1 || Pa > 65535 || Pb < 1 || Pb > 65535 || N < 1 || N > (1 << 20) || a_bytes < 4 || b_bytes < 4) return true;
    return max_words < 1 || max_words > (int64_t)SZ_MAX_SIDE * (SZ_MAX_SIDE / 32);
}

}  // namespace

extern "C" {

int64_t cvlm_mask_rle_decode_workspace_bytes(int32_t P, int64_t max_pixels) {
    if (P < 1 || P > 65535 || max_pixels < 1 || max_pixels > GT_MAX_PIXELS) return CVLM_E_BADARG;
    return (int64_t)P * gd_plane_ws_bytes(max_pixels);
}

int cvlm_mask_rle_decode(const int32_t* counts, int64_t total, const int64_t* run_offsets, const int32_t* dims, const int64_t* bit_offsets,
                         int32_t P, int64_t max_pixels, uint8_t* bits, int64_t bits_bytes, int32_t* area, int32_t* box, int32_t* status,
                         void* workspace, int64_t workspace_bytes, void* stream) {
    if (gd_bad(counts, total, run_offsets, dims, bit_offsets, P, max_pixels, bits, bits_bytes, area, box, status)) return CVLM_E_BADARG;
    const int64_t plane_bytes = gd_plane_ws_bytes(max_pixels);
    if (mb_bad_workspace(workspace, workspace_bytes, plane_bytes)) return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int fit = mb_fit(P, workspace_bytes, plane_bytes);
    const int64_t ws_stride = plane_bytes / 4;
    uint32_t* ws = (uint32_t*)workspace;
    hipLaunchKernelGGL(gd_init_kernel, dim3((P + 255) / 256), dim3(256), 0, st, (int*)area, (int*)box, (int)P, (int*)status);
    CVLM_CHECK_LAUNCH();
    for (int p0 = 0; p0 < P; p0 += fit) {
        const int n = std::min(fit, P - p0);
        const hipError_t e = hipMemsetAsync(ws, 0, (size_t)n * plane_bytes, st);           // verdicts 0, streams clear
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(gd_toggle_kernel, dim3(n), dim3(GD_SCAN), 0, st, counts, total, run_offsets, (const int*)dims, bit_offsets,
                           bits_bytes, max_pixels, p0, ws, ws_stride, (int*)status);
        CVLM_CHECK_LAUNCH();
        hipLaunchKernelGGL(gd_prefix_kernel, dim3(n), dim3(GD_SCAN), 0, st, (const int*)dims, p0, ws, ws_stride);
        CVLM_CHECK_LAUNCH();
        const int rc = gd_rows_round(dims, bit_offsets, bits, bits_bytes, p0, n, max_pixels, ws, ws_stride, area, box, st);
        if (rc) return rc;
    }
    return 0;
}

// The same functions on host memory, plane by plane, through gt_logic.h
int cvlm_debug_mask_rle_decode_host(const int32_t* counts, int64_t total, const int64_t* run_offsets, const int32_t* dims,
                                    const int64_t* bit_offsets, int32_t P, int64_t max_pixels, uint8_t* bits, int64_t bits_bytes,
                                    int32_t* area, int32_t* box, int32_t* status) {
    if (gd_bad(counts, total, run_offsets, dims, bit_offsets, P, max_pixels, bits, bits_bytes, area, box, status)) return CVLM_E_BADARG;
    status[0] = 0;
    std::vector<uint32_t> stream;
    for (int p = 0; p < P; ++p) {
        if (area) mb_init(area, box, p);
        const int h = dims[2 * p], w = dims[2 * p + 1];
        const int64_t off = run_offsets[p], end = run_offsets[p + 1], boff = bit_offsets[p];
        const bool table = sz_plane_ok(h, w, boff, bit_offsets[p + 1], bits_bytes);
        bool good = table && gd_shape_ok(h, w, max_pixels) && gd_slice_ok(off, end, total);
        if (good) {
            const int hw = h * w;
            const int64_t swords = gd_stream_words(hw);
            stream.assign((size_t)swords, 0u);
            int64_t e = 0;
            for (int64_t k = 0; k < end - off && good; ++k) {
                const int c = counts[off + k];
                e += c;
                if (c < 0 || e > hw) { good = false; break; }
                int word;
                uint32_t bit;
                if (k < end - off - 1 && gd_toggle(e, hw, word, bit)) stream[(size_t)word] ^= bit;
            }
            good = good && e == hw;
            if (good) gd_prefix_host(stream.data(), swords, stream.data(), false);
        }
        if (!good) status[0] |= 1;
        if (!table) continue;                                         // nothing of its slice is stored
        gd_rows_host(good ? stream.data() : nullptr, (int64_t)stream.size(), h, w, (uint32_t*)(bits + boff), area ? area + p : nullptr,
                     box ? box + 4 * p : nullptr);
    }
    return 0;
}

int64_t cvlm_mask_poly_decode_workspace_bytes(int32_t P, int64_t max_pixels) {
    if (P < 1 || P > 65535 || max_pixels < 1 || max_pixels > GT_MAX_PIXELS) return CVLM_E_BADARG;
    return (int64_t)P * 2 * gd_plane_ws_bytes(max_pixels);
}

int cvlm_mask_poly_decode(const double* xy, int64_t total, const int64_t* poly_offsets, const int32_t* plane_polys, const int32_t* dims,
                          const int64_t* bit_offsets, int32_t P, int32_t Q, int64_t max_pixels, uint8_t* bits, int64_t bits_bytes,
                          int32_t* area, int32_t* box, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
    if (gp_bad(xy, total, poly_offsets, plane_polys, dims, bit_offsets, P, Q, max_pixels, bits, bits_bytes, area, box, status)) return CVLM_E_BADARG;
    const int64_t plane_bytes = gd_plane_ws_bytes(max_pixels);
    if (mb_bad_workspace(workspace, workspace_bytes, 2 * plane_bytes)) return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int fit = mb_fit(P, workspace_bytes, 2 * plane_bytes);
    const int64_t ws_stride = plane_bytes / 4;
    uint32_t* ws = (uint32_t*)workspace;                                                 // the round's accumulators, then its second streams
    uint32_t* cur = ws + (int64_t)fit * ws_stride;
    const int layered = Q > P;                                                           // some plane has several polygons
    hipLaunchKernelGGL(gd_init_kernel, dim3((P + 255) / 256), dim3(256), 0, st, (int*)area, (int*)box, (int)P, (int*)status);
    CVLM_CHECK_LAUNCH();
    for (int p0 = 0; p0 < P; p0 += fit) {
        const int n = std::min(fit, P - p0);
        const hipError_t e = hipMemsetAsync(ws, 0, (size_t)(layered ? fit + n : n) * plane_bytes, st);   // verdicts 0, streams clear
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(gp_toggle_kernel, dim3(n), dim3(GD_SCAN), 0, st, xy, total, poly_offsets, (const int*)plane_polys, (int)Q,
                           (const int*)dims, bit_offsets, bits_bytes, max_pixels, layered, p0, ws, ws_stride, (int*)status);
        CVLM_CHECK_LAUNCH();
        hipLaunchKernelGGL(gd_prefix_kernel, dim3(n), dim3(GD_SCAN), 0, st, (const int*)dims, p0, ws, ws_stride);
        CVLM_CHECK_LAUNCH();
        if (layered) {
            hipLaunchKernelGGL(gp_layers_kernel, dim3(n), dim3(GD_SCAN), 0, st, xy, total, poly_offsets, (const int*)plane_polys,
                               (const int*)dims, p0, ws, cur, ws_stride, (int*)status);
            CVLM_CHECK_LAUNCH();
        }
        const int rc = gd_rows_round(dims, bit_offsets, bits, bits_bytes, p0, n, max_pixels, ws, ws_stride, area, box, st);
        if (rc) return rc;
    }
    return 0;
}

// The same functions on host memory, plane by plane and polygon by polygon, through poly_logic.h and gt_logic.h
int cvlm_debug_mask_poly_decode_host(const double* xy, int64_t total, const int64_t* poly_offsets, const int32_t* plane_polys,
                                     const int32_t* dims, const int64_t* bit_offsets, int32_t P, int32_t Q, int64_t max_pixels, uint8_t* bits,
                                     int64_t bits_bytes, int32_t* area, int32_t* box, int32_t* status) {
    if (gp_bad(xy, total, poly_offsets, plane_polys, dims, bit_offsets, P, Q, max_pixels, bits, bits_bytes, area, box, status)) return CVLM_E_BADARG;
    status[0] = 0;
    std::vector<uint32_t> acc, cur;
    for (int p = 0; p < P; ++p) {
        if (area) mb_init(area, box, p);
        const int h = dims[2 * p], w = dims[2 * p + 1];
        const int q0 = plane_polys[p], q1 = plane_polys[p + 1];
        const int64_t boff = bit_offsets[p];
        const bool table = sz_plane_ok(h, w, boff, bit_offsets[p + 1], bits_bytes);
        bool good = table && gd_shape_ok(h, w, max_pixels) && pl_polys_ok(q0, q1, Q) && (Q > P || q1 - q0 == 1);
        if (good) {
            const int hw = h * w;
            const int64_t swords = gd_stream_words(hw);
            acc.assign((size_t)swords, 0u);
            for (int q = q0; q < q1 && good; ++q) {
                const int64_t off = poly_offsets[q], end = poly_offsets[q + 1];
                if (!pl_slice_ok(off, end, total)) { good = false; break; }
                const int k = (int)((end - off) >> 1);
                const double* v = xy + off;
                int64_t pts = 0;
                for (int j = 0; j < k && good; ++j) {
                    const int jn = j + 1 < k ? j + 1 : 0;
                    if (!pl_coord_ok(v[2 * j]) || !pl_coord_ok(v[2 * j + 1])) good = false;
                    else if (pl_coord_ok(v[2 * jn]) && pl_coord_ok(v[2 * jn + 1]))
                        pts += pl_edge_of(pl_scale(v[2 * j]), pl_scale(v[2 * j + 1]), pl_scale(v[2 * jn]), pl_scale(v[2 * jn + 1])).n;
                }
                if (!good || pts > PL_MAX_POINTS) { good = false; break; }
                cur.assign((size_t)swords, 0u);
                int up = 0, vp = 0;
                bool first = true;
                for (int j = 0; j < k; ++j) {
                    const int jn = j + 1 < k ? j + 1 : 0;
                    const pl_edge e = pl_edge_of(pl_scale(v[2 * j]), pl_scale(v[2 * j + 1]), pl_scale(v[2 * jn]), pl_scale(v[2 * jn + 1]));
                    for (int d = 0; d < e.n; ++d) {
                        int u, t, word;
                        uint32_t bit;
                        int64_t pos;
                        pl_point(e, d, u, t);
                        if (!first && pl_candidate(up, vp, u, t, h, w, pos) && gd_toggle(pos, hw, word, bit)) cur[(size_t)word] ^= bit;
                        up = u; vp = t;
                        first = false;
                    }
                }
                gd_prefix_host(cur.data(), swords, acc.data(), true);
            }
        }
        if (!good) status[0] |= 1;
        if (!table) continue;                                         // nothing of its slice is stored
        gd_rows_host(good ? acc.data() : nullptr, (int64_t)acc.size(), h, w, (uint32_t*)(bits + boff), area ? area + p : nullptr,
                     box ? box + 4 * p : nullptr);
    }
    return 0;
}

int cvlm_mask_inter_sized(const uint8_t* a_bits, int64_t a_bytes, const int64_t* a_offsets, const int32_t* a_dims, int32_t Pa,
                          const uint8_t* b_bits, int64_t b_bytes, const int64_t* b_offsets, const int32_t* b_dims, int32_t Pb,
                          const int32_t* pairs, int32_t N, int64_t max_words, int32_t* inter, int32_t* status, void* stream) {
    if (gi_bad(a_bits, a_bytes, a_offsets, a_dims, Pa, b_bits, b_bytes, b_offsets, b_dims, Pb, pairs, N, max_words, inter, status))
        return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int gy = (int)std::min<int64_t>((max_words + GI_SPAN - 1) / GI_SPAN, 64);       // larger planes go in strides
    hipLaunchKernelGGL(gi_init_kernel, dim3((N + 255) / 256), dim3(256), 0, st, (int*)inter, (int)N, (int*)status);
    CVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(gi_inter_kernel, dim3(N, gy), dim3(256), 0, st, a_bits, a_bytes, a_offsets, (const int*)a_dims, (int)Pa, b_bits,
                       b_bytes, b_offsets, (const int*)b_dims, (int)Pb, (const int*)pairs, (int*)inter, (int*)status);
    CVLM_CHECK_LAUNCH();
    return 0;
}

int cvlm_debug_mask_inter_sized_host(const uint8_t* a_bits, int64_t a_bytes, const int64_t* a_offsets, const int32_t* a_dims, int32_t Pa,
                                     const uint8_t* b_bits, int64_t b_bytes, const int64_t* b_offsets, const int32_t* b_dims, int32_t Pb,
                                     const int32_t* pairs, int32_t N, int64_t max_words, int32_t* inter, int32_t* status) {
    if (gi_bad(a_bits, a_bytes, a_offsets, a_dims, Pa, b_bits, b_bytes, b_offsets, b_dims, Pb, pairs, N, max_words, inter, status))
        return CVLM_E_BADARG;
    status[0] = 0;
    for (int i = 0; i < N; ++i) {
        const int a = pairs[2 * i], b = pairs[2 * i + 1];
        if (!gi_pair_ok(a, b, Pa, Pb, a_dims, a_offsets, a_bytes, b_dims, b_offsets, b_bytes)) {
            inter[i] = -1;
            status[0] |= 1;
            continue;
        }
        const int h = a_dims[2 * a], w = a_dims[2 * a + 1], wsr = sz_words_per_row(w);
        const uint32_t* pa = (const uint32_t*)(a_bits + a_offsets[a]);
        const uint32_t* pb = (const uint32_t*)(b_bits + b_offsets[b]);
        int n = 0;
        for (int wi = 0; wi < h * wsr; ++wi) n += gi_word(pa[wi], pb[wi], wi % wsr, w);
        inter[i] = n;
    }
    return 0;
}

}  // extern "C"
