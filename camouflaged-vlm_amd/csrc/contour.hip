// Crack contours of sized planes (include/cvlm.h: cvlm_mask_contour_count / cvlm_mask_contour_emit): the boundary between
// set and clear pixels as closed rings of lattice points, foreground on the right, straight runs merged -- COCO polygons out.  The
// per-thread logic -- the corner maps of a lattice word, the dense index, the successor of a vertex -- is contour_logic.h, shared with
// the sequential host entry at the end of this file.  All integers.
//
// Counting: ct_init_kernel, ct_count_kernel (a thread per lattice word, at most one atomic per workgroup and plane), ct_cap_kernel.
// Emitting, through the caller's workspace, planes of one call side by side:
//   ct_map_kernel    a thread per lattice word: the four maps and the word's vertex count;
//   ct_scan_kernel   a workgroup per plane: the exclusive prefix of the counts; a total that is not the slice's length refuses the plane;
//   ct_link_kernel   a thread per lattice word: the successor of each of its vertices;
//   ct_rank_kernel   a workgroup per plane: pointer doubling over the successors carries (smallest dense index seen, steps to it) until
//                    no vertex learns a smaller one; ring lengths at the leaders, their exclusive prefix, the ring counts;
//   ct_place_kernel  a thread per lattice word: each vertex to its ring's base + its rank.
// No workgroup waits for another; a refused plane is never read.
#include <algorithm>
#include <vector>

#include "../../include/cvlm.h"
#include "common.h"
#include "contour_logic.h"

namespace {

constexpr int CT_SCAN = 1024;                                         // threads of the one workgroup per plane of the scan and the rank

// The workspace of a call, in words: a verdict per plane, CT_MAPS maps of map_stride words per plane, CT_RING_ARRAYS arrays of
// round_vertices words
struct ct_layout { int64_t maps, ring, words; };
ct_layout ct_layout_of(int64_t P, int64_t round_vertices, int64_t max_words) {
    ct_layout l;
    l.maps = (P + 3) / 4 * 4;
    l.ring = l.maps + CT_MAPS * P * ct_map_stride(max_words);
    l.words = (l.ring + CT_RING_ARRAYS * round_vertices + 3) / 4 * 4;
    return l;
}

// what the kernels are told about a call
struct ct_call {
    const uint8_t* bits;
    int64_t nbytes;
    const int64_t* offsets;
    const int* dims;
    const int64_t* vertex_offsets;
    int64_t total, round_vertices, map_stride;
    uint32_t* ws;                                                     // verdicts
    uint32_t* maps;
    int* ring;
    int connectivity;
};

// one plane as a kernel sees it
struct ct_plane {
    int h, w, ws, lw, cnt;
    int64_t v0, rb;
    const uint32_t* src;
    bool ok, slice_ok;
};

__device__ __forceinline__ ct_plane ct_plane_of(const ct_call& a, int p) {
    ct_plane q;
    q.h = a.dims[2 * p]; q.w = a.dims[2 * p + 1];
    const int64_t off = a.offsets[p], end = a.offsets[p + 1];
    const int64_t v0 = a.vertex_offsets[p], v1 = a.vertex_offsets[p + 1];
    q.slice_ok = ct_slice_ok(v0, v1, a.total);
    q.ok = q.slice_ok && sz_plane_ok(q.h, q.w, off, end, a.nbytes) && ct_maps_ok(q.h, q.w, a.map_stride) &&
           ct_ring_ok(v0, v1, a.vertex_offsets[0], a.round_vertices);
    q.v0 = v0;
    q.cnt = q.slice_ok ? (int)(v1 - v0) : 0;
    q.rb = v0 - a.vertex_offsets[0];
    q.ws = q.ok ? sz_words_per_row(q.w) : 0;
    q.lw = q.ok ? ct_lattice_words(q.w) : 0;
    q.src = (const uint32_t*)(a.bits + (q.ok ? off : 0));
    return q;
}

__device__ __forceinline__ uint32_t* ct_map(const ct_call& a, int p, int which) {
    return a.maps + ((int64_t)p * CT_MAPS + which) * a.map_stride;
}
__device__ __forceinline__ ct_maps ct_maps_of(const ct_call& a, int p, const ct_plane& q) {
    ct_maps m;
    m.any = ct_map(a, p, 0); m.two = ct_map(a, p, 1); m.up = ct_map(a, p, 2); m.hout = ct_map(a, p, 3);
    m.table = (const int*)ct_map(a, p, 4);
    m.rows = q.h + 1; m.lw = q.lw;
    return m;
}
__device__ __forceinline__ int* ct_ring(const ct_call& a, int which, int64_t rb) { return a.ring + which * a.round_vertices + rb; }

__global__ __launch_bounds__(256) void ct_init_kernel(int* __restrict__ per_plane, int n, int* __restrict__ status, uint32_t* __restrict__ verdict,
                                                      int P) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) status[0] = 0;
    if (i < n) per_plane[i] = 0;
    if (verdict && i < P) verdict[i] = 0u;
}

// n_vertices[blockIdx.y] += the vertices of the lattice words this workgroup walks
__global__ __launch_bounds__(256) void ct_count_kernel(const uint8_t* __restrict__ bits, int64_t nbytes, const int64_t* __restrict__ offsets,
                                                       const int* __restrict__ dims, int connectivity, int* __restrict__ n_vertices,
                                                       int* __restrict__ status) {
    const int p = blockIdx.y;
    const int h = dims[2 * p], w = dims[2 * p + 1];
    const int64_t off = offsets[p], end = offsets[p + 1];
    if (!sz_plane_ok(h, w, off, end, nbytes)) {                       // the same for every thread of the plane
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, 1);
        return;
    }
    const int ws = sz_words_per_row(w), lw = ct_lattice_words(w), words = (h + 1) * lw;
    const uint32_t* src = (const uint32_t*)(bits + off);
    int n[1] = {0};
    for (int k = blockIdx.x * 256 + threadIdx.x; k < words; k += gridDim.x * 256) {
        const int i = k / lw, c = k - i * lw;
        const ct_corner q = ct_corners(i > 0 ? src + (int64_t)(i - 1) * ws : nullptr, i < h ? src + (int64_t)i * ws : nullptr, c, ws, w,
                                       connectivity);
        n[0] += ct_vertices(q);
    }
    if (mb_block_sum(n) && n[0]) atomicAdd(&n_vertices[p], n[0]);
}

__global__ __launch_bounds__(256) void ct_cap_kernel(int* __restrict__ n_vertices, int P, int* __restrict__ status) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < P && n_vertices[p] > CT_MAX_VERTS) {
        n_vertices[p] = 0;
        atomicOr(status, 1);
    }
}

__global__ __launch_bounds__(256) void ct_map_kernel(ct_call a) {
    const int p = blockIdx.y;
    const ct_plane q = ct_plane_of(a, p);
    if (!q.ok) return;
    const int words = (q.h + 1) * q.lw;
    uint32_t *any = ct_map(a, p, 0), *two = ct_map(a, p, 1), *up = ct_map(a, p, 2), *hout = ct_map(a, p, 3);
    int* table = (int*)ct_map(a, p, 4);
    for (int k = blockIdx.x * 256 + threadIdx.x; k < words; k += gridDim.x * 256) {       // words <= map_stride: ct_maps_ok
        const int i = k / q.lw, c = k - i * q.lw;
        const ct_corner r = ct_corners(i > 0 ? q.src + (int64_t)(i - 1) * q.ws : nullptr, i < q.h ? q.src + (int64_t)i * q.ws : nullptr, c,
                                       q.ws, q.w, a.connectivity);
        any[k] = r.any; two[k] = r.two; up[k] = r.up; hout[k] = r.hout;
        table[k] = ct_vertices(r);
    }
}

// Exclusive prefix of v[0 .. n) in place over the workgroup's CT_SCAN threads -> the total, in every thread.  Sequential over slabs of
// CT_SCAN entries with a carry; inside a slab a wave scan by shuffles and the waves' totals through LDS, double-buffered by the slab's
// parity: one barrier per slab.  Every thread of the workgroup calls it.  out may be v.
__device__ __forceinline__ int ct_block_scan(const int* v, int* out, int n, int (*s_sum)[CT_SCAN / 64]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int k0 = 0, slab = 0; k0 < n; k0 += CT_SCAN, slab ^= 1) {
        const int k = k0 + threadIdx.x;
        const int x = k < n ? v[k] : 0;
        int sum = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(sum, o, 64);
            if (lane >= o) sum += t;
        }
        if (lane == 63) s_sum[slab][wave] = sum;
        __syncthreads();
        int before = carry, all = carry;
#pragma unroll
        for (int i = 0; i < CT_SCAN / 64; ++i) {
            const int t = s_sum[slab][i];
            if (i < wave) before += t;
            all += t;
        }
        if (k < n) out[k] = before + sum - x;
        carry = all;
    }
    return carry;
}

// One workgroup per plane: the table becomes the vertices before each lattice word; the verdict is 1 when they are as many as the slice
__global__ __launch_bounds__(CT_SCAN) void ct_scan_kernel(ct_call a, int* __restrict__ status) {
    __shared__ int s_sum[2][CT_SCAN / 64];
    const int p = blockIdx.x;
    const ct_plane q = ct_plane_of(a, p);
    if (!q.ok) {                                                      // the same for every thread
        if (threadIdx.x == 0) atomicOr(status, 1);
        return;
    }
    int* table = (int*)ct_map(a, p, 4);
    const int total = ct_block_scan(table, table, (q.h + 1) * q.lw, s_sum);
    if (threadIdx.x == 0) {
        if (total == q.cnt) a.ws[p] = 1u;
        else atomicOr(status, 1);
    }
}

// the vertices of lattice word k of a plane, west to east: f(bit, east, dense index)
template <typename F>
__device__ __forceinline__ void ct_for_vertices(const ct_maps& m, int k, F&& f) {
    const uint32_t two = m.two[k];
    int v = m.table[k];
    for (uint32_t rest = m.any[k]; rest; rest &= rest - 1u) {
        const int bit = __builtin_ctz(rest);
        f(bit, 0, v++);
        if ((two >> bit) & 1u) f(bit, 1, v++);
    }
}

__global__ __launch_bounds__(256) void ct_link_kernel(ct_call a) {
    const int p = blockIdx.y;
    if (a.ws[p] == 0u) return;                                        // the whole workgroup
    const ct_plane q = ct_plane_of(a, p);
    const ct_maps m = ct_maps_of(a, p, q);
    int *succ = ct_ring(a, 0, q.rb), *next = ct_ring(a, 1, q.rb), *lead = ct_ring(a, 3, q.rb), *dist = ct_ring(a, 5, q.rb);
    const int words = (q.h + 1) * q.lw, cnt = q.cnt;
    for (int k = blockIdx.x * 256 + threadIdx.x; k < words; k += gridDim.x * 256) {
        const int i = k / q.lw, c = k - i * q.lw;
        ct_for_vertices(m, k, [&](int bit, int east, int v) {
            if ((unsigned)v >= (unsigned)cnt) return;                 // the slot against the slice, before every store
            int s = ct_succ(m, i, c, bit, east, v);
            if ((unsigned)s >= (unsigned)cnt) s = v;
            succ[v] = s; next[v] = s; lead[v] = v; dist[v] = 0;
        });
    }
}

// One workgroup per plane.  Round r doubles the window of every vertex from 2^r to 2^(r + 1) vertices: (the smallest dense index in
// the window, the steps to it) joined with those of the vertex one window ahead, which `next` names.  A round in which no vertex
// learns a smaller index ends the loop: every window then holds its ring's smallest vertex, the LEADER, and the steps to it are the
// distance along the ring.  Values pass between the threads through global memory; the barrier orders them.
__global__ __launch_bounds__(CT_SCAN) void ct_rank_kernel(ct_call a, int* __restrict__ n_rings, int* __restrict__ status) {
    __shared__ int s_sum[2][CT_SCAN / 64], s_changed[3], s_rings[2];
    const int p = blockIdx.x;
    if (a.ws[p] == 0u) return;                                        // the whole workgroup
    const ct_plane q = ct_plane_of(a, p);
    const int cnt = q.cnt;
    const int* succ = ct_ring(a, 0, q.rb);
    if (threadIdx.x < 3) s_changed[threadIdx.x] = 0;
    if (threadIdx.x < 2) s_rings[threadIdx.x] = 0;
    __syncthreads();
    int cur = 0;
    for (int r = 0; r < CT_MAX_ROUNDS; ++r, cur ^= 1) {
        const int *next = ct_ring(a, 1 + cur, q.rb), *lead = ct_ring(a, 3 + cur, q.rb), *dist = ct_ring(a, 5 + cur, q.rb);
        int *next_o = ct_ring(a, 2 - cur, q.rb), *lead_o = ct_ring(a, 4 - cur, q.rb), *dist_o = ct_ring(a, 6 - cur, q.rb);
        bool changed = false;
        for (int v = threadIdx.x; v < cnt; v += CT_SCAN) {
            int j = next[v];
            if ((unsigned)j >= (unsigned)cnt) j = v;
            const int mine = lead[v], ahead = lead[j];
            int jj = next[j];
            if ((unsigned)jj >= (unsigned)cnt) jj = v;
            next_o[v] = jj;
            if (ahead < mine) {
                lead_o[v] = ahead; dist_o[v] = (1 << r) + dist[j];
                changed = true;
            } else {
                lead_o[v] = mine; dist_o[v] = dist[v];
            }
        }
        if (changed) s_changed[r % 3] = 1;
        __syncthreads();
        const int any = s_changed[r % 3];
        if (threadIdx.x == 0) s_changed[(r + 2) % 3] = 0;             // read last in round r - 1, set next in round r + 2
        if (!any) break;                                              // the same for every thread; `cur` holds what `other` holds
    }
    const int *lead = ct_ring(a, 3 + cur, q.rb), *dist = ct_ring(a, 5 + cur, q.rb);
    int *len = ct_ring(a, 1, q.rb), *base = ct_ring(a, 2, q.rb);      // the two copies of `next` are free now
    int outer = 0, holes = 0;
    for (int v = threadIdx.x; v < cnt; v += CT_SCAN) {
        int n = 0;
        if (lead[v] == v) {
            const int s = succ[v];
            n = (unsigned)s < (unsigned)cnt ? dist[s] + 1 : 1;
            if (s == v + 1) ++outer;                                  // the first edge heads east; a hole's heads south
            else ++holes;
        }
        len[v] = n;
    }
    if (outer) atomicAdd(&s_rings[0], outer);
    if (holes) atomicAdd(&s_rings[1], holes);
    __syncthreads();
    const int total = ct_block_scan(len, base, cnt, s_sum);
    if (threadIdx.x == 0) {
        if (total == cnt) {
            n_rings[2 * p] = s_rings[0]; n_rings[2 * p + 1] = s_rings[1];
        } else {                                                      // ring lengths that do not add up: no contour's successors
            a.ws[p] = 0u;
            atomicOr(status, 1);
        }
    }
}

// Both copies of (leader, distance) hold the final values: the round that ended the loop changed nothing.  This reads the first.
__global__ __launch_bounds__(256) void ct_place_kernel(ct_call a, uint32_t* __restrict__ xy, uint8_t* __restrict__ ring_start) {
    const int p = blockIdx.y;
    const ct_plane q = ct_plane_of(a, p);
    if (a.ws[p] == 0u) {                                              // the whole workgroup: a refused plane's slice holds zeros
        if (q.slice_ok)
            for (int t = blockIdx.x * 256 + threadIdx.x; t < q.cnt; t += gridDim.x * 256) { xy[q.v0 + t] = 0u; ring_start[q.v0 + t] = 0; }
        return;
    }
    const ct_maps m = ct_maps_of(a, p, q);
    const int words = (q.h + 1) * q.lw, cnt = q.cnt;
    const int *len = ct_ring(a, 1, q.rb), *base = ct_ring(a, 2, q.rb);
    const int *lead0 = ct_ring(a, 3, q.rb), *dist0 = ct_ring(a, 5, q.rb);
    for (int k = blockIdx.x * 256 + threadIdx.x; k < words; k += gridDim.x * 256) {
        const int i = k / q.lw, c = k - i * q.lw;
        ct_for_vertices(m, k, [&](int bit, int east, int v) {
            if ((unsigned)v >= (unsigned)cnt) return;
            const int l = lead0[v];
            if ((unsigned)l >= (unsigned)cnt) return;
            const int n = len[l], d = dist0[v];
            if (d < 0 || d >= n) return;
            const int rank = ct_rank(d, n);
            const int64_t slot = (int64_t)base[l] + rank;
            if (slot < 0 || slot >= cnt) return;                      // the slot against the slice, before the store
            xy[q.v0 + slot] = ct_pack_xy(32 * c + bit, i);
            ring_start[q.v0 + slot] = rank == 0;
        });
    }
}

bool ct_bad_planes(const uint8_t* bits, int64_t nbytes, const int64_t* offsets, const int32_t* dims, int32_t P, int32_t connectivity,
                   int64_t max_words) {
    if (!bits || !offsets || !dims || mb_misaligned(4, bits, dims) || mb_misaligned(8, offsets)) return true;
    if (P < 1 || P > 65535 || nbytes < 4 || max_words < 1 || max_words > (int64_t)SZ_MAX_SIDE * (SZ_MAX_SIDE / 32)) return true;
    return connectivity != 4 && connectivity != 8;
}

bool ct_bad_emit(const uint8_t* bits, int64_t nbytes, int32_t P, const int64_t* vertex_offsets, int64_t round_vertices, const uint8_t* xy,
                 const uint8_t* ring_start, const int32_t* n_rings, int64_t total, const int32_t* status, const void* workspace,
                 int64_t workspace_bytes, bool need_ws, int64_t max_words) {
    if (!vertex_offsets || !n_rings || !status || total < 0 || round_vertices < 0 || round_vertices > (int64_t)P * CT_MAX_VERTS) return true;
    if (total > 0 && (!xy || !ring_start)) return true;
    if (mb_misaligned(8, vertex_offsets) || mb_misaligned(4, xy, n_rings, status)) return true;
    const uint64_t nb = (uint64_t)nbytes, nx = 4 * (uint64_t)total, nr = (uint64_t)total, ng = 8 * (uint64_t)P;
    const void* outs[4] = {xy, ring_start, n_rings, status};
    const uint64_t sizes[4] = {nx, nr, ng, 4};
    for (int i = 0; i < 4; ++i) {
        if (mb_ranges_meet(outs[i], sizes[i], bits, nb)) return true;
        for (int j = i + 1; j < 4; ++j)
            if (mb_ranges_meet(outs[i], sizes[i], outs[j], sizes[j])) return true;
    }
    if (!need_ws) return false;
    const int64_t need = 4 * ct_layout_of(P, round_vertices, max_words).words;
    if (mb_bad_workspace(workspace, workspace_bytes, need)) return true;
    const uint64_t nw = (uint64_t)workspace_bytes;
    if (mb_ranges_meet(workspace, nw, bits, nb)) return true;
    for (int i = 0; i < 4; ++i)
        if (mb_ranges_meet(workspace, nw, outs[i], sizes[i])) return true;
    return false;
}

// workgroups per plane of the kernels that walk lattice words: about 4096 in all, at most 256, no more than the largest plane has work for
int ct_grid_x(int32_t P, int64_t max_words) {
    const int64_t by_work = (ct_map_stride(max_words) + 255) / 256;
    const int64_t want = (4096 + P - 1) / P;
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(by_work, want), 256));
}

}  // namespace

extern "C" {

int64_t cvlm_mask_contour_workspace_bytes(int32_t P, int64_t round_vertices, int64_t max_words) {
    if (P < 1 || P > 65535 || round_vertices < 0 || round_vertices > (int64_t)P * CT_MAX_VERTS || max_words < 1 ||
        max_words > (int64_t)SZ_MAX_SIDE * (SZ_MAX_SIDE / 32))
        return CVLM_E_BADARG;
    return 4 * ct_layout_of(P, round_vertices, max_words).words;
}

int cvlm_mask_contour_count(const uint8_t* bits, int64_t n_bytes, const int64_t* offsets, const int32_t* dims, int32_t P, int32_t connectivity,
                            int64_t max_words, int32_t* n_vertices, int32_t* status, void* stream) {
    if (ct_bad_planes(bits, n_bytes, offsets, dims, P, connectivity, max_words) || !n_vertices || !status ||
        mb_misaligned(4, n_vertices, status))
        return CVLM_E_BADARG;
    if (mb_ranges_meet(n_vertices, 4 * (uint64_t)P, bits, (uint64_t)n_bytes) || mb_ranges_meet(status, 4, bits, (uint64_t)n_bytes) ||
        mb_ranges_meet(n_vertices, 4 * (uint64_t)P, status, 4))
        return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ct_init_kernel, dim3((P + 255) / 256), dim3(256), 0, st, (int*)n_vertices, (int)P, (int*)status, (uint32_t*)nullptr, 0);
    CVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(ct_count_kernel, dim3(ct_grid_x(P, max_words), P), dim3(256), 0, st, bits, n_bytes, offsets, (const int*)dims,
                       (int)connectivity, (int*)n_vertices, (int*)status);
    CVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(ct_cap_kernel, dim3((P + 255) / 256), dim3(256), 0, st, (int*)n_vertices, (int)P, (int*)status);
    CVLM_CHECK_LAUNCH();
    return 0;
}

int cvlm_mask_contour_emit(const uint8_t* bits, int64_t n_bytes, const int64_t* offsets, const int32_t* dims, int32_t P, int32_t connectivity,
                           int64_t max_words, const int64_t* vertex_offsets, int64_t round_vertices, int16_t* xy, uint8_t* ring_start,
                           int32_t* n_rings, int64_t total, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
    if (ct_bad_planes(bits, n_bytes, offsets, dims, P, connectivity, max_words) ||
        ct_bad_emit(bits, n_bytes, P, vertex_offsets, round_vertices, (const uint8_t*)xy, ring_start, n_rings, total, status, workspace,
                    workspace_bytes, true, max_words))
        return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const ct_layout l = ct_layout_of(P, round_vertices, max_words);
    ct_call a;
    a.bits = bits; a.nbytes = n_bytes; a.offsets = offsets; a.dims = (const int*)dims; a.vertex_offsets = vertex_offsets;
    a.total = total; a.round_vertices = round_vertices; a.map_stride = ct_map_stride(max_words);
    a.ws = (uint32_t*)workspace; a.maps = a.ws + l.maps; a.ring = (int*)(a.ws + l.ring);
    a.connectivity = connectivity;
    const int gx = ct_grid_x(P, max_words);
    hipLaunchKernelGGL(ct_init_kernel, dim3((2 * P + 255) / 256), dim3(256), 0, st, (int*)n_rings, 2 * (int)P, (int*)status, a.ws, (int)P);
    CVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(ct_map_kernel, dim3(gx, P), dim3(256), 0, st, a);
    CVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(ct_scan_kernel, dim3(P), dim3(CT_SCAN), 0, st, a, (int*)status);
    CVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(ct_link_kernel, dim3(gx, P), dim3(256), 0, st, a);
    CVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(ct_rank_kernel, dim3(P), dim3(CT_SCAN), 0, st, a, (int*)n_rings, (int*)status);
    CVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(ct_place_kernel, dim3(gx, P), dim3(256), 0, st, a, (uint32_t*)xy, ring_start);
    CVLM_CHECK_LAUNCH();
    return 0;
}

// The same contours on host memory: the maps and the successors through contour_logic.h, the rings by following the successors from
// every vertex not yet seen, in dense order -- the first of a ring is its leader.  vertex_offsets == NULL: only n_vertices.
int cvlm_debug_mask_contour_host(const uint8_t* bits, int64_t n_bytes, const int64_t* offsets, const int32_t* dims, int32_t P,
                                 int32_t connectivity, int32_t* n_vertices, const int64_t* vertex_offsets, int16_t* xy, uint8_t* ring_start,
                                 int32_t* n_rings, int64_t total, int32_t* status) {
    if (ct_bad_planes(bits, n_bytes, offsets, dims, P, connectivity, 1) || !n_vertices || !status || mb_misaligned(4, n_vertices, status))
        return CVLM_E_BADARG;
    if (!vertex_offsets && (xy || ring_start || n_rings)) return CVLM_E_BADARG;
    if (vertex_offsets && ct_bad_emit(bits, n_bytes, P, vertex_offsets, 0, (const uint8_t*)xy, ring_start, n_rings, total, status, nullptr, 0,
                                      false, 1))
        return CVLM_E_BADARG;
    status[0] = 0;
    uint32_t* out = (uint32_t*)xy;
    std::vector<uint32_t> maps[4];
    std::vector<int> table, succ;
    std::vector<char> seen;
    for (int p = 0; p < P; ++p) {
        n_vertices[p] = 0;
        if (vertex_offsets) n_rings[2 * p] = n_rings[2 * p + 1] = 0;
        const int h = dims[2 * p], w = dims[2 * p + 1];
        const bool plane_ok = sz_plane_ok(h, w, offsets[p], offsets[p + 1], n_bytes);
        const int64_t v0 = vertex_offsets ? vertex_offsets[p] : 0, v1 = vertex_offsets ? vertex_offsets[p + 1] : 0;
        const bool slice_ok = vertex_offsets && ct_slice_ok(v0, v1, total);
        const int cnt = slice_ok ? (int)(v1 - v0) : 0;
        auto refuse = [&]() {
            status[0] |= 1;
            if (slice_ok)
                for (int t = 0; t < cnt; ++t) { out[v0 + t] = 0u; ring_start[v0 + t] = 0; }
        };
        if (!plane_ok) { refuse(); continue; }
        const int ws = sz_words_per_row(w), lw = ct_lattice_words(w), words = (h + 1) * lw;
        const uint32_t* src = (const uint32_t*)(bits + offsets[p]);
        for (auto& m : maps) m.assign((size_t)words, 0u);
        table.assign((size_t)words, 0);
        int64_t n = 0;
        for (int k = 0; k < words; ++k) {
            const int i = k / lw, c = k - i * lw;
            const ct_corner q = ct_corners(i > 0 ? src + (int64_t)(i - 1) * ws : nullptr, i < h ? src + (int64_t)i * ws : nullptr, c, ws, w,
                                           connectivity);
            maps[0][(size_t)k] = q.any; maps[1][(size_t)k] = q.two; maps[2][(size_t)k] = q.up; maps[3][(size_t)k] = q.hout;
            table[(size_t)k] = (int)n;
            n += ct_vertices(q);
        }
        if (n > CT_MAX_VERTS) { refuse(); continue; }
        n_vertices[p] = (int32_t)n;
        if (!vertex_offsets) continue;
        if (!slice_ok || n != cnt) { n_vertices[p] = slice_ok ? (int32_t)n : 0; refuse(); continue; }
        ct_maps m;
        m.any = maps[0].data(); m.two = maps[1].data(); m.up = maps[2].data(); m.hout = maps[3].data(); m.table = table.data();
        m.rows = h + 1; m.lw = lw;
        succ.assign((size_t)cnt, 0);
        std::vector<uint32_t> where((size_t)cnt);
        for (int k = 0; k < words; ++k) {
            const int i = k / lw, c = k - i * lw;
            int v = table[(size_t)k];
            for (uint32_t rest = maps[0][(size_t)k]; rest; rest &= rest - 1u) {
                const int bit = __builtin_ctz(rest);
                const int slots = (maps[1][(size_t)k] >> bit) & 1u ? 2 : 1;
                for (int east = 0; east < slots; ++east, ++v) {
                    int s = ct_succ(m, i, c, bit, east, v);
                    if (s < 0 || s >= cnt) s = v;
                    succ[(size_t)v] = s;
                    where[(size_t)v] = ct_pack_xy(32 * c + bit, i);
                }
            }
        }
        seen.assign((size_t)cnt, 0);
        int64_t pos = 0;
        int outer = 0, holes = 0;
        bool whole = true;
        for (int v = 0; v < cnt && whole; ++v) {
            if (seen[(size_t)v]) continue;
            if (succ[(size_t)v] == v + 1) ++outer;
            else ++holes;
            int u = v;
            do {
                if (seen[(size_t)u] || pos >= cnt) { whole = false; break; }
                seen[(size_t)u] = 1;
                out[v0 + pos] = where[(size_t)u];
                ring_start[v0 + pos] = u == v;
                ++pos;
                u = succ[(size_t)u];
            } while (u != v);
        }
        if (!whole || pos != cnt) { refuse(); continue; }
        n_rings[2 * p] = outer; n_rings[2 * p + 1] = holes;
    }
    return 0;
}

}  // extern "C"
