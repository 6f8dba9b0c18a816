// Simplified contour rings (include/cvlm.h: cvlm_contour_simplify_mark / cvlm_contour_simplify_emit): Ramer-Douglas-Peucker
// on the closed rings of cvlm_mask_contour_emit, in exact integers, the rings staying on the device.  The per-thread logic -- the key of a
// vertex under a chord, the keep test, the anchor rule -- is simplify_logic.h, shared with the sequential host entry at the end of this file.
//
// Marking, one workgroup of SP_WG threads per plane over the plane's slice of the caller's workspace (sp_mark_kernel):
//   the ring of every vertex by one segmented max-scan of ring_start with a slab carry; the ring's end parked at its start;
//   anchor B of every ring by an integer atomicMax of |v - v_0|^2 at the ring's start, then an atomicMin of the index among the equals;
//   rounds: every resting vertex bids its key at its left anchor (atomicMax), the equals bid their index (atomicMin), every anchor
//   applies the keep test to the winner and splits its chord, every resting vertex behind the new anchor moves to it.  A chord that
//   did not split is final and its vertices bid no more.  A workgroup-uniform flag ends the loop; a round that goes on has kept a vertex;
//   rings left with A and B alone are dropped; the counts.
// Emitting, one workgroup per plane (sp_emit_kernel): the kept vertices counted against the output slice, then a streaming scan of
// `keep` with a slab carry and one 32-bit store per kept vertex.
// No workgroup waits for another; a refused plane is never read.  All integers; max / min atomics only, so the result does not depend
// on the order in which the threads run.
#include <vector>

#include "../../include/cvlm.h"
#include "common.h"
#include "simplify_logic.h"

namespace {

typedef unsigned long long u64;

constexpr int SP_WG = 1024;                                           // threads of the one workgroup per plane
constexpr int SP_WORDS_PER_VERTEX = 6;                                // best_num (two words), rs, seg, nxt, best_idx

// the workspace of a call, in 4-byte words: best_num first, which keeps it on 8 bytes; behind the arrays four words of which the first
// holds, after the call, the rounds of its deepest plane (tools/bench_simplify.py reads it; no caller needs to)
int64_t sp_tail_word(int64_t round_vertices) { return (SP_WORDS_PER_VERTEX * round_vertices + 3) / 4 * 4; }
int64_t sp_workspace_words(int64_t round_vertices) { return sp_tail_word(round_vertices) + 4; }

// what the mark kernel is told about a call
struct sp_call {
    const uint32_t* xy;
    const uint8_t* ring_start;
    const int64_t* vertex_offsets;
    const int* T;
    int64_t total, round_vertices;
    u64* best_num;                                                    // per anchor: the largest key bid under its chord
    int *rs, *seg, *nxt, *best_idx;                                   // per vertex: its ring's start, its left anchor; per anchor: the next one, the bidder
    int* deepest;                                                     // one word: the rounds of the call's deepest plane
};

// one plane as a kernel sees it
struct sp_plane {
    int64_t v0, rb;
    int cnt, T;
    bool slice_ok, ok;
};

__device__ __forceinline__ sp_plane sp_plane_of(const sp_call& a, int p) {
    sp_plane q;
    const int64_t v0 = a.vertex_offsets[p], v1 = a.vertex_offsets[p + 1];
    q.T = a.T[p];
    q.slice_ok = ct_slice_ok(v0, v1, a.total);
    q.ok = q.slice_ok && sp_tolerance_ok(q.T) && ct_ring_ok(v0, v1, a.vertex_offsets[0], a.round_vertices);
    q.v0 = v0;
    q.cnt = q.slice_ok ? (int)(v1 - v0) : 0;
    q.rb = v0 - a.vertex_offsets[0];
    return q;
}

// The bids are integer atomics, which the device carries out in its second-level cache; what reads or resets them goes there too.
__device__ __forceinline__ u64 sp_load(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int sp_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void sp_reset(u64* num, int* idx, int at, int state) {
    __hip_atomic_store(num + at, (u64)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(idx + at, state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void sp_init_kernel(int* __restrict__ status, int* __restrict__ deepest) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        status[0] = 0;
        if (deepest) deepest[0] = 0;
    }
}

// rs[k] = the largest index <= k that starts a ring (start[0] != 0 is the caller's).  Sequential over slabs of SP_WG entries with a
// carry; inside a slab a wave scan by shuffles and the waves' results through LDS, double-buffered by the slab's parity: one barrier
// per slab.  Every thread of the workgroup calls it.
__device__ __forceinline__ void sp_ring_starts(const uint8_t* start, int* rs, int n, int (*s_part)[SP_WG / 64]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int k0 = 0, slab = 0; k0 < n; k0 += SP_WG, slab ^= 1) {
        const int k = k0 + threadIdx.x;
        int m = k < n && start[k] != 0 ? k : -1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(m, o, 64);
            if (lane >= o) m = max(m, t);
        }
        if (lane == 63) s_part[slab][wave] = m;
        __syncthreads();
        int before = carry, all = carry;
#pragma unroll
        for (int i = 0; i < SP_WG / 64; ++i) {
            const int t = s_part[slab][i];
            if (i < wave) before = max(before, t);
            all = max(all, t);
        }
        if (k < n) rs[k] = max(before, m);
        carry = all;
    }
}

// the point at the far end j of a chord of the ring that starts at r: a vertex, or the closing appearance of v_0
__device__ __forceinline__ sp_pt sp_far_end(const uint32_t* xy, const uint8_t* start, int j, int r, int cnt) {
    const int at = sp_closes(start, j, cnt) ? r : j;
    return sp_unpack(xy[(unsigned)at < (unsigned)cnt ? at : 0]);
}

__global__ __launch_bounds__(SP_WG) void sp_mark_kernel(sp_call a, uint8_t* __restrict__ keep_all, int* __restrict__ n_kept,
                                                        int* __restrict__ n_rings_out, int* __restrict__ status) {
    __shared__ int s_part[2][SP_WG / 64], s_changed[3], s_total[3];
    const int p = blockIdx.x;
    const sp_plane q = sp_plane_of(a, p);
    const int cnt = q.cnt;
    // a slice that does not begin with a ring's start is no plane's rings -- a refused plane of the contour call passed through
    const bool ok = q.ok && (cnt == 0 || a.ring_start[q.v0] != 0);   // the same for every thread
    if (!ok || cnt == 0) {
        if (q.slice_ok)
            for (int v = threadIdx.x; v < cnt; v += SP_WG) keep_all[q.v0 + v] = 0;
        if (threadIdx.x == 0) {
            n_kept[p] = 0; n_rings_out[2 * p] = 0; n_rings_out[2 * p + 1] = 0;
            if (!ok) atomicOr(status, 1);
        }
        return;
    }
    const uint32_t* xy = a.xy + q.v0;
    const uint8_t* start = a.ring_start + q.v0;
    uint8_t* keep = keep_all + q.v0;                                  // 0 rests, 1 anchor, 2 kept in this round
    u64* best_num = a.best_num + q.rb;
    int *rs = a.rs + q.rb, *seg = a.seg + q.rb, *nxt = a.nxt + q.rb, *best_idx = a.best_idx + q.rb;
    const int T = q.T;
    if (threadIdx.x < 3) { s_changed[threadIdx.x] = 0; s_total[threadIdx.x] = 0; }
    // the start of v's ring, held against the slice: a ring starts at or before its vertices
    auto ring_of = [&](int v) {
        const int r = rs[v];
        return (unsigned)r <= (unsigned)v ? r : v;
    };

    sp_ring_starts(start, rs, cnt, s_part);
    __syncthreads();
    // the end of every ring parked in nxt at its start; A kept; the bids for B opened
    for (int v = threadIdx.x; v < cnt; v += SP_WG) {
        const bool first = start[v] != 0;
        if (first && v > 0) nxt[ring_of(v - 1)] = v;
        if (v == cnt - 1) nxt[ring_of(v)] = cnt;
        keep[v] = first;
        if (first) sp_reset(best_num, best_idx, v, SP_NONE);
    }
    __syncthreads();
    for (int v = threadIdx.x; v < cnt; v += SP_WG) {
        const int r = ring_of(v);
        atomicMax(&best_num[r], (u64)sp_d2(sp_unpack(xy[v]), sp_unpack(xy[r])));
    }
    __syncthreads();
    for (int v = threadIdx.x; v < cnt; v += SP_WG) {
        const int r = ring_of(v);
        if (sp_d2(sp_unpack(xy[v]), sp_unpack(xy[r])) == sp_load(&best_num[r])) atomicMin(&best_idx[r], v);
    }
    __syncthreads();
    // B of the ring that starts at r, held against the ring before use: r itself where the ring is one point
    auto anchor_b = [&](int r) {
        const int b = sp_load(&best_idx[r]);
        return b > r && b < cnt && rs[b] == r ? b : r;
    };
    for (int v = threadIdx.x; v < cnt; v += SP_WG) {
        const int r = ring_of(v), b = anchor_b(r);
        seg[v] = b != r && v > b ? b : r;
    }
    __syncthreads();
    for (int v = threadIdx.x; v < cnt; v += SP_WG) {
        if (start[v] == 0) continue;
        const int b = anchor_b(v);
        if (b != v) {
            nxt[b] = nxt[v]; nxt[v] = b;
            keep[b] = 1;
            sp_reset(best_num, best_idx, b, SP_NONE);
        }
        sp_reset(best_num, best_idx, v, SP_NONE);
    }
    __syncthreads();

    // the key of resting vertex v under the chord of its left anchor -> false where the chord is final or the workspace names no chord
    auto bid = [&](int v, int& i, u64& num) {
        i = seg[v];
        if ((unsigned)i >= (unsigned)v) return false;                 // the index against the slice, before use
        if (sp_load(&best_idx[i]) == SP_FINAL) return false;
        const int j = nxt[i];
        if (j <= v || j > cnt) return false;
        uint64_t L;
        num = sp_key(sp_unpack(xy[i]), sp_far_end(xy, start, j, ring_of(v), cnt), sp_unpack(xy[v]), &L);
        return true;
    };
    int rounds = 0;
    for (int r = 0; r <= cnt; ++r) {                                  // a round that goes on keeps a vertex: cnt rounds at the most
        ++rounds;
        for (int v = threadIdx.x; v < cnt; v += SP_WG) {
            int i; u64 num;
            if (keep[v] == 0 && bid(v, i, num)) atomicMax(&best_num[i], num);
        }
        __syncthreads();
        for (int v = threadIdx.x; v < cnt; v += SP_WG) {
            int i; u64 num;
            if (keep[v] == 0 && bid(v, i, num) && num == sp_load(&best_num[i])) atomicMin(&best_idx[i], v);
        }
        __syncthreads();
        bool changed = false;
        for (int v = threadIdx.x; v < cnt; v += SP_WG) {
            if (keep[v] != 1) continue;
            const int m = sp_load(&best_idx[v]);
            if (m == SP_FINAL) continue;
            const int j = nxt[v];
            bool split = false;
            if (m > v && m < j && j <= cnt && keep[m] == 0) {         // SP_NONE: nobody bid; anything else out of the chord: no split
                uint64_t L;
                const uint64_t num = sp_key(sp_unpack(xy[v]), sp_far_end(xy, start, j, ring_of(v), cnt), sp_unpack(xy[m]), &L);
                split = sp_keeps(num, L, T);
            }
            if (split) {
                nxt[m] = j; nxt[v] = m;
                keep[m] = 2;
                sp_reset(best_num, best_idx, m, SP_NONE);
                sp_reset(best_num, best_idx, v, SP_NONE);
                changed = true;
            } else {
                sp_reset(best_num, best_idx, v, SP_FINAL);
            }
        }
        if (changed) s_changed[r % 3] = 1;
        __syncthreads();
        const int any = s_changed[r % 3];
        if (threadIdx.x == 0) s_changed[(r + 2) % 3] = 0;             // read last in round r - 1, set next in round r + 2
        if (!any) break;                                              // the same for every thread
        for (int v = threadIdx.x; v < cnt; v += SP_WG) {             // each thread meets its own vertices again: no barrier behind this
            const int k = keep[v];
            if (k == 2) keep[v] = 1;
            if (k != 0) continue;
            const int i = seg[v];
            if ((unsigned)i >= (unsigned)v) continue;
            const int n = nxt[i];
            if (n > i && n < v) seg[v] = n;
        }
    }

    // a ring left with A and B alone lies within T / 4 of one segment: dropped.  seg of a ring's start is free: it holds the verdict
    int outer = 0, holes = 0;
    for (int v = threadIdx.x; v < cnt; v += SP_WG) {
        if (start[v] == 0) continue;
        const int b = nxt[v];
        bool dropped = b <= v || sp_closes(start, b, cnt);
        if (!dropped) {
            const int c = nxt[b];
            dropped = c <= b || sp_closes(start, c, cnt);
        }
        seg[v] = dropped;
        if (dropped) continue;
        if (v + 1 < cnt && sp_ring_code(sp_unpack(xy[v]), sp_unpack(xy[v + 1])) == 1) ++outer;
        else ++holes;
    }
    if (outer) atomicAdd(&s_total[1], outer);
    if (holes) atomicAdd(&s_total[2], holes);
    __syncthreads();
    int kept = 0;
    for (int v = threadIdx.x; v < cnt; v += SP_WG) {
        const bool k = keep[v] == 1 && seg[ring_of(v)] == 0;
        keep[v] = k;
        kept += k;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o, 64);
    if ((threadIdx.x & 63) == 0 && kept) atomicAdd(&s_total[0], kept);
    __syncthreads();
    if (threadIdx.x == 0) {
        n_kept[p] = s_total[0]; n_rings_out[2 * p] = s_total[1]; n_rings_out[2 * p + 1] = s_total[2];
        atomicMax(a.deepest, rounds);
    }
}

// One workgroup per plane: the kept vertices of the input slice, in order, to the output slice
__global__ __launch_bounds__(SP_WG) void sp_emit_kernel(const uint32_t* __restrict__ xy_all, const uint8_t* __restrict__ start_all,
                                                        const int64_t* __restrict__ vertex_offsets, int64_t total,
                                                        const uint8_t* __restrict__ keep_all, const int64_t* __restrict__ out_offsets,
                                                        uint32_t* __restrict__ xy_out, uint8_t* __restrict__ start_out, int64_t total_out,
                                                        int* __restrict__ status) {
    __shared__ int s_part[2][SP_WG / 64], s_total;
    const int p = blockIdx.x;
    const int64_t v0 = vertex_offsets[p], v1 = vertex_offsets[p + 1], o0 = out_offsets[p], o1 = out_offsets[p + 1];
    const bool in_ok = ct_slice_ok(v0, v1, total), out_ok = ct_slice_ok(o0, o1, total_out);
    const int cnt = in_ok ? (int)(v1 - v0) : 0, ocnt = out_ok ? (int)(o1 - o0) : 0;
    auto refuse = [&]() {                                             // the whole workgroup
        for (int t = threadIdx.x; t < ocnt; t += SP_WG) { xy_out[o0 + t] = 0u; start_out[o0 + t] = 0; }
        if (threadIdx.x == 0) atomicOr(status, 1);
    };
    if (!in_ok || !out_ok) { refuse(); return; }
    const uint32_t* xy = xy_all + v0;
    const uint8_t *start = start_all + v0, *keep = keep_all + v0;
    if (threadIdx.x == 0) s_total = 0;
    __syncthreads();
    int kept = 0;
    for (int v = threadIdx.x; v < cnt; v += SP_WG) kept += keep[v] != 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o, 64);
    if ((threadIdx.x & 63) == 0 && kept) atomicAdd(&s_total, kept);
    __syncthreads();
    if (s_total != ocnt) { refuse(); return; }                        // the same for every thread
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int k0 = 0, slab = 0; k0 < cnt; k0 += SP_WG, slab ^= 1) {
        const int k = k0 + threadIdx.x;
        const int x = k < cnt && keep[k] != 0;
        int sum = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(sum, o, 64);
            if (lane >= o) sum += t;
        }
        if (lane == 63) s_part[slab][wave] = sum;
        __syncthreads();
        int before = carry, all = carry;
#pragma unroll
        for (int i = 0; i < SP_WG / 64; ++i) {
            const int t = s_part[slab][i];
            if (i < wave) before += t;
            all += t;
        }
        const int slot = before + sum - x;
        if (x && slot >= 0 && slot < ocnt) {                          // the slot against the slice, before the store
            xy_out[o0 + slot] = xy[k];
            start_out[o0 + slot] = start[k] == 0 ? 0 : k + 1 < cnt ? sp_ring_code(sp_unpack(xy[k]), sp_unpack(xy[k + 1])) : 2;
        }
        carry = all;
    }
}

struct sp_range { const void* at; uint64_t bytes; };

// an output shares a byte with an input or with another output
template <int NI, int NO>
bool sp_meet(const sp_range (&ins)[NI], const sp_range (&outs)[NO]) {
    for (int i = 0; i < NO; ++i) {
        for (int j = 0; j < NI; ++j)
            if (mb_ranges_meet(outs[i].at, outs[i].bytes, ins[j].at, ins[j].bytes)) return true;
        for (int j = i + 1; j < NO; ++j)
            if (mb_ranges_meet(outs[i].at, outs[i].bytes, outs[j].at, outs[j].bytes)) return true;
    }
    return false;
}

bool sp_bad_rings(const int16_t* xy, const uint8_t* ring_start, const int64_t* vertex_offsets, int64_t total, int32_t P) {
    if (!vertex_offsets || total < 0 || P < 1 || P > 65535) return true;
    if (total > 0 && (!xy || !ring_start)) return true;
    return mb_misaligned(4, xy) || mb_misaligned(8, vertex_offsets);
}

bool sp_bad_mark(const int16_t* xy, const uint8_t* ring_start, const int64_t* vertex_offsets, int64_t total, const int32_t* T, int32_t P,
                 int64_t round_vertices, const uint8_t* keep, const int32_t* n_kept, const int32_t* n_rings_out, const int32_t* status,
                 const void* workspace, int64_t workspace_bytes, bool need_ws) {
    if (sp_bad_rings(xy, ring_start, vertex_offsets, total, P) || !T || !n_kept || !n_rings_out || !status || (total > 0 && !keep)) return true;
    if (mb_misaligned(4, T, n_kept, n_rings_out, status)) return true;
    if (round_vertices < 0 || round_vertices > (int64_t)P * CT_MAX_VERTS) return true;
    const uint64_t n = (uint64_t)total, np = (uint64_t)P;
    const sp_range ins[4] = {{xy, 4 * n}, {ring_start, n}, {vertex_offsets, 8 * (np + 1)}, {T, 4 * np}};
    const sp_range outs[4] = {{keep, n}, {n_kept, 4 * np}, {n_rings_out, 8 * np}, {status, 4}};
    if (sp_meet(ins, outs)) return true;
    if (!need_ws) return false;
    if (mb_bad_workspace(workspace, workspace_bytes, 4 * sp_workspace_words(round_vertices))) return true;
    const sp_range ws[1] = {{workspace, (uint64_t)workspace_bytes}};
    const sp_range all[8] = {ins[0], ins[1], ins[2], ins[3], outs[0], outs[1], outs[2], outs[3]};
    return sp_meet(all, ws);
}

bool sp_bad_emit(const int16_t* xy, const uint8_t* ring_start, const int64_t* vertex_offsets, int64_t total, const uint8_t* keep, int32_t P,
                 const int64_t* out_offsets, const int16_t* xy_out, const uint8_t* ring_start_out, int64_t total_out, const int32_t* status,
                 bool keep_is_input) {
    if (sp_bad_rings(xy, ring_start, vertex_offsets, total, P) || !out_offsets || !status || total_out < 0 || (total > 0 && !keep)) return true;
    if (total_out > 0 && (!xy_out || !ring_start_out)) return true;
    if (mb_misaligned(4, xy_out, status) || mb_misaligned(8, out_offsets)) return true;
    const uint64_t n = (uint64_t)total, no = (uint64_t)total_out, np = (uint64_t)P;
    const sp_range ins[5] = {{xy, 4 * n}, {ring_start, n}, {vertex_offsets, 8 * (np + 1)}, {out_offsets, 8 * (np + 1)},
                             {keep_is_input ? keep : nullptr, n}};
    const sp_range outs[3] = {{xy_out, 4 * no}, {ring_start_out, no}, {status, 4}};
    return sp_meet(ins, outs);
}

}  // namespace

extern "C" {

int64_t cvlm_contour_simplify_workspace_bytes(int32_t P, int64_t round_vertices) {
    if (P < 1 || P > 65535 || round_vertices < 0 || round_vertices > (int64_t)P * CT_MAX_VERTS) return CVLM_E_BADARG;
    return 4 * sp_workspace_words(round_vertices);
}

int cvlm_contour_simplify_mark(const int16_t* xy, const uint8_t* ring_start, const int64_t* vertex_offsets, int64_t total, const int32_t* T,
                               int32_t P, int64_t round_vertices, uint8_t* keep, int32_t* n_kept, int32_t* n_rings_out, int32_t* status,
                               void* workspace, int64_t workspace_bytes, void* stream) {
    if (sp_bad_mark(xy, ring_start, vertex_offsets, total, T, P, round_vertices, keep, n_kept, n_rings_out, status, workspace, workspace_bytes,
                    true))
        return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    sp_call a;
    a.xy = (const uint32_t*)xy; a.ring_start = ring_start; a.vertex_offsets = vertex_offsets; a.T = (const int*)T;
    a.total = total; a.round_vertices = round_vertices;
    a.best_num = (u64*)workspace;
    a.rs = (int*)(a.best_num + round_vertices);
    a.seg = a.rs + round_vertices; a.nxt = a.seg + round_vertices; a.best_idx = a.nxt + round_vertices;
    a.deepest = (int*)workspace + sp_tail_word(round_vertices);
    hipLaunchKernelGGL(sp_init_kernel, dim3(1), dim3(256), 0, st, (int*)status, a.deepest);
    CVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(sp_mark_kernel, dim3(P), dim3(SP_WG), 0, st, a, keep, (int*)n_kept, (int*)n_rings_out, (int*)status);
    CVLM_CHECK_LAUNCH();
    return 0;
}

int cvlm_contour_simplify_emit(const int16_t* xy, const uint8_t* ring_start, const int64_t* vertex_offsets, int64_t total, const uint8_t* keep,
                               int32_t P, const int64_t* out_offsets, int16_t* xy_out, uint8_t* ring_start_out, int64_t total_out,
                               int32_t* status, void* stream) {
    if (sp_bad_emit(xy, ring_start, vertex_offsets, total, keep, P, out_offsets, xy_out, ring_start_out, total_out, status, true))
        return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sp_init_kernel, dim3(1), dim3(256), 0, st, (int*)status, (int*)nullptr);
    CVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(sp_emit_kernel, dim3(P), dim3(SP_WG), 0, st, (const uint32_t*)xy, ring_start, vertex_offsets, total, keep, out_offsets,
                       (uint32_t*)xy_out, ring_start_out, total_out, (int*)status);
    CVLM_CHECK_LAUNCH();
    return 0;
}

// The same marks and polygons on host memory: ring after ring, the split as a sequential recursion with an explicit stack of chords
// over simplify_logic.h.  out_offsets == NULL: only the marks and the counts.
int cvlm_debug_contour_simplify_host(const int16_t* xy, const uint8_t* ring_start, const int64_t* vertex_offsets, int64_t total,
                                     const int32_t* T, int32_t P, uint8_t* keep, int32_t* n_kept, int32_t* n_rings_out,
                                     const int64_t* out_offsets, int16_t* xy_out, uint8_t* ring_start_out, int64_t total_out,
                                     int32_t* status) {
    if (sp_bad_mark(xy, ring_start, vertex_offsets, total, T, P, 0, keep, n_kept, n_rings_out, status, nullptr, 0, false))
        return CVLM_E_BADARG;
    if (!out_offsets && (xy_out || ring_start_out)) return CVLM_E_BADARG;
    if (out_offsets) {
        if (sp_bad_emit(xy, ring_start, vertex_offsets, total, keep, P, out_offsets, xy_out, ring_start_out, total_out, status, false))
            return CVLM_E_BADARG;
        const uint64_t np = (uint64_t)P;
        const sp_range ins[1] = {{T, 4 * np}};
        const sp_range outs[5] = {{xy_out, 4 * (uint64_t)total_out}, {ring_start_out, (uint64_t)total_out}, {keep, (uint64_t)total},
                                  {n_kept, 4 * np}, {n_rings_out, 8 * np}};
        const sp_range offs[1] = {{out_offsets, 8 * (np + 1)}};
        const sp_range marks[3] = {outs[2], outs[3], outs[4]};
        if (sp_meet(ins, outs) || sp_meet(offs, marks)) return CVLM_E_BADARG;
    }
    status[0] = 0;
    const uint32_t* in = (const uint32_t*)xy;
    uint32_t* out = (uint32_t*)xy_out;
    std::vector<std::pair<int, int>> stack;
    for (int p = 0; p < P; ++p) {
        n_kept[p] = 0; n_rings_out[2 * p] = n_rings_out[2 * p + 1] = 0;
        const int64_t v0 = vertex_offsets[p], v1 = vertex_offsets[p + 1];
        const bool slice_ok = ct_slice_ok(v0, v1, total);
        const int cnt = slice_ok ? (int)(v1 - v0) : 0;
        if (slice_ok)
            for (int v = 0; v < cnt; ++v) keep[v0 + v] = 0;
        const bool ok = slice_ok && sp_tolerance_ok(T[p]) && (cnt == 0 || ring_start[v0] != 0);
        if (!ok) status[0] |= 1;
        const uint32_t* pts = in + (slice_ok ? v0 : 0);
        const uint8_t* start = ring_start + (slice_ok ? v0 : 0);
        uint8_t* kp = keep + (slice_ok ? v0 : 0);                         // a refused plane's marks are zeros: nothing of it is emitted
        int kept = 0;
        for (int a = 0, b; ok && a < cnt; a = b) {
            for (b = a + 1; b < cnt && start[b] == 0; ++b) {}
            const sp_pt first = sp_unpack(pts[a]);
            uint64_t far = 0;
            int at = a;
            for (int v = a; v < b; ++v) {
                const uint64_t d = sp_d2(sp_unpack(pts[v]), first);
                if (sp_beats(d, v, far, at)) { far = d; at = v; }
            }
            kp[a] = 1;
            int n = 1;
            stack.clear();
            if (at != a) {
                kp[at] = 1; ++n;
                stack.push_back({a, at});
                stack.push_back({at, b});
            }
            while (!stack.empty()) {
                const int i = stack.back().first, j = stack.back().second;
                stack.pop_back();
                const sp_pt pi = sp_unpack(pts[i]), pj = sp_unpack(pts[j == b ? a : j]);
                uint64_t best = 0, L = 1;
                int m = SP_NONE;
                for (int v = i + 1; v < j; ++v) {
                    const uint64_t num = sp_key(pi, pj, sp_unpack(pts[v]), &L);
                    if (sp_beats(num, v, best, m)) { best = num; m = v; }
                }
                if (m == SP_NONE || !sp_keeps(best, L, T[p])) continue;
                kp[m] = 1; ++n;
                stack.push_back({i, m});
                stack.push_back({m, j});
            }
            if (n < 3) {
                for (int v = a; v < b; ++v) kp[v] = 0;
                continue;
            }
            kept += n;
            ++n_rings_out[2 * p + (a + 1 < cnt && sp_ring_code(first, sp_unpack(pts[a + 1])) == 1 ? 0 : 1)];
        }
        n_kept[p] = kept;
        if (!out_offsets) continue;
        const int64_t o0 = out_offsets[p], o1 = out_offsets[p + 1];
        const bool out_ok = ct_slice_ok(o0, o1, total_out);
        const int ocnt = out_ok ? (int)(o1 - o0) : 0;
        if (!slice_ok || !out_ok || kept != ocnt) {
            status[0] |= 1;
            for (int t = 0; t < ocnt; ++t) { out[o0 + t] = 0u; ring_start_out[o0 + t] = 0; }
            continue;
        }
        int slot = 0;
        for (int v = 0; v < cnt; ++v) {
            if (!kp[v]) continue;
            out[o0 + slot] = pts[v];
            ring_start_out[o0 + slot] = start[v] == 0 ? 0 : v + 1 < cnt ? sp_ring_code(sp_unpack(pts[v]), sp_unpack(pts[v + 1])) : 2;
            ++slot;
        }
    }
    return 0;
}

}  // extern "C"
