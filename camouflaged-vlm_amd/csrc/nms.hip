// Mask NMS on the device (include/cvlm.h: cvlm_mask_nms_inter, cvlm_mask_nms): the duplicate instances of an image --
// one object found under several class hypotheses -- dropped or decayed without a read of the device.  Two entries of two launches.
//
// cvlm_mask_nms_inter  nm_inter_init_kernel: status = 0, every inter = -1 (what no accepted group owns stays refused).
//                      nm_inter_kernel: workgroup (g, y) of four waves takes the pairs 4 y + wave, + 4 gridDim.y, ... of group g's
//                      triangle; ONE WAVE PER PAIR.  The wave checks the pair, intersects the two boxes, and its 64 lanes stride over
//                      the words of that window alone: whole-word loads of both planes, the first and last word column masked to the
//                      window's pixel columns, a shuffle reduction, one plain store by lane 0.  No atomic on inter, no LDS; boxes that
//                      do not meet store 0 without a load of either plane.  Integer sums: the same bytes whatever the schedule.
// cvlm_mask_nms        nm_fill_kernel: every output to "named by no accepted group".
//                      nm_nms_kernel: one workgroup per group.  (1) rows, scores, areas and categories to LDS; (2) stable rank by
//                      counting predecessors (mt_precedes), order out; (3) greedy: the ranks in turn, every thread testing the later
//                      ranks against the kept one, a barrier per KEPT instance -- or Matrix NMS: thread per instance, c_i = max m
//                      over the ranks above i into LDS, then the minimum over the ranks above j.  The triangle is read from global
//                      memory.  No workgroup waits for another.
// Both kernels decide a group's refusal the same way for every thread (nm_group_span, then a workgroup OR over the members).
#include <vector>

#include "../../include/cvlm.h"
#include "common.h"
#include "nms_logic.h"

namespace {

constexpr int NM_THREADS = 256;
// Threads that share a pair in nm_inter_kernel: 64, a wave (the product), or 256, the whole workgroup -- the mapping DESIGN.md §30
// measured against it, built with -DCVLM_NMS_PAIR_THREADS=256 into a probe library (tools/bench_nms.py --inter-only)
#ifndef CVLM_NMS_PAIR_THREADS
#define CVLM_NMS_PAIR_THREADS 64
#endif
constexpr int NM_PAIR_THREADS = CVLM_NMS_PAIR_THREADS;
static_assert(NM_PAIR_THREADS == CVLM_WAVE || NM_PAIR_THREADS == NM_THREADS, "a wave or the workgroup");
constexpr int NM_PAIRS = NM_THREADS / NM_PAIR_THREADS;   // pairs a workgroup of nm_inter_kernel has in flight

__global__ __launch_bounds__(256) void nm_inter_init_kernel(int* __restrict__ inter, int64_t N, int* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) status[0] = 0;
    if (i < N) inter[i] = -1;
}

// The group's verdict, the same in every thread of the workgroup: the tables, then every member inside [0, Q)
__device__ __forceinline__ bool nm_group_ok_block(const int* __restrict__ group_off, const int* __restrict__ member,
                                                  const int64_t* __restrict__ pair_off, int g, int Q, int64_t N, nm_group& q) {
    if (!nm_group_span(group_off, pair_off, g, Q, N, q)) return false;
    int bad = 0;
    for (int k = threadIdx.x; k < q.D; k += NM_THREADS) bad |= nm_member_ok(member[q.m0 + k], Q) ? 0 : 1;
    return __syncthreads_or(bad) == 0;
}

__global__ __launch_bounds__(NM_THREADS) void nm_inter_kernel(const uint8_t* __restrict__ bits, int64_t nbytes, const int64_t* __restrict__ offsets,
                                                              const int* __restrict__ dims, const int* __restrict__ area,
                                                              const int* __restrict__ box, int Q, const int* __restrict__ group_off,
                                                              const int* __restrict__ member, const int64_t* __restrict__ pair_off, int64_t N,
                                                              int* __restrict__ inter, int* __restrict__ status) {
    nm_group q;
    if (!nm_group_ok_block(group_off, member, pair_off, blockIdx.x, Q, N, q)) {
        if (blockIdx.y == 0 && threadIdx.x == 0) atomicOr(status, NM_GROUP_REFUSED);
        return;
    }
    const int slot = threadIdx.x / NM_PAIR_THREADS, lane = threadIdx.x % NM_PAIR_THREADS;
    const int64_t T = (int64_t)q.D * (q.D - 1) / 2;
    for (int64_t t = (int64_t)blockIdx.y * NM_PAIRS + slot; t < T; t += (int64_t)gridDim.y * NM_PAIRS) {
        int i, j;
        nm_pair_of(t, q.D, i, j);
        const int a = member[q.m0 + i], b = member[q.m0 + j];
        if (!nm_pair_ok(a, b, dims, offsets, nbytes, box)) {          // the same for every thread of the pair
            if (lane == 0) { inter[q.p0 + t] = -1; atomicOr(status, NM_PAIR_REFUSED); }
            continue;
        }
        const nm_window v = nm_window_of(box + 4 * a, area[a], box + 4 * b, area[b]);
        int n = 0;
        if (v.rows) {
            const int ws = sz_words_per_row(dims[2 * a + 1]);
            const uint32_t* pa = (const uint32_t*)(bits + offsets[a]) + (int64_t)v.y0 * ws + v.c0;
            const uint32_t* pb = (const uint32_t*)(bits + offsets[b]) + (int64_t)v.y0 * ws + v.c0;
            const int words = v.rows * v.cols;                        // <= 2^23
            const int dr = NM_PAIR_THREADS / v.cols, dc = NM_PAIR_THREADS - dr * v.cols;    // the word NM_PAIR_THREADS on: one division per pair
            int r = lane / v.cols, c = lane - r * v.cols;
            for (int k = lane; k < words; k += NM_PAIR_THREADS) {
                const int64_t at = (int64_t)r * ws + c;
                n += nm_word(pa[at], pb[at], v.c0 + c, v.x0, v.x1);
                r += dr; c += dc;
                if (c >= v.cols) { c -= v.cols; ++r; }
            }
        }
        if constexpr (NM_PAIR_THREADS == CVLM_WAVE) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
        } else {                                                      // the probe: the pair is the workgroup's, so every thread is here
            int sum[1] = {n};
            mb_block_sum(sum);
            n = sum[0];
            __syncthreads();                                          // the sum's LDS is free for the next pair
        }
        if (lane == 0) inter[q.p0 + t] = n;
    }
}

__global__ __launch_bounds__(256) void nm_fill_kernel(int Q, int G, int* __restrict__ order, uint8_t* __restrict__ keep, int* __restrict__ by,
                                                      float* __restrict__ decay, int* __restrict__ n_keep, int* __restrict__ status) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) status[0] = 0;
    if (i < Q) { order[i] = -1; keep[i] = 0; by[i] = -1; decay[i] = 0.0f; }
    if (i < G) n_keep[i] = 0;
}

// m of the group's instances x and y (places in member order) from the triangle
__device__ __forceinline__ double nm_measure_at(const int* __restrict__ tri, int D, int x, int y, const int* ar, const int* ct, int measure) {
    const int lo = x < y ? x : y, hi = x < y ? y : x;
    return nm_measure(tri[nm_pair_at(lo, hi, D)], ar[x], ar[y], measure, ct[x] == ct[y]);
}

__global__ __launch_bounds__(NM_THREADS) void nm_nms_kernel(const int* __restrict__ group_off, const int* __restrict__ member,
                                                            const int64_t* __restrict__ pair_off, const int* __restrict__ inter, int64_t N,
                                                            const int* __restrict__ area, const float* __restrict__ score,
                                                            const int* __restrict__ category, int Q, int measure, int method, double thr,
                                                            double sigma, int* __restrict__ order, uint8_t* __restrict__ keep,
                                                            int* __restrict__ by, float* __restrict__ decay, int* __restrict__ n_keep,
                                                            int* __restrict__ status) {
    __shared__ float sc[NM_CAP];
    __shared__ int row[NM_CAP], ar[NM_CAP], ct[NM_CAP], ord[NM_CAP];
    __shared__ double cmax[NM_CAP];                                   // Matrix NMS: c of the instance of each RANK
    __shared__ uint8_t gone[NM_CAP];                                  // greedy: suppressed
    const int tid = threadIdx.x, g = blockIdx.x;
    nm_group q;
    if (!nm_group_ok_block(group_off, member, pair_off, g, Q, N, q)) {
        if (tid == 0) atomicOr(status, NM_GROUP_REFUSED);
        return;
    }
    const int D = q.D;
    const int* tri = inter + q.p0;                                    // D < 2: never read
    for (int k = tid; k < D; k += NM_THREADS) {
        const int r = member[q.m0 + k];
        row[k] = r; sc[k] = score[r]; ar[k] = area[r]; ct[k] = category ? category[r] : 0; gone[k] = 0;
    }
    __syncthreads();
    for (int i = tid; i < D; i += NM_THREADS) {
        const float si = sc[i];
        int r = 0;
        for (int j = 0; j < D; ++j) r += mt_precedes(sc[j], j, si, i) ? 1 : 0;
        ord[r] = i;
        order[q.m0 + r] = row[i];
    }
    __syncthreads();
    int n[1] = {0};
    if (method == NM_GREEDY) {
        for (int r = 0; r < D; ++r) {
            const int i = ord[r];
            if (gone[i] || ar[i] < 1) continue;                       // LDS as the last barrier left it: the same for every thread
            for (int s = r + 1 + tid; s < D; s += NM_THREADS) {
                const int j = ord[s];
                if (!gone[j] && nm_measure_at(tri, D, i, j, ar, ct, measure) > thr) { gone[j] = 1; by[row[j]] = row[i]; }
            }
            __syncthreads();
        }
        for (int k = tid; k < D; k += NM_THREADS) {
            const bool kept = !gone[k] && ar[k] >= 1;
            keep[row[k]] = kept ? 1 : 0;
            decay[row[k]] = kept ? 1.0f : 0.0f;
            n[0] += kept ? 1 : 0;
        }
    } else {
        for (int s = tid; s < D; s += NM_THREADS) {
            const int i = ord[s];
            double c = 0.0;
            for (int t = 0; t < s; ++t) {
                const double m = nm_clamp(nm_measure_at(tri, D, ord[t], i, ar, ct, measure));
                c = m > c ? m : c;
            }
            cmax[s] = c;
        }
        __syncthreads();
        for (int s = tid; s < D; s += NM_THREADS) {
            const int j = ord[s];
            double best = method == NM_LINEAR ? 1.0 : 0.0;            // linear: the least term; gaussian: the largest argument
            for (int t = 0; t < s; ++t) {
                const double m = nm_clamp(nm_measure_at(tri, D, ord[t], j, ar, ct, measure));
                if (method == NM_LINEAR) {
                    const double v = nm_linear_term(m, cmax[t]);
                    best = v < best ? v : best;
                } else {
                    const double v = nm_gauss_arg(m, cmax[t]);
                    best = v > best ? v : best;
                }
            }
            const bool kept = ar[j] >= 1;
            keep[row[j]] = kept ? 1 : 0;
            decay[row[j]] = (float)(method == NM_LINEAR ? best : nm_gauss_decay(sigma, best));
            n[0] += kept ? 1 : 0;
        }
    }
    if (mb_block_sum(n)) n_keep[g] = n[0];
}

struct nm_range { const void* p; uint64_t bytes; };
// some output shares a byte with an input or with another output
template <size_t NI, size_t NO>
bool nm_outputs_meet(const nm_range (&in)[NI], const nm_range (&out)[NO]) {
    for (size_t o = 0; o < NO; ++o) {
        for (size_t i = 0; i < NI; ++i)
            if (mb_ranges_meet(out[o].p, out[o].bytes, in[i].p, in[i].bytes)) return true;
        for (size_t k = o + 1; k < NO; ++k)
            if (mb_ranges_meet(out[o].p, out[o].bytes, out[k].p, out[k].bytes)) return true;
    }
    return false;
}

bool nm_bad_counts(int32_t Q, int32_t G, int64_t N) { return Q < 1 || Q > NM_MAX_ROWS || G < 1 || G > NM_MAX_ROWS || N < 0 || N > NM_MAX_PAIRS; }

// what both intersection entries refuse
bool nm_inter_bad(const uint8_t* bits, int64_t n_bytes, const int64_t* offsets, const int32_t* dims, const int32_t* area, const int32_t* box,
                  int32_t Q, const int32_t* group_offsets, const int32_t* member, const int64_t* pair_offsets, int32_t G, int64_t N,
                  const int32_t* inter, const int32_t* status) {
    if (!bits || !offsets || !dims || !area || !box || !group_offsets || !member || !pair_offsets || !status || (N > 0 && !inter)) return true;
    if (nm_bad_counts(Q, G, N) || n_bytes < 4) return true;
    if (mb_misaligned(4, bits, dims, area, box, group_offsets, member, inter, status) || mb_misaligned(8, offsets, pair_offsets)) return true;
    const uint64_t q = (uint64_t)Q, g = (uint64_t)G;
    const nm_range in[] = {{bits, (uint64_t)n_bytes}, {offsets, 8 * (q + 1)}, {dims, 8 * q}, {area, 4 * q}, {box, 16 * q},
                           {group_offsets, 4 * (g + 1)}, {member, 4 * q}, {pair_offsets, 8 * (g + 1)}};
    const nm_range out[] = {{inter, 4 * (uint64_t)N}, {status, 4}};
    return nm_outputs_meet(in, out);
}

// what both NMS entries refuse; params: {thr, sigma} on the host
bool nm_bad(const int32_t* group_offsets, const int32_t* member, const int64_t* pair_offsets, int32_t G, const int32_t* inter, int64_t N,
            const int32_t* area, const float* score, const int32_t* category, int32_t Q, int32_t measure, int32_t method, const double* params,
            const int32_t* order, const uint8_t* keep, const int32_t* by, const float* decay, const int32_t* n_keep, const int32_t* status) {
    if (!group_offsets || !member || !pair_offsets || !area || !score || !params || !order || !keep || !by || !decay || !n_keep || !status ||
        (N > 0 && !inter))
        return true;
    if (nm_bad_counts(Q, G, N)) return true;
    if (mb_misaligned(4, group_offsets, member, inter, area, score, category, order, by, decay, n_keep, status) ||
        mb_misaligned(8, pair_offsets, params))
        return true;
    if (measure != NM_IOU && measure != NM_MIN) return true;
    if (method != NM_GREEDY && method != NM_LINEAR && method != NM_GAUSS) return true;
    if (!(params[0] >= 0.0 && params[0] <= 1.0)) return true;        // a NaN fails both
    if (method == NM_GAUSS && !(isfinite(params[1]) && params[1] > 0.0)) return true;
    const uint64_t q = (uint64_t)Q, g = (uint64_t)G;
    const nm_range in[] = {{group_offsets, 4 * (g + 1)}, {member, 4 * q}, {pair_offsets, 8 * (g + 1)}, {inter, 4 * (uint64_t)N},
                           {area, 4 * q},                {score, 4 * q},  {category, 4 * q}};
    const nm_range out[] = {{order, 4 * q}, {keep, q}, {by, 4 * q}, {decay, 4 * q}, {n_keep, 4 * g}, {status, 4}};
    return nm_outputs_meet(in, out);
}

// the host's verdict on a group: nm_group_ok_block run by one thread
bool nm_group_ok_host(const int32_t* group_offsets, const int32_t* member, const int64_t* pair_offsets, int g, int Q, int64_t N, nm_group& q) {
    if (!nm_group_span(group_offsets, pair_offsets, g, Q, N, q)) return false;
    for (int k = 0; k < q.D; ++k)
        if (!nm_member_ok(member[q.m0 + k], Q)) return false;
    return true;
}

}  // namespace

extern "C" {

int cvlm_mask_nms_inter(const uint8_t* bits, int64_t n_bytes, const int64_t* offsets, const int32_t* dims, const int32_t* area,
                        const int32_t* box, int32_t Q, const int32_t* group_offsets, const int32_t* member, const int64_t* pair_offsets,
                        int32_t G, int64_t N, int32_t* inter, int32_t* status, void* stream) {
    if (nm_inter_bad(bits, n_bytes, offsets, dims, area, box, Q, group_offsets, member, pair_offsets, G, N, inter, status)) return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    // workgroups per group: what the average group needs to give every wave one pair, larger groups go in strides
    const int64_t per_group = (N + (int64_t)G * NM_PAIRS - 1) / ((int64_t)G * NM_PAIRS);
    const int64_t cap = 4096 / NM_PAIRS;
    const int gy = (int)(per_group < 1 ? 1 : (per_group > cap ? cap : per_group));
    hipLaunchKernelGGL(nm_inter_init_kernel, dim3((unsigned)((N + 256) / 256)), dim3(256), 0, st, (int*)inter, N, (int*)status);
    CVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(nm_inter_kernel, dim3(G, gy), dim3(NM_THREADS), 0, st, bits, n_bytes, offsets, (const int*)dims, (const int*)area,
                       (const int*)box, (int)Q, (const int*)group_offsets, (const int*)member, pair_offsets, N, (int*)inter, (int*)status);
    CVLM_CHECK_LAUNCH();
    return 0;
}

// The same functions on host memory, group by group and pair by pair
int cvlm_debug_mask_nms_inter_host(const uint8_t* bits, int64_t n_bytes, const int64_t* offsets, const int32_t* dims, const int32_t* area,
                                   const int32_t* box, int32_t Q, const int32_t* group_offsets, const int32_t* member,
                                   const int64_t* pair_offsets, int32_t G, int64_t N, int32_t* inter, int32_t* status) {
    if (nm_inter_bad(bits, n_bytes, offsets, dims, area, box, Q, group_offsets, member, pair_offsets, G, N, inter, status)) return CVLM_E_BADARG;
    status[0] = 0;
    for (int64_t i = 0; i < N; ++i) inter[i] = -1;
    for (int g = 0; g < G; ++g) {
        nm_group q;
        if (!nm_group_ok_host(group_offsets, member, pair_offsets, g, Q, N, q)) {
            status[0] |= NM_GROUP_REFUSED;
            continue;
        }
        const int64_t T = (int64_t)q.D * (q.D - 1) / 2;
        for (int64_t t = 0; t < T; ++t) {
            int i, j;
            nm_pair_of(t, q.D, i, j);
            const int a = member[q.m0 + i], b = member[q.m0 + j];
            if (!nm_pair_ok(a, b, dims, offsets, n_bytes, box)) {
                inter[q.p0 + t] = -1;
                status[0] |= NM_PAIR_REFUSED;
                continue;
            }
            const nm_window v = nm_window_of(box + 4 * a, area[a], box + 4 * b, area[b]);
            int n = 0;
            if (v.rows) {
                const int ws = sz_words_per_row(dims[2 * a + 1]);
                const uint32_t* pa = (const uint32_t*)(bits + offsets[a]) + (int64_t)v.y0 * ws + v.c0;
                const uint32_t* pb = (const uint32_t*)(bits + offsets[b]) + (int64_t)v.y0 * ws + v.c0;
                for (int k = 0; k < v.rows * v.cols; ++k) {
                    const int r = k / v.cols, c = k - r * v.cols;
                    const int64_t at = (int64_t)r * ws + c;
                    n += nm_word(pa[at], pb[at], v.c0 + c, v.x0, v.x1);
                }
            }
            inter[q.p0 + t] = n;
        }
    }
    return 0;
}

int cvlm_mask_nms(const int32_t* group_offsets, const int32_t* member, const int64_t* pair_offsets, int32_t G, const int32_t* inter, int64_t N,
                  const int32_t* area, const float* score, const int32_t* category, int32_t Q, int32_t measure, int32_t method,
                  const double* params, int32_t* order, uint8_t* keep, int32_t* by, float* decay, int32_t* n_keep, int32_t* status,
                  void* stream) {
    if (nm_bad(group_offsets, member, pair_offsets, G, inter, N, area, score, category, Q, measure, method, params, order, keep, by, decay,
               n_keep, status))
        return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int cells = Q > G ? Q : G;
    hipLaunchKernelGGL(nm_fill_kernel, dim3((cells + 255) / 256), dim3(256), 0, st, (int)Q, (int)G, (int*)order, keep, (int*)by, decay,
                       (int*)n_keep, (int*)status);
    CVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(nm_nms_kernel, dim3(G), dim3(NM_THREADS), 0, st, (const int*)group_offsets, (const int*)member, pair_offsets,
                       (const int*)inter, N, (const int*)area, score, (const int*)category, (int)Q, (int)measure, (int)method, params[0],
                       params[1], (int*)order, keep, (int*)by, decay, (int*)n_keep, (int*)status);
    CVLM_CHECK_LAUNCH();
    return 0;
}

// The same functions on host memory, group by group, the kernel's steps in its order
int cvlm_debug_mask_nms_host(const int32_t* group_offsets, const int32_t* member, const int64_t* pair_offsets, int32_t G, const int32_t* inter,
                             int64_t N, const int32_t* area, const float* score, const int32_t* category, int32_t Q, int32_t measure,
                             int32_t method, const double* params, int32_t* order, uint8_t* keep, int32_t* by, float* decay, int32_t* n_keep,
                             int32_t* status) {
    if (nm_bad(group_offsets, member, pair_offsets, G, inter, N, area, score, category, Q, measure, method, params, order, keep, by, decay,
               n_keep, status))
        return CVLM_E_BADARG;
    const double thr = params[0], sigma = params[1];
    status[0] = 0;
    for (int i = 0; i < Q; ++i) { order[i] = -1; keep[i] = 0; by[i] = -1; decay[i] = 0.0f; }
    for (int g = 0; g < G; ++g) n_keep[g] = 0;
    std::vector<int> row, ar, ct, ord;
    std::vector<float> sc;
    std::vector<double> cmax;
    std::vector<uint8_t> gone;
    for (int g = 0; g < G; ++g) {
        nm_group q;
        if (!nm_group_ok_host(group_offsets, member, pair_offsets, g, Q, N, q)) {
            status[0] |= NM_GROUP_REFUSED;
            continue;
        }
        const int D = q.D;
        const int* tri = inter + q.p0;
        row.assign((size_t)D, 0); ar.assign((size_t)D, 0); ct.assign((size_t)D, 0); ord.assign((size_t)D, 0);
        sc.assign((size_t)D, 0.0f); cmax.assign((size_t)D, 0.0); gone.assign((size_t)D, 0);
        for (int k = 0; k < D; ++k) {
            const int r = member[q.m0 + k];
            row[(size_t)k] = r; sc[(size_t)k] = score[r]; ar[(size_t)k] = area[r]; ct[(size_t)k] = category ? category[r] : 0;
        }
        for (int i = 0; i < D; ++i) {
            int r = 0;
            for (int j = 0; j < D; ++j) r += mt_precedes(sc[(size_t)j], j, sc[(size_t)i], i) ? 1 : 0;
            ord[(size_t)r] = i;
            order[q.m0 + r] = row[(size_t)i];
        }
        auto m_of = [&](int x, int y) {
            const int lo = x < y ? x : y, hi = x < y ? y : x;
            return nm_measure(tri[nm_pair_at(lo, hi, D)], ar[(size_t)x], ar[(size_t)y], measure, ct[(size_t)x] == ct[(size_t)y]);
        };
        int n = 0;
        if (method == NM_GREEDY) {
            for (int r = 0; r < D; ++r) {
                const int i = ord[(size_t)r];
                if (gone[(size_t)i] || ar[(size_t)i] < 1) continue;
                for (int s = r + 1; s < D; ++s) {
                    const int j = ord[(size_t)s];
                    if (!gone[(size_t)j] && m_of(i, j) > thr) { gone[(size_t)j] = 1; by[row[(size_t)j]] = row[(size_t)i]; }
                }
            }
            for (int k = 0; k < D; ++k) {
                const bool kept = !gone[(size_t)k] && ar[(size_t)k] >= 1;
                keep[row[(size_t)k]] = kept ? 1 : 0;
                decay[row[(size_t)k]] = kept ? 1.0f : 0.0f;
                n += kept ? 1 : 0;
            }
        } else {
            for (int s = 0; s < D; ++s) {
                double c = 0.0;
                for (int t = 0; t < s; ++t) {
                    const double m = nm_clamp(m_of(ord[(size_t)t], ord[(size_t)s]));
                    c = m > c ? m : c;
                }
                cmax[(size_t)s] = c;
            }
            for (int s = 0; s < D; ++s) {
                const int j = ord[(size_t)s];
                double best = method == NM_LINEAR ? 1.0 : 0.0;
                for (int t = 0; t < s; ++t) {
                    const double m = nm_clamp(m_of(ord[(size_t)t], j));
                    if (method == NM_LINEAR) {
                        const double v = nm_linear_term(m, cmax[(size_t)t]);
                        best = v < best ? v : best;
                    } else {
                        const double v = nm_gauss_arg(m, cmax[(size_t)t]);
                        best = v > best ? v : best;
                    }
                }
                const bool kept = ar[(size_t)j] >= 1;
                keep[row[(size_t)j]] = kept ? 1 : 0;
                decay[row[(size_t)j]] = (float)(method == NM_LINEAR ? best : nm_gauss_decay(sigma, best));
                n += kept ? 1 : 0;
            }
        }
        n_keep[g] = n;
    }
    return 0;
}

}  // extern "C"
