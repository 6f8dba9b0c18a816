// Distance maps of sized planes and directed surface totals (include/cvlm.h: cvlm_mask_distance_sized, cvlm_mask_surface_totals;
// DESIGN.md §27): for every pixel of a plane the squared distance to its nearest set pixel, exact in int32, and for pairs (A, B) the
// counts and sums of B's map over the set pixels of A from which the Hausdorff distance, ASSD, NSD and the boundary F-measure follow.
// The per-thread logic -- the chunk of a row, the two gaps of a pixel, the column search, one pixel's share of the totals -- is
// distance_logic.h, shared with the sequential host entries at the end of this file.
//
// cvlm_mask_distance_sized, three launches: dt_init_kernel (status), then through the caller's workspace (f, a uint16 per pixel)
//   dt_rows_kernel: a wave per row.  The lanes load 64 words at once; the wave walks their 32 chunks forwards with the carried gap
//                   towards the row's start and parks each pixel's gap in f, then walks them backwards with the carried gap towards
//                   the row's end, and each lane replaces what it parked itself by the smaller of the two, cut at the reach;
//   dt_cols_kernel: a wave per (row, 64 pixel columns), a thread per pixel, the lanes on consecutive x: every read of f(y +- k, x) is
//                   one coalesced row segment.  The search runs outwards from k = 0 and ends per lane; D2 goes out as one int32.
// cvlm_mask_surface_totals, three launches: dt_totals_init_kernel, dt_totals_kernel (a thread per word of A: popcount, then a walk
// over its set bits against B's map; sums per workgroup; at most one integer atomic per integer output, workgroup and pair; sum_d as
// one partial per workgroup and pair in the workspace), dt_totals_finalize_kernel (a thread per pair adds its partials in order).
// No workgroup waits for another; a refused plane or pair is never read.
#include <algorithm>
#include <cstring>

#include "../../include/cvlm.h"
#include "common.h"
#include "distance_logic.h"

namespace {

__global__ void dt_init_kernel(int* __restrict__ status) { status[0] = 0; }

// Plane blockIdx.y; wave v of workgroup g takes the rows 4 g + v, + 4 gridDim.x, ...  A row has at most 512 words: 8 loads of 64.
__global__ __launch_bounds__(256) void dt_rows_kernel(const uint8_t* __restrict__ bits, int64_t nbytes, const int64_t* __restrict__ offsets,
                                                      const int* __restrict__ dims, const int* __restrict__ reach,
                                                      const int64_t* __restrict__ pix_offsets, int64_t n_pix, uint16_t* workspace) {
    const int p = blockIdx.y;
    const int h = dims[2 * p], w = dims[2 * p + 1], R = reach[p];
    const int64_t off = offsets[p], end = offsets[p + 1], poff = pix_offsets[p], pend = pix_offsets[p + 1];
    if (!sz_plane_ok(h, w, off, end, nbytes) || !dt_reach_ok(R) || !dt_slice_ok(h, w, poff, pend, n_pix)) return;    // the same for every thread
    if (blockIdx.x * 4 >= h) return;
    const int ws = sz_words_per_row(w), chunks = (ws + 1) >> 1, nblk = (chunks + 31) >> 5;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t* src = (const uint32_t*)(bits + off);
    uint16_t* f = workspace + poff;
    for (int y = blockIdx.x * 4 + wave; y < h; y += gridDim.x * 4) {
        const uint32_t* row = src + (int64_t)y * ws;
        uint16_t* frow = f + (int64_t)y * w;
        int carry = DT_NONE;
        for (int b = 0; b < nblk; ++b) {
            const int c = 64 * b + lane;
            const uint32_t v = c < ws ? cc_unpack(row[c]) : 0u;
            const int nch = min(32, chunks - 32 * b);
            for (int k = 0; k < nch; ++k) {
                const int x0 = 64 * (32 * b + k);
                const uint64_t m = dt_chunk(__shfl(v, 2 * k, 64), __shfl(v, 2 * k + 1, 64), x0, w);
                if (x0 + lane < w) frow[x0 + lane] = dt_row_park(dt_gap_back(m, lane, carry));
                carry = dt_gap_back(m, 63, carry);
            }
        }
        carry = DT_NONE;
        for (int b = nblk - 1; b >= 0; --b) {
            const int c = 64 * b + lane;
            const uint32_t v = c < ws ? cc_unpack(row[c]) : 0u;
            const int nch = min(32, chunks - 32 * b);
            for (int k = nch - 1; k >= 0; --k) {
                const int x0 = 64 * (32 * b + k);
                const uint64_t m = dt_chunk(__shfl(v, 2 * k, 64), __shfl(v, 2 * k + 1, 64), x0, w);
                if (x0 + lane < w) frow[x0 + lane] = dt_row_value(frow[x0 + lane], dt_gap_fwd(m, lane, carry), R);    // parked by this lane
                carry = dt_gap_fwd(m, 0, carry);
            }
        }
    }
}

// Plane blockIdx.y.  A UNIT is (64 pixel columns, row): ceil(w / 64) column strips times h rows, the rows of a strip consecutive; wave v
// of workgroup g takes the units 4 g + v, + 4 gridDim.x, ... -- the four waves of a workgroup search neighbouring rows of one strip.
__global__ __launch_bounds__(256) void dt_cols_kernel(int64_t nbytes, const int64_t* __restrict__ offsets, const int* __restrict__ dims,
                                                      const int* __restrict__ reach, const int64_t* __restrict__ pix_offsets, int64_t n_pix,
                                                      const uint16_t* __restrict__ workspace, int32_t* __restrict__ out_d2,
                                                      int* __restrict__ status) {
    const int p = blockIdx.y;
    const int h = dims[2 * p], w = dims[2 * p + 1], R = reach[p];
    const int64_t off = offsets[p], end = offsets[p + 1], poff = pix_offsets[p], pend = pix_offsets[p + 1];
    if (!sz_plane_ok(h, w, off, end, nbytes) || !dt_reach_ok(R) || !dt_slice_ok(h, w, poff, pend, n_pix)) {          // the same for every thread
        if (dt_slice_sound(poff, pend, n_pix))
            for (int64_t i = poff + (int64_t)blockIdx.x * 256 + threadIdx.x; i < pend; i += (int64_t)gridDim.x * 256) out_d2[i] = DT_FAR;
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, 1);
        return;
    }
    const int strips = (w + 63) >> 6;
    const int64_t units = (int64_t)strips * h;                        // <= 256 * 16384
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint16_t* f = workspace + poff;
    int32_t* dst = out_d2 + poff;
    for (int64_t u = (int64_t)blockIdx.x * 4 + wave; u < units; u += (int64_t)gridDim.x * 4) {
        const int s = (int)(u / h), y = (int)(u - (int64_t)s * h), x = 64 * s + lane;
        if (x < w) dst[(int64_t)y * w + x] = dt_column(f, h, w, y, x, R);
    }
}

__global__ __launch_bounds__(256) void dt_totals_init_kernel(int N, int T, int* __restrict__ n, int* __restrict__ far,
                                                             int* __restrict__ within, int* __restrict__ max_d2,
                                                             long long* __restrict__ sum_d2, int* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) status[0] = 0;
    if (i >= N) return;
    n[i] = 0;
    far[i] = 0;
    max_d2[i] = -1;
    sum_d2[i] = 0;
    for (int k = 0; k < T; ++k) within[i * T + k] = 0;
}

// the rest of a thread's share summed over a 256-thread workgroup in a fixed order: thread 0 holds the results behind the call
__device__ __forceinline__ void dt_block_rest(int& mx, int64_t& s2, double& sd) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mx = max(mx, __shfl_xor(mx, o, 64));
        s2 += __shfl_xor(s2, o, 64);
        sd += __shfl_xor(sd, o, 64);
    }
    __shared__ int r_mx[4];
    __shared__ int64_t r_s2[4];
    __shared__ double r_sd[4];
    if ((threadIdx.x & 63) == 0) {
        r_mx[threadIdx.x >> 6] = mx;
        r_s2[threadIdx.x >> 6] = s2;
        r_sd[threadIdx.x >> 6] = sd;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    mx = max(max(r_mx[0], r_mx[1]), max(r_mx[2], r_mx[3]));
    s2 = r_s2[0] + r_s2[1] + r_s2[2] + r_s2[3];
    sd = ((r_sd[0] + r_sd[1]) + r_sd[2]) + r_sd[3];
}

// Pairs blockIdx.y, + gridDim.y, ...; the workgroups blockIdx.x of a pair share the words of its plane of A.  partial: [N][gridDim.x].
__global__ __launch_bounds__(256) void dt_totals_kernel(const uint8_t* __restrict__ a_bits, int64_t a_bytes, const int64_t* __restrict__ a_offsets,
                                                        const int* __restrict__ a_dims, int Pa, const int32_t* __restrict__ b_d2,
                                                        const int64_t* __restrict__ b_pix_offsets, int64_t b_n_pix,
                                                        const int* __restrict__ b_dims, int Pb, const int* __restrict__ pairs, int N,
                                                        const int* __restrict__ radii, int T, double* __restrict__ partial,
                                                        int* __restrict__ n, int* __restrict__ far, int* __restrict__ within,
                                                        int* __restrict__ max_d2, unsigned long long* __restrict__ sum_d2,
                                                        int* __restrict__ status) {
    for (int64_t pair = blockIdx.y; pair < N; pair += gridDim.y) {
        const int ia = pairs[2 * pair], ib = pairs[2 * pair + 1];
        const int* rad = radii + pair * T;
        double* part = partial + pair * gridDim.x + blockIdx.x;
        if (!dt_pair_ok(ia, ib, Pa, Pb, a_dims, a_offsets, a_bytes, b_dims, b_pix_offsets, b_n_pix, rad, T)) {        // the same for every thread
            if (threadIdx.x == 0) {
                part[0] = 0.0;
                if (blockIdx.x == 0) {                                // nobody else writes a refused pair's outputs
                    n[pair] = far[pair] = max_d2[pair] = -1;
                    sum_d2[pair] = ~0ull;
                    for (int k = 0; k < T; ++k) within[pair * T + k] = -1;
                    atomicOr(status, 1);
                }
            }
            continue;
        }
        const int h = a_dims[2 * ia], w = a_dims[2 * ia + 1], ws = sz_words_per_row(w);
        const uint32_t* src = (const uint32_t*)(a_bits + a_offsets[ia]);
        const int32_t* map = b_d2 + b_pix_offsets[ib];
        int64_t r2[DT_MAX_T];
#pragma unroll
        for (int k = 0; k < DT_MAX_T; ++k) r2[k] = k < T ? (int64_t)rad[k] * rad[k] : -1;
        dt_totals t;
        const int64_t words = (int64_t)h * ws;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) {
            const int y = (int)(i / ws), c = (int)(i - (int64_t)y * ws);
            uint32_t m = cc_unpack(src[i]) & dt_word_mask(c, w);
            const int32_t* mrow = map + (int64_t)y * w + 32 * c;
            while (m) {
                dt_pixel(t, mrow[__builtin_ctz(m)], r2);
                m &= m - 1;
            }
        }
        int v[2 + DT_MAX_T];
        v[0] = t.n;
        v[1] = t.far;
#pragma unroll
        for (int k = 0; k < DT_MAX_T; ++k) v[2 + k] = t.within[k];
        const bool first = mb_block_sum(v);
        dt_block_rest(t.max_d2, t.sum_d2, t.sum_d);
        if (first) {
            if (v[0]) atomicAdd(&n[pair], v[0]);
            if (v[1]) atomicAdd(&far[pair], v[1]);
#pragma unroll
            for (int k = 0; k < DT_MAX_T; ++k)
                if (k < T && v[2 + k]) atomicAdd(&within[pair * T + k], v[2 + k]);
            if (t.max_d2 >= 0) atomicMax(&max_d2[pair], t.max_d2);
            if (t.sum_d2) atomicAdd(&sum_d2[pair], (unsigned long long)t.sum_d2);
            part[0] = t.sum_d;
        }
        __syncthreads();                                              // the sums' LDS is free for the next pair
    }
}

__global__ __launch_bounds__(256) void dt_totals_finalize_kernel(const double* __restrict__ partial, int nparts, int N,
                                                                 double* __restrict__ sum_d) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    double s = 0.0;
    for (int j = 0; j < nparts; ++j) s += partial[i * nparts + j];
    sum_d[i] = s;
}

int64_t dt_round16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// partials of a pair = the workgroups that share it: about 4096 workgroups in all, at most 256 per pair -- a function of N alone
int dt_pair_parts(int64_t N) { return (int)std::max<int64_t>(1, std::min<int64_t>((4096 + N - 1) / N, 256)); }

// what both distance entries refuse
int dt_bad(const uint8_t* bits, int64_t nbytes, const int64_t* offsets, const int32_t* dims, const int32_t* reach, int32_t P,
           int64_t max_words, const int64_t* pix_offsets, int64_t n_pix, const void* workspace, int64_t ws_bytes, const int32_t* out_d2,
           const int32_t* status) {
    if (!bits || !offsets || !dims || !reach || !pix_offsets || !workspace || !out_d2 || !status) return CVLM_E_BADARG;
    if (mb_misaligned(4, bits, dims, reach, out_d2, status) || mb_misaligned(8, offsets, pix_offsets) || mb_misaligned(16, workspace))
        return CVLM_E_BADARG;
    if (P < 1 || P > 65535 || nbytes < 4 || n_pix < 1 || n_pix > ((int64_t)1 << 46) || max_words < 1 ||
        max_words > (int64_t)SZ_MAX_SIDE * (SZ_MAX_SIDE / 32))
        return CVLM_E_BADARG;
    if (ws_bytes < dt_round16(2 * n_pix)) return CVLM_E_WORKSPACE;
    const uint64_t nb = (uint64_t)nbytes, no = 4 * (uint64_t)n_pix, nw = (uint64_t)ws_bytes;
    const uint64_t nt = 4 * (uint64_t)P;
    const void* in[5] = {bits, offsets, dims, reach, pix_offsets};
    const uint64_t in_bytes[5] = {nb, 8 * ((uint64_t)P + 1), 2 * nt, nt, 8 * ((uint64_t)P + 1)};
    for (int i = 0; i < 5; ++i)
        if (mb_ranges_meet(out_d2, no, in[i], in_bytes[i]) || mb_ranges_meet(workspace, nw, in[i], in_bytes[i]) ||
            mb_ranges_meet(status, 4, in[i], in_bytes[i]))
            return CVLM_E_BADARG;
    if (mb_ranges_meet(out_d2, no, workspace, nw) || mb_ranges_meet(status, 4, out_d2, no) || mb_ranges_meet(status, 4, workspace, nw))
        return CVLM_E_BADARG;
    return 0;
}

// what both totals entries refuse
int dt_totals_bad(const uint8_t* a_bits, int64_t a_bytes, const int64_t* a_offsets, const int32_t* a_dims, int32_t Pa, const int32_t* b_d2,
                  const int64_t* b_pix_offsets, int64_t b_n_pix, const int32_t* b_dims, int32_t Pb, const int32_t* pairs, int64_t N,
                  const int32_t* radii, int32_t T, int64_t max_words, const void* workspace, int64_t ws_bytes, const int32_t* n,
                  const int32_t* far, const int32_t* within, const int32_t* max_d2, const int64_t* sum_d2, const double* sum_d,
                  const int32_t* status) {
    if (!a_bits || !a_offsets || !a_dims || !b_d2 || !b_pix_offsets || !b_dims || !pairs || !radii || !workspace || !n || !far || !within ||
        !max_d2 || !sum_d2 || !sum_d || !status)
        return CVLM_E_BADARG;
    if (mb_misaligned(4, a_bits, a_dims, b_d2, b_dims, pairs, radii, n, far, within, max_d2, status) ||
        mb_misaligned(8, a_offsets, b_pix_offsets, sum_d2, sum_d) || mb_misaligned(16, workspace))
        return CVLM_E_BADARG;
    if (Pa < 1 || Pa > 65535 || Pb < 1 || Pb > 65535 || N < 1 || N > ((int64_t)1 << 24) || T < 1 || T > DT_MAX_T || a_bytes < 4 ||
        b_n_pix < 1 || b_n_pix > ((int64_t)1 << 46) || max_words < 1 || max_words > (int64_t)SZ_MAX_SIDE * (SZ_MAX_SIDE / 32))
        return CVLM_E_BADARG;
    if (ws_bytes < dt_round16(8 * N * dt_pair_parts(N))) return CVLM_E_WORKSPACE;
    const uint64_t n4 = 4 * (uint64_t)N, n8 = 8 * (uint64_t)N;
    const void* in[8] = {a_bits, a_offsets, a_dims, b_d2, b_pix_offsets, b_dims, pairs, radii};
    const uint64_t in_bytes[8] = {(uint64_t)a_bytes, 8 * ((uint64_t)Pa + 1), 8 * (uint64_t)Pa, 4 * (uint64_t)b_n_pix, 8 * ((uint64_t)Pb + 1),
                                  8 * (uint64_t)Pb, 2 * n4, n4 * (uint64_t)T};
    const void* out[8] = {workspace, n, far, within, max_d2, sum_d2, sum_d, status};
    const uint64_t out_bytes[8] = {(uint64_t)ws_bytes, n4, n4, n4 * (uint64_t)T, n4, n8, n8, 4};
    for (int o = 0; o < 8; ++o) {
        for (int i = 0; i < 8; ++i)
            if (mb_ranges_meet(out[o], out_bytes[o], in[i], in_bytes[i])) return CVLM_E_BADARG;
        for (int q = o + 1; q < 8; ++q)
            if (mb_ranges_meet(out[o], out_bytes[o], out[q], out_bytes[q])) return CVLM_E_BADARG;
    }
    return 0;
}

}  // namespace

extern "C" {

int64_t cvlm_mask_distance_workspace_bytes(int32_t P, int64_t max_pixels) {
    if (P < 1 || P > 65535 || max_pixels < 1 || max_pixels > (int64_t)SZ_MAX_SIDE * SZ_MAX_SIDE) return CVLM_E_BADARG;
    return dt_round16(2 * (int64_t)P * max_pixels);
}

int cvlm_mask_distance_sized(const uint8_t* bits, int64_t n_bytes, const int64_t* offsets, const int32_t* dims, const int32_t* reach,
                             int32_t P, int64_t max_words, const int64_t* pix_offsets, int64_t n_pix, void* workspace, int64_t ws_bytes,
                             int32_t* out_d2, int32_t* status, void* stream) {
    if (const int rc = dt_bad(bits, n_bytes, offsets, dims, reach, P, max_words, pix_offsets, n_pix, workspace, ws_bytes, out_d2, status))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    // workgroups per plane: about 4096 in all and at most 256; the row pass has no more work than the largest plane's rows (fewer than
    // its words), the column pass none beyond its units (more than its words / 2); the waves walk what is left in strides
    const int64_t want = (4096 + P - 1) / P;
    const int gr = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>((max_words + 3) / 4, want), 256));
    const int gc = (int)std::max<int64_t>(1, std::min<int64_t>(want, 256));
    hipLaunchKernelGGL(dt_init_kernel, dim3(1), dim3(1), 0, st, (int*)status);
    CVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(dt_rows_kernel, dim3(gr, P), dim3(256), 0, st, bits, n_bytes, offsets, (const int*)dims, (const int*)reach, pix_offsets,
                       n_pix, (uint16_t*)workspace);
    CVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(dt_cols_kernel, dim3(gc, P), dim3(256), 0, st, n_bytes, offsets, (const int*)dims, (const int*)reach, pix_offsets, n_pix,
                       (const uint16_t*)workspace, out_d2, (int*)status);
    CVLM_CHECK_LAUNCH();
    return 0;
}

int64_t cvlm_mask_surface_workspace_bytes(int64_t N) {
    if (N < 1 || N > ((int64_t)1 << 24)) return CVLM_E_BADARG;
    return dt_round16(8 * N * dt_pair_parts(N));
}

int cvlm_mask_surface_totals(const uint8_t* a_bits, int64_t a_bytes, const int64_t* a_offsets, const int32_t* a_dims, int32_t Pa,
                             const int32_t* b_d2, const int64_t* b_pix_offsets, int64_t b_n_pix, const int32_t* b_dims, int32_t Pb,
                             const int32_t* pairs, int64_t N, const int32_t* radii, int32_t T, int64_t max_words, void* workspace,
                             int64_t ws_bytes, int32_t* n, int32_t* far, int32_t* within, int32_t* max_d2, int64_t* sum_d2, double* sum_d,
                             int32_t* status, void* stream) {
    if (const int rc = dt_totals_bad(a_bits, a_bytes, a_offsets, a_dims, Pa, b_d2, b_pix_offsets, b_n_pix, b_dims, Pb, pairs, N, radii, T,
                                     max_words, workspace, ws_bytes, n, far, within, max_d2, sum_d2, sum_d, status))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    // a thread per word: no more workgroups per pair than the largest plane has 256 words for, never more than the partials hold
    const int gx = (int)std::max<int64_t>(1, std::min<int64_t>((max_words + 255) / 256, dt_pair_parts(N)));
    const int gy = (int)std::min<int64_t>(N, 65535);
    hipLaunchKernelGGL(dt_totals_init_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, (int)N, (int)T, (int*)n, (int*)far,
                       (int*)within, (int*)max_d2, (long long*)sum_d2, (int*)status);
    CVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(dt_totals_kernel, dim3(gx, gy), dim3(256), 0, st, a_bits, a_bytes, a_offsets, (const int*)a_dims, (int)Pa, b_d2,
                       b_pix_offsets, b_n_pix, (const int*)b_dims, (int)Pb, (const int*)pairs, (int)N, (const int*)radii, (int)T,
                       (double*)workspace, (int*)n, (int*)far, (int*)within, (int*)max_d2, (unsigned long long*)sum_d2, (int*)status);
    CVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(dt_totals_finalize_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, (const double*)workspace, gx, (int)N,
                       sum_d);
    CVLM_CHECK_LAUNCH();
    return 0;
}

// The same functions on host memory: plane by plane, the row pass chunk by chunk and pixel by pixel into the workspace, the column
// pass pixel by pixel
int cvlm_debug_mask_distance_sized_host(const uint8_t* bits, int64_t n_bytes, const int64_t* offsets, const int32_t* dims,
                                        const int32_t* reach, int32_t P, int64_t max_words, const int64_t* pix_offsets, int64_t n_pix,
                                        void* workspace, int64_t ws_bytes, int32_t* out_d2, int32_t* status) {
    if (const int rc = dt_bad(bits, n_bytes, offsets, dims, reach, P, max_words, pix_offsets, n_pix, workspace, ws_bytes, out_d2, status))
        return rc;
    status[0] = 0;
    for (int p = 0; p < P; ++p) {
        const int h = dims[2 * p], w = dims[2 * p + 1], R = reach[p];
        const int64_t off = offsets[p], end = offsets[p + 1], poff = pix_offsets[p], pend = pix_offsets[p + 1];
        if (!sz_plane_ok(h, w, off, end, n_bytes) || !dt_reach_ok(R) || !dt_slice_ok(h, w, poff, pend, n_pix)) {
            if (dt_slice_sound(poff, pend, n_pix))
                for (int64_t i = poff; i < pend; ++i) out_d2[i] = DT_FAR;
            status[0] |= 1;
            continue;
        }
        const int ws = sz_words_per_row(w), chunks = (ws + 1) >> 1;
        const uint32_t* src = (const uint32_t*)(bits + off);
        uint16_t* f = (uint16_t*)workspace + poff;
        for (int y = 0; y < h; ++y) {
            const uint32_t* row = src + (int64_t)y * ws;
            uint16_t* frow = f + (int64_t)y * w;
            auto chunk_of = [&](int k) {
                return dt_chunk(cc_unpack(row[2 * k]), 2 * k + 1 < ws ? cc_unpack(row[2 * k + 1]) : 0u, 64 * k, w);
            };
            int carry = DT_NONE;
            for (int k = 0; k < chunks; ++k) {
                const uint64_t m = chunk_of(k);
                for (int i = 0; i < 64 && 64 * k + i < w; ++i) frow[64 * k + i] = dt_row_park(dt_gap_back(m, i, carry));
                carry = dt_gap_back(m, 63, carry);
            }
            carry = DT_NONE;
            for (int k = chunks - 1; k >= 0; --k) {
                const uint64_t m = chunk_of(k);
                for (int i = 0; i < 64 && 64 * k + i < w; ++i) frow[64 * k + i] = dt_row_value(frow[64 * k + i], dt_gap_fwd(m, i, carry), R);
                carry = dt_gap_fwd(m, 0, carry);
            }
        }
        int32_t* dst = out_d2 + poff;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) dst[(int64_t)y * w + x] = dt_column(f, h, w, y, x, R);
    }
    return 0;
}

// ... pair by pair, word by word, sum_d added in that order
int cvlm_debug_mask_surface_totals_host(const uint8_t* a_bits, int64_t a_bytes, const int64_t* a_offsets, const int32_t* a_dims, int32_t Pa,
                                        const int32_t* b_d2, const int64_t* b_pix_offsets, int64_t b_n_pix, const int32_t* b_dims, int32_t Pb,
                                        const int32_t* pairs, int64_t N, const int32_t* radii, int32_t T, int64_t max_words, void* workspace,
                                        int64_t ws_bytes, int32_t* n, int32_t* far, int32_t* within, int32_t* max_d2, int64_t* sum_d2,
                                        double* sum_d, int32_t* status) {
    if (const int rc = dt_totals_bad(a_bits, a_bytes, a_offsets, a_dims, Pa, b_d2, b_pix_offsets, b_n_pix, b_dims, Pb, pairs, N, radii, T,
                                     max_words, workspace, ws_bytes, n, far, within, max_d2, sum_d2, sum_d, status))
        return rc;
    status[0] = 0;
    for (int64_t pair = 0; pair < N; ++pair) {
        const int ia = pairs[2 * pair], ib = pairs[2 * pair + 1];
        const int32_t* rad = radii + pair * T;
        if (!dt_pair_ok(ia, ib, Pa, Pb, a_dims, a_offsets, a_bytes, b_dims, b_pix_offsets, b_n_pix, rad, T)) {
            n[pair] = far[pair] = max_d2[pair] = -1;
            sum_d2[pair] = -1;
            sum_d[pair] = 0.0;
            for (int k = 0; k < T; ++k) within[pair * T + k] = -1;
            status[0] |= 1;
            continue;
        }
        const int h = a_dims[2 * ia], w = a_dims[2 * ia + 1], ws = sz_words_per_row(w);
        const uint32_t* src = (const uint32_t*)(a_bits + a_offsets[ia]);
        const int32_t* map = b_d2 + b_pix_offsets[ib];
        int64_t r2[DT_MAX_T];
        for (int k = 0; k < DT_MAX_T; ++k) r2[k] = k < T ? (int64_t)rad[k] * rad[k] : -1;
        dt_totals t;
        for (int y = 0; y < h; ++y)
            for (int c = 0; c < ws; ++c) {
                uint32_t m = cc_unpack(src[(int64_t)y * ws + c]) & dt_word_mask(c, w);
                for (; m; m &= m - 1) dt_pixel(t, map[(int64_t)y * w + 32 * c + __builtin_ctz(m)], r2);
            }
        n[pair] = t.n;
        far[pair] = t.far;
        max_d2[pair] = t.max_d2;
        sum_d2[pair] = t.sum_d2;
        sum_d[pair] = t.sum_d;
        for (int k = 0; k < T; ++k) within[pair * T + k] = t.within[k];
    }
    return 0;
}

}  // extern "C"
