// Thinning of sized planes (include/cvlm.h: cvlm_mask_thin_sized): Guo & Hall's two-subiteration rule run to its fixed
// point, or for max_iter iterations, on planes of any mix of sizes -- skeletons of masks, one-pixel edges of thick edge maps, the
// centre lines of clDice.  The rule on 32 pixels at once -- eight neighbour words, three bit-sliced adders -- is thin_logic.h's th_word,
// shared with the sequential host entry at the end of this file.  All integers.
//
// th_init_kernel     status, areas, boxes, iters, done and the flags of the stepping path.
// th_resident_kernel one workgroup per plane.  A plane that fits (th_resident_in) is unpacked once into LDS inside a clear border of one
//                    row and one word column, so that no neighbour read needs a branch and a border word, being clear, stays clear.
//                    Per subiteration every thread computes the new words of its share (TH_SHARE at most, a word that is clear reads
//                    nothing) into registers from the old state; a barrier; the words that changed are stored; a barrier.  One LDS word
//                    per iteration parity collects "cleared something"; an iteration that cleared nothing, or the plane's max_iter,
//                    ends the loop: every iteration that continues has cleared a pixel.  Then the plane is packed to out_bits with its
//                    area and box.  The same workgroup zeroes the slice of a plane that is refused.
// th_step_kernel     the planes that are not resident, and every plane under mode = 1: one launch per subiteration, a thread per word,
//                    subiteration 1 from out_bits (the call's first from the input) into the workspace, subiteration 2 back; one
//                    integer atomic per workgroup into the plane's flag of that iteration.  A plane whose previous flag is clear, or
//                    whose max_iter is spent, costs a workgroup one flag read.
// th_finish_kernel   area and box of the stepped planes, iters and done from the flags.
// No workgroup waits for another; a refused plane is never read.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/cvlm.h"
#include "common.h"
#include "thin_logic.h"

namespace {

__global__ __launch_bounds__(256) void th_init_kernel(int P, int64_t n_flags, int* __restrict__ status, int* __restrict__ area,
                                                      int* __restrict__ box, int* __restrict__ iters, int* __restrict__ done,
                                                      int* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) status[0] = 0;
    if (i < P) {
        if (area) mb_init(area, box, (int)i);
        iters[i] = 0;
        done[i] = 0;
    }
    if (i < n_flags) flags[i] = 0;
}

// every thread of the plane's one workgroup: the slice zeroed where it can be, the refusal recorded
__device__ __forceinline__ void th_refuse(uint8_t* __restrict__ out_bits, int64_t off, int64_t end, int64_t nbytes, int* __restrict__ status) {
    if (th_slice_ok(off, end, nbytes)) {
        uint32_t* z = (uint32_t*)(out_bits + off);
        const int64_t n = (end - off) >> 2;
        for (int64_t i = threadIdx.x; i < n; i += blockDim.x) z[i] = 0u;
    }
    if (threadIdx.x == 0) atomicOr(status, 1);
}

// Plane blockIdx.x, NT = 256 or 1024 threads, dynamic LDS: the bordered plane.
template <int NT>
__global__ __launch_bounds__(NT) void th_resident_kernel(const uint8_t* __restrict__ bits, int64_t nbytes, const int64_t* __restrict__ offsets,
                                                         const int* __restrict__ dims, const int* __restrict__ max_iter, int64_t lds_bytes,
                                                         int64_t cells, int steps, uint8_t* __restrict__ out_bits, int* __restrict__ out_area,
                                                         int* __restrict__ out_box, int* __restrict__ out_iters, int* __restrict__ out_done,
                                                         int* __restrict__ status) {
    extern __shared__ uint32_t th_plane[];
    __shared__ int any[2];
    __shared__ volatile int geo[3];
    __shared__ unsigned red[NT / 64][5];
    constexpr int nt = NT;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int h = dims[2 * p], w = dims[2 * p + 1], mi = max_iter[p];
    const int64_t off = offsets[p], end = offsets[p + 1];
    if (!sz_plane_ok(h, w, off, end, nbytes) || !th_iter_ok(mi)) {    // the same for every thread
        th_refuse(out_bits, off, end, nbytes, status);
        return;
    }
    if (!th_resident_in(h, w, lds_bytes, cells)) {                    // the stepping path's; a call without steps has none
        if (steps == 0) th_refuse(out_bits, off, end, nbytes, status);
        return;
    }
    const int ws = sz_words_per_row(w), stride = ws + 2, words = h * ws;
    const int total = (h + 2) * stride;                               // <= lds_bytes / 4
    for (int j = tid; j < total; j += nt) th_plane[j] = 0u;
    if (tid < 2) any[tid] = 0;
    __syncthreads();
    const uint32_t* src = (const uint32_t*)(bits + off);
    for (int i = tid; i < words; i += nt) {
        const int y = i / ws, c = i - y * ws;
        th_plane[(y + 1) * stride + c + 1] = cc_unpack(src[i]) & th_col_mask(c, w);
    }
    __syncthreads();
    // the sweep: the rows 1 .. h of the bordered plane as one range; a border word is clear and is skipped like any clear word, so a
    // word that is worked on has all eight neighbours inside [0, total)
    // The range's ends and the number of shares (<= TH_SHARE: th_resident_in) are read back from LDS in every subiteration.  Kept
    // as values that the compiler knows not to change, their 38 tests were computed ahead of the loop and spilled.
    if (tid == 0) {
        geo[0] = stride;
        geo[1] = (h + 1) * stride;
        geo[2] = (h * stride + nt - 1) / nt;
    }
    __syncthreads();
    int it = 0;
    for (;;) {
        bool ch = false;
        int more = 0;
#pragma unroll 1
        for (int sub = 0; sub < 2; ++sub) {
            uint32_t nw[TH_SHARE];
            uint64_t diff = 0;
            const int j0 = geo[0], j1 = geo[1], shares = geo[2];
#pragma unroll
            for (int k = 0; k < TH_SHARE; ++k) {
                nw[k] = 0u;
                if (k < shares) {
                    const int j = j0 + tid + k * nt;
                    const uint32_t c = j < j1 ? th_plane[j] : 0u;
                    if (c) {
                        const uint32_t* n = th_plane + (j - stride);
                        const uint32_t* s = th_plane + (j + stride);
                        nw[k] = th_word(sub != 0, n[-1], n[0], n[1], th_plane[j - 1], c, th_plane[j + 1], s[-1], s[0], s[1], 0xffffffffu);
                        if (nw[k] != c) diff |= (uint64_t)1 << k;
                    }
                }
            }
            ch |= diff != 0;
            if (sub == 1 && ch) any[it & 1] = 1;                      // every writer writes the same value
            __syncthreads();                                          // every read of the old state is done
            if (sub == 1) {
                more = any[it & 1];
                if (tid == 0) any[(it + 1) & 1] = 0;                  // the next iteration's, which nobody touches before the barrier below
            }
#pragma unroll
            for (int k = 0; k < TH_SHARE; ++k)
                if ((diff >> k) & 1) th_plane[j0 + tid + k * nt] = nw[k];
            __syncthreads();
        }
        if (!more) break;
        ++it;
        if (mi != 0 && it >= mi) break;
    }
    uint32_t* dst = (uint32_t*)(out_bits + off);
    mb_stats st;
    for (int i = tid; i < words; i += nt) {
        const int y = i / ws, c = i - y * ws;
        const uint32_t m = th_plane[(y + 1) * stride + c + 1];
        dst[i] = cc_pack(m);
        if (m) mb_word(st, m, c, y);
    }
    if (tid == 0) {
        out_iters[p] = it;
        out_done[p] = 1;
    }
    if (!out_area) return;
    // the workgroup tail for up to 16 waves; the plane has this one workgroup, so thread 0 stores
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        st.cnt += __shfl_xor(st.cnt, o, 64);
        st.x0 = min(st.x0, __shfl_xor(st.x0, o, 64)); st.y0 = min(st.y0, __shfl_xor(st.y0, o, 64));
        st.x1 = max(st.x1, __shfl_xor(st.x1, o, 64)); st.y1 = max(st.y1, __shfl_xor(st.y1, o, 64));
    }
    if ((tid & 63) == 0) {
        unsigned* r = red[tid >> 6];
        r[0] = st.cnt; r[1] = st.x0; r[2] = st.y0; r[3] = (unsigned)st.x1; r[4] = (unsigned)st.y1;
    }
    __syncthreads();
    if (tid == 0) {
        mb_stats all;
        for (int v = 0; v < nt / 64; ++v) {
            all.cnt += red[v][0];
            all.x0 = min(all.x0, red[v][1]); all.y0 = min(all.y0, red[v][2]);
            all.x1 = max(all.x1, (int)red[v][3]); all.y1 = max(all.y1, (int)red[v][4]);
        }
        mb_store(all, out_area, out_box, p);                          // an empty plane keeps what the init kernel wrote
    }
}

// what the stepping kernels skip: -> true if plane p is theirs
__device__ __forceinline__ bool th_stepped(int h, int w, int mi, int64_t off, int64_t end, int64_t nbytes, int mode, int64_t lds_bytes,
                                           int64_t cells) {
    if (!sz_plane_ok(h, w, off, end, nbytes) || !th_iter_ok(mi)) return false;
    return mode != 0 || !th_resident_in(h, w, lds_bytes, cells);
}

// Subiteration `second` of iteration k of the call, plane blockIdx.y, a thread per word in strides.  flags: int [P][steps].
__global__ __launch_bounds__(256) void th_step_kernel(const uint8_t* __restrict__ src_bits, uint8_t* __restrict__ dst_bits, int64_t nbytes,
                                                      const int64_t* __restrict__ offsets, const int* __restrict__ dims,
                                                      const int* __restrict__ max_iter, int mode, int64_t lds_bytes, int64_t cells, int steps,
                                                      int k, int second, int* __restrict__ flags) {
    __shared__ int wg_any;
    const int p = blockIdx.y;
    const int h = dims[2 * p], w = dims[2 * p + 1], mi = max_iter[p];
    const int64_t off = offsets[p], end = offsets[p + 1];
    if (!th_stepped(h, w, mi, off, end, nbytes, mode, lds_bytes, cells)) return;      // the same for every thread of the plane
    if (mi != 0 && k >= mi) return;
    int* f = flags + (int64_t)p * steps;
    if (k > 0 && f[k - 1] == 0) return;                               // the iteration before cleared nothing, or never ran
    const int ws = sz_words_per_row(w), words = h * ws;
    if ((int64_t)blockIdx.x * 256 >= words) return;
    if (threadIdx.x == 0) wg_any = 0;
    __syncthreads();
    const uint32_t* src = (const uint32_t*)(src_bits + off);
    uint32_t* dst = (uint32_t*)(dst_bits + off);
    bool ch = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) {
        const int y = (int)(i / ws), c = (int)(i - (int64_t)y * ws);
        uint32_t old;
        const uint32_t nw = th_step_word(second != 0, src, h, w, ws, y, c, old);
        ch |= nw != old;
        dst[i] = cc_pack(nw);                                         // i < words: inside the plane's slice
    }
    if (__ballot(ch) && (threadIdx.x & 63) == 0) atomicOr(&wg_any, 1);
    __syncthreads();
    if (threadIdx.x == 0 && wg_any) atomicOr(&f[k], 1);
}

__global__ __launch_bounds__(256) void th_finish_kernel(const uint8_t* __restrict__ out_bits, int64_t nbytes, const int64_t* __restrict__ offsets,
                                                        const int* __restrict__ dims, const int* __restrict__ max_iter, int mode,
                                                        int64_t lds_bytes, int64_t cells, int steps, const int* __restrict__ flags,
                                                        int* __restrict__ out_area, int* __restrict__ out_box, int* __restrict__ out_iters,
                                                        int* __restrict__ out_done) {
    const int p = blockIdx.y;
    const int h = dims[2 * p], w = dims[2 * p + 1], mi = max_iter[p];
    const int64_t off = offsets[p], end = offsets[p + 1];
    if (!th_stepped(h, w, mi, off, end, nbytes, mode, lds_bytes, cells)) return;      // the same for every thread of the plane
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // the flags of a plane are set for a prefix of the iterations it was allowed: the ones that cleared something
        const int* f = flags + (int64_t)p * steps;
        const int cap = mi == 0 ? steps : min(steps, mi);
        int n = 0;
        while (n < cap && f[n]) ++n;
        out_iters[p] = n;
        out_done[p] = n < cap || (mi != 0 && n >= mi) ? 1 : 0;
    }
    if (!out_area) return;
    const int ws = sz_words_per_row(w), words = h * ws;
    if ((int64_t)blockIdx.x * 256 >= words) return;
    const uint32_t* src = (const uint32_t*)(out_bits + off);
    mb_stats st;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) {
        const int y = (int)(i / ws), c = (int)(i - (int64_t)y * ws);
        const uint32_t m = cc_unpack(src[i]);                         // the state's pad bits are clear
        if (m) mb_word(st, m, c, y);
    }
    mb_block_commit(st, out_area, out_box, p);
}

int64_t th_round16(int64_t v) { return (v + 15) & ~(int64_t)15; }
int64_t th_ws_need(int64_t n_bytes, int64_t P, int64_t steps) { return th_round16(n_bytes) + th_round16(4 * P * steps); }

// What ONE launch of the resident kernel offers, from max_words alone (the sizes are device memory): a plane of at most M words has
// at most 3 M + 6 words with its border -- h = M, one word column -- and sweeps at most 3 M of them.
struct th_offer { int threads; int64_t lds, cells; };
th_offer th_offer_of(int64_t max_words, int mode) {
    th_offer o;
    o.threads = 3 * max_words + 6 <= (int64_t)256 * TH_SHARE ? 256 : TH_THREADS;
    o.cells = (int64_t)o.threads * TH_SHARE;
    o.lds = mode != 0 ? 0 : std::min<int64_t>(TH_LDS_BUDGET, 4 * (3 * max_words + 6));
    return o;
}

// what both entries refuse
int th_bad(const uint8_t* bits, int64_t nbytes, const int64_t* offsets, const int32_t* dims, const int32_t* max_iter, int32_t P,
           int64_t max_words, int32_t mode, int32_t steps, const void* workspace, int64_t ws_bytes, const uint8_t* out_bits,
           const int32_t* out_area, const int32_t* out_box, const int32_t* out_iters, const int32_t* out_done, const int32_t* status) {
    if (!bits || !offsets || !dims || !max_iter || !workspace || !out_bits || !out_iters || !out_done || !status) return CVLM_E_BADARG;
    if ((out_area == nullptr) != (out_box == nullptr)) return CVLM_E_BADARG;
    if (mb_misaligned(4, bits, dims, max_iter, out_bits, out_area, out_box, out_iters, out_done, status) || mb_misaligned(8, offsets) ||
        mb_misaligned(16, workspace))
        return CVLM_E_BADARG;
    if (P < 1 || P > 65535 || nbytes < 4 || max_words < 1 || max_words > (int64_t)SZ_MAX_SIDE * (SZ_MAX_SIDE / 32)) return CVLM_E_BADARG;
    if (mode < 0 || mode > 1 || steps < 0 || steps > TH_MAX_STEPS) return CVLM_E_BADARG;
    // steps = 0 where a plane needs the stepping path, as far as the host can tell: every plane under mode = 1, and the largest
    // plane where its max_words words cannot be resident whatever its shape (h + ws >= 2 sqrt(h ws))
    if (steps == 0 && (mode == 1 || 4.0 * ((double)max_words + 4.0 * std::sqrt((double)max_words) + 4.0) > (double)TH_LDS_BUDGET))
        return CVLM_E_BADARG;
    if (ws_bytes < th_ws_need(nbytes, P, steps)) return CVLM_E_WORKSPACE;
    const uint64_t n4 = 4 * (uint64_t)P;
    const void* in[4] = {bits, offsets, dims, max_iter};
    const uint64_t in_bytes[4] = {(uint64_t)nbytes, 8 * ((uint64_t)P + 1), 2 * n4, n4};
    const void* out[7] = {workspace, out_bits, out_area, out_box, out_iters, out_done, status};
    const uint64_t out_bytes[7] = {(uint64_t)ws_bytes, (uint64_t)nbytes, n4, 4 * n4, n4, n4, 4};
    for (int o = 0; o < 7; ++o) {
        for (int i = 0; i < 4; ++i)
            if (mb_ranges_meet(out[o], out_bytes[o], in[i], in_bytes[i])) return CVLM_E_BADARG;
        for (int q = o + 1; q < 7; ++q)
            if (mb_ranges_meet(out[o], out_bytes[o], out[q], out_bytes[q])) return CVLM_E_BADARG;
    }
    return 0;
}

}  // namespace

extern "C" {

int64_t cvlm_mask_thin_workspace_bytes(int64_t n_bytes, int32_t P, int32_t steps) {
    if (n_bytes < 4 || n_bytes > ((int64_t)1 << 46) || P < 1 || P > 65535 || steps < 0 || steps > TH_MAX_STEPS) return CVLM_E_BADARG;
    return th_ws_need(n_bytes, P, steps);
}

int cvlm_mask_thin_resident(int32_t h, int32_t w) { return th_resident(h, w) ? 1 : 0; }

int cvlm_mask_thin_sized(const uint8_t* bits, int64_t n_bytes, const int64_t* offsets, const int32_t* dims, const int32_t* max_iter, int32_t P,
                         int64_t max_words, int32_t mode, int32_t steps, void* workspace, int64_t ws_bytes, uint8_t* out_bits,
                         int32_t* out_area, int32_t* out_box, int32_t* out_iters, int32_t* out_done, int32_t* status, void* stream) {
    if (const int rc = th_bad(bits, n_bytes, offsets, dims, max_iter, P, max_words, mode, steps, workspace, ws_bytes, out_bits, out_area,
                              out_box, out_iters, out_done, status))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const th_offer o = th_offer_of(max_words, mode);
    if (o.lds > 48 * 1024) {                                          // only the 1024-thread form is offered that much
        static bool once[16] = {};
        if (cvlm_first_on_device(once)) {
            const hipError_t e = hipFuncSetAttribute((const void*)th_resident_kernel<TH_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)TH_LDS_BUDGET);
            if (e != hipSuccess) return (int)e;
        }
    }
    uint8_t* state = (uint8_t*)workspace;
    int* flags = (int*)(state + th_round16(n_bytes));
    const int64_t n_flags = (int64_t)P * steps;
    hipLaunchKernelGGL(th_init_kernel, dim3((unsigned)((std::max<int64_t>(P, n_flags) + 255) / 256)), dim3(256), 0, st, (int)P, n_flags,
                       (int*)status, (int*)out_area, (int*)out_box, (int*)out_iters, (int*)out_done, flags);
    CVLM_CHECK_LAUNCH();
    if (o.threads == 256)
        hipLaunchKernelGGL(th_resident_kernel<256>, dim3(P), dim3(256), (size_t)o.lds, st, bits, n_bytes, offsets, (const int*)dims,
                           (const int*)max_iter, o.lds, o.cells, (int)steps, out_bits, (int*)out_area, (int*)out_box, (int*)out_iters,
                           (int*)out_done, (int*)status);
    else
        hipLaunchKernelGGL(th_resident_kernel<TH_THREADS>, dim3(P), dim3(TH_THREADS), (size_t)o.lds, st, bits, n_bytes, offsets,
                           (const int*)dims, (const int*)max_iter, o.lds, o.cells, (int)steps, out_bits, (int*)out_area, (int*)out_box,
                           (int*)out_iters, (int*)out_done, (int*)status);
    CVLM_CHECK_LAUNCH();
    if (steps == 0) return 0;
    // workgroups per plane: about 4096 in all and at most 256, none beyond the largest plane's words; the threads walk the rest in strides
    const int64_t want = (4096 + P - 1) / P;
    const int gx = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>((max_words + 255) / 256, want), 256));
    for (int k = 0; k < steps; ++k) {
        hipLaunchKernelGGL(th_step_kernel, dim3(gx, P), dim3(256), 0, st, k == 0 ? bits : (const uint8_t*)out_bits, state, n_bytes, offsets,
                           (const int*)dims, (const int*)max_iter, (int)mode, o.lds, o.cells, (int)steps, k, 0, flags);
        CVLM_CHECK_LAUNCH();
        hipLaunchKernelGGL(th_step_kernel, dim3(gx, P), dim3(256), 0, st, (const uint8_t*)state, out_bits, n_bytes, offsets, (const int*)dims,
                           (const int*)max_iter, (int)mode, o.lds, o.cells, (int)steps, k, 1, flags);
        CVLM_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(th_finish_kernel, dim3(gx, P), dim3(256), 0, st, (const uint8_t*)out_bits, n_bytes, offsets, (const int*)dims,
                       (const int*)max_iter, (int)mode, o.lds, o.cells, (int)steps, (const int*)flags, (int*)out_area, (int*)out_box,
                       (int*)out_iters, (int*)out_done);
    CVLM_CHECK_LAUNCH();
    return 0;
}

// The same th_word on host memory: plane by plane, subiteration 1 from the state (first the input) into the workspace, subiteration 2
// back into out_bits, word by word, until an iteration clears nothing or max_iter iterations have run.  mode and steps are checked
// and otherwise unused: every plane that is not refused is done.
int cvlm_debug_mask_thin_sized_host(const uint8_t* bits, int64_t n_bytes, const int64_t* offsets, const int32_t* dims, const int32_t* max_iter,
                                    int32_t P, int64_t max_words, int32_t mode, int32_t steps, void* workspace, int64_t ws_bytes,
                                    uint8_t* out_bits, int32_t* out_area, int32_t* out_box, int32_t* out_iters, int32_t* out_done,
                                    int32_t* status) {
    if (const int rc = th_bad(bits, n_bytes, offsets, dims, max_iter, P, max_words, mode, steps, workspace, ws_bytes, out_bits, out_area,
                              out_box, out_iters, out_done, status))
        return rc;
    status[0] = 0;
    for (int p = 0; p < P; ++p) {
        if (out_area) mb_init(out_area, out_box, p);
        out_iters[p] = out_done[p] = 0;
        const int h = dims[2 * p], w = dims[2 * p + 1], mi = max_iter[p];
        const int64_t off = offsets[p], end = offsets[p + 1];
        if (!sz_plane_ok(h, w, off, end, n_bytes) || !th_iter_ok(mi)) {
            if (th_slice_ok(off, end, n_bytes)) memset(out_bits + off, 0, (size_t)(end - off));
            status[0] |= 1;
            continue;
        }
        const int ws = sz_words_per_row(w);
        uint32_t* a = (uint32_t*)(out_bits + off);
        uint32_t* b = (uint32_t*)((uint8_t*)workspace + off);
        const uint32_t* src = (const uint32_t*)(bits + off);
        int it = 0;
        for (;;) {
            bool ch = false;
            for (int sub = 0; sub < 2; ++sub) {
                const uint32_t* from = sub ? b : src;
                uint32_t* to = sub ? a : b;
                for (int y = 0; y < h; ++y)
                    for (int c = 0; c < ws; ++c) {
                        uint32_t old;
                        const uint32_t nw = th_step_word(sub != 0, from, h, w, ws, y, c, old);
                        ch |= nw != old;
                        to[(int64_t)y * ws + c] = cc_pack(nw);
                    }
            }
            src = a;
            if (!ch) break;
            ++it;
            if (mi != 0 && it >= mi) break;
        }
        out_iters[p] = it;
        out_done[p] = 1;
        if (!out_area) continue;
        mb_stats st;
        for (int y = 0; y < h; ++y)
            for (int c = 0; c < ws; ++c)
                if (const uint32_t m = cc_unpack(a[(int64_t)y * ws + c])) mb_word(st, m, c, y);
        mb_store(st, out_area, out_box, p);
    }
    return 0;
}

}  // extern "C"
