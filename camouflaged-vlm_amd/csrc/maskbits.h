// The packed-mask family: what its members share, written once.  The stored word order, the area and box of a
// plane -- accumulator, workgroup tail, init and store --, the workgroup sum of per-plane counts, and the predicates from which every
// entry's *_bad* function states what it refuses.  A new member includes this header, not a sibling's *_logic.h.  Host and device; no
// HIP runtime call, no allocation.  Everything here has at least two callers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CC_HD __host__ __device__ __forceinline__
#else
#define CC_HD inline
#endif

// ---- words ----------------------------------------------------------------------------------------------------------------------------
// In memory a word is in numpy.packbits' order (pixel i -> bit 7 - (i & 7) of byte i >> 3, bytes in memory order): what cvlm_mask_pack
// stores.  cc_unpack turns it into bit i = pixel i of the word; cc_pack is its inverse: bit reversal + byte swap.
CC_HD uint32_t cc_unpack(uint32_t stored) { return __builtin_bitreverse32(__builtin_bswap32(stored)); }
CC_HD uint32_t cc_pack(uint32_t word) { return __builtin_bswap32(__builtin_bitreverse32(word)); }

// ---- area and box of a plane -------------------------------------------------------------------------------------------------------------
// area = 0, box = (-1, -1, -1, -1) before anything is counted: the corners x0 / y0 are then lowered by UNSIGNED minima (0xffffffff is
// the largest unsigned and -1 as the int32 the caller reads), x1 / y1 raised by signed maxima -- an empty plane needs no second pass.
// mb_stats is one thread's, or one host loop's, share of a plane in the same scheme.
struct mb_stats {
    unsigned cnt = 0, x0 = 0xffffffffu, y0 = 0xffffffffu;
    int x1 = -1, y1 = -1;
};
// one set pixel
CC_HD void mb_pixel(mb_stats& s, int x, int y) {
    ++s.cnt;
    s.x0 = (unsigned)x < s.x0 ? (unsigned)x : s.x0;
    s.y0 = (unsigned)y < s.y0 ? (unsigned)y : s.y0;
    s.x1 = x > s.x1 ? x : s.x1;
    s.y1 = y > s.y1 ? y : s.y1;
}
// the set pixels of the unpacked word m != 0 of word column c of row y
CC_HD void mb_word(mb_stats& s, uint32_t m, int c, int y) {
    s.cnt += (unsigned)__builtin_popcount(m);
    const unsigned lo = (unsigned)(32 * c + __builtin_ctz(m));
    const int hi = 32 * c + 31 - __builtin_clz(m);
    s.x0 = lo < s.x0 ? lo : s.x0;
    s.y0 = (unsigned)y < s.y0 ? (unsigned)y : s.y0;
    s.x1 = hi > s.x1 ? hi : s.x1;
    s.y1 = y > s.y1 ? y : s.y1;
}
CC_HD void mb_init(int32_t* area, int32_t* box, int p) {
    area[p] = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) box[4 * p + k] = -1;
}
// a sequential caller's whole plane: one that found nothing leaves what mb_init wrote
CC_HD void mb_store(const mb_stats& s, int32_t* area, int32_t* box, int p) {
    if (!s.cnt) return;
    area[p] = (int32_t)s.cnt;
    box[4 * p + 0] = (int32_t)s.x0; box[4 * p + 1] = (int32_t)s.y0; box[4 * p + 2] = s.x1; box[4 * p + 3] = s.y1;
}

#if defined(__HIPCC__) || defined(__CUDACC__)
// The body of a family member's init kernel, one thread per plane of 256-thread workgroups: status = 0 (where the entry has one),
// then mb_init for each of the P planes (where the call asks for areas and boxes).
__device__ __forceinline__ void mb_init_planes(int* __restrict__ status, int* __restrict__ area, int* __restrict__ box, int P) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (status && p == 0) status[0] = 0;
    if (!area || p >= P) return;
    mb_init(area, box, p);
}

// The tail of a 256-thread workgroup that has walked a part of plane p: the threads' shares reduced over the wave by xor-shuffles,
// over the four waves through LDS, then five atomics by thread 0.  Every thread of the workgroup calls it.
__device__ __forceinline__ void mb_block_commit(mb_stats s, int* __restrict__ area, int* __restrict__ box, int64_t p) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s.cnt += __shfl_xor(s.cnt, o, 64);
        s.x0 = min(s.x0, __shfl_xor(s.x0, o, 64)); s.y0 = min(s.y0, __shfl_xor(s.y0, o, 64));
        s.x1 = max(s.x1, __shfl_xor(s.x1, o, 64)); s.y1 = max(s.y1, __shfl_xor(s.y1, o, 64));
    }
    __shared__ unsigned red[4][5];
    if ((threadIdx.x & 63) == 0) {
        unsigned* r = red[threadIdx.x >> 6];
        r[0] = s.cnt; r[1] = s.x0; r[2] = s.y0; r[3] = (unsigned)s.x1; r[4] = (unsigned)s.y1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned c = red[0][0] + red[1][0] + red[2][0] + red[3][0];
        if (c) {                                                      // a workgroup that found nothing leaves the plane's results alone
            atomicAdd(&area[p], (int)c);
            atomicMin((unsigned*)&box[4 * p + 0], min(min(red[0][1], red[1][1]), min(red[2][1], red[3][1])));
            atomicMin((unsigned*)&box[4 * p + 1], min(min(red[0][2], red[1][2]), min(red[2][2], red[3][2])));
            atomicMax(&box[4 * p + 2], max(max((int)red[0][3], (int)red[1][3]), max((int)red[2][3], (int)red[3][3])));
            atomicMax(&box[4 * p + 3], max(max((int)red[0][4], (int)red[1][4]), max((int)red[2][4], (int)red[3][4])));
        }
    }
}

// N integer sums over a 256-thread workgroup: v[0 .. N) of every thread go in, and behind the call thread 0 holds the totals in its
// v (the other threads' v are then partial sums of no meaning).  -> true in thread 0 alone, so that `if (mb_block_sum(n) && n[0])
// atomicAdd(...)` is the caller's own "add only if non-zero".  Every thread of the workgroup calls it.
template <int N>
__device__ __forceinline__ bool mb_block_sum(int (&v)[N]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] += __shfl_xor(v[i], o, 64);
    __shared__ int red[4][N];
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int i = 0; i < N; ++i) red[threadIdx.x >> 6][i] = v[i];
    __syncthreads();
    if (threadIdx.x != 0) return false;
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = red[0][i] + red[1][i] + red[2][i] + red[3][i];
    return true;
}
#endif

// ---- what the entries refuse: pure predicates on values, host only -----------------------------------------------------------------------
// P planes of H rows of W / 32 whole words, the pixel index of a plane an int, the plane a grid's y index
inline bool mb_bad_planes(int32_t P, int32_t H, int32_t W) {
    return P < 1 || P > 65535 || H <= 0 || W <= 0 || W % 32 != 0 || (int64_t)H * W >= ((int64_t)1 << 31);
}
// any of these pointers is off a multiple of `align` (4, 8 or 16) bytes; a NULL is on one
template <typename... T>
inline bool mb_misaligned(uintptr_t align, const T*... ptrs) { return ((... | (uintptr_t)ptrs) & (align - 1)) != 0; }
// the workspace of a call that needs at least `need` bytes of it
inline bool mb_bad_workspace(const void* workspace, int64_t bytes, int64_t need) {
    return !workspace || mb_misaligned(16, workspace) || bytes < need;
}
// planes of a round: as many as the workspace holds
inline int mb_fit(int32_t P, int64_t workspace_bytes, int64_t plane_bytes) {
    const int64_t fit = workspace_bytes / plane_bytes;
    return (int)(fit < P ? fit : P);
}
// two byte ranges that exist share a byte
inline bool mb_ranges_meet(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + b_bytes && y < x + a_bytes;
}
