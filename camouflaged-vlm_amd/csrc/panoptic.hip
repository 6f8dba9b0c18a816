// Panoptic quality on the device (include/cvlm.h: cvlm_pan_*): panopticapi's pq_compute restated for §23's flat maps --
// raw ground-truth ids to dense segment indices, the pair counts inter[b][g][s] of a ground-truth map against a predicted one, the
// per-image matching (true positives by IoU > 0.5, false negatives and crowd, false positives and ignored) and the sums over a dataset.
// The per-thread logic is panoptic_logic.h, shared with the sequential host entries at the end of this file.  The only floating-point
// results are one f64 division per candidate pair and the f64 sums of cvlm_pan_accumulate, added in a fixed order.
#include <algorithm>

#include "../../include/cvlm.h"
#include "common.h"
#include "panoptic_logic.h"

namespace {

typedef unsigned long long u64;

// what every pixel kernel does first: image b's table entries, the same for every thread of the image
struct pn_image { int h, w, upr, units; int64_t off; };
__device__ __forceinline__ bool pn_image_of(const int* __restrict__ dims, const int64_t* __restrict__ pix_off, int b, int64_t n_pix,
                                            int* __restrict__ status, pn_image& im) {
    im.h = dims[2 * b]; im.w = dims[2 * b + 1];
    im.off = pix_off[b];
    if (!pn_image_ok(im.h, im.w, im.off, pix_off[b + 1], n_pix)) {    // nothing of the image is read or stored
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, 1);
        return false;
    }
    im.upr = pn_units_per_row(im.w);
    im.units = im.h * im.upr;
    return true;
}

__global__ __launch_bounds__(256) void pn_zero_kernel(int* __restrict__ a, int64_t n) {
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) a[i] = 0;
}

// ---- remap ------------------------------------------------------------------------------------------------------------------------------
// Wave v of workgroup g takes the units 4 g + v, + 4 gridDim.x, ...; a lane searches its pixel's id in the image's keys.  The pixels
// whose id is not found are counted by ballot and popcount and reach unknown[b] as one atomic per wave that found one.
template <bool RGB>
__global__ __launch_bounds__(256) void pn_remap_kernel(const void* __restrict__ raw, const int* __restrict__ dims,
                                                       const int64_t* __restrict__ pix_off, int64_t n_pix, const int* __restrict__ keys,
                                                       const int* __restrict__ vals, const int64_t* __restrict__ tab_off, int64_t n_keys,
                                                       int* __restrict__ out, int* __restrict__ unknown, int* __restrict__ status) {
    const int b = blockIdx.y;
    pn_image im;
    if (!pn_image_of(dims, pix_off, b, n_pix, status, im)) return;
    const int64_t t0 = tab_off[b], t1 = tab_off[b + 1];
    if (!pn_table_ok(t0, t1, n_keys)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, 1);
        return;
    }
    const int nk = (int)(t1 - t0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int missed = 0;                                                   // the same in every lane
    for (int u = blockIdx.x * 4 + wave; u < im.units; u += gridDim.x * 4) {
        const int y = u / im.upr, x = 64 * (u - y * im.upr) + lane;
        bool unk = false;
        if (x < im.w) {
            const int64_t pix = im.off + (int64_t)y * im.w + x;
            const int id = RGB ? pn_rgb2id((const uint8_t*)raw + 3 * pix) : ((const int*)raw)[pix];
            out[pix] = pn_remap(keys + t0, vals + t0, nk, id, unk);
        }
        missed += __popcll(__ballot(unk));
    }
    if (missed && lane == 0) atomicAdd(&unknown[b], missed);
}

// ---- pair counts ----------------------------------------------------------------------------------------------------------------------------
// The walk of one wave over its units: the lanes that hold the same cell are counted by one ballot and popcount, and the count of one cell
// is held back (wave-uniform registers) until the wave meets another cell -- segment maps are piecewise constant, so a wave that walks
// the inside of a segment pair ends in one `add` instead of one per unit.  add(cell, n) is called by every lane; lane 0 acts.
template <typename Add>
__device__ __forceinline__ void pn_walk(const int* __restrict__ pred, const int* __restrict__ gt, const pn_image& im, int G, int S,
                                        int* __restrict__ status, Add add) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int held = -1, held_n = 0;                                        // the same in every lane; a wave sees fewer than 2^29 pixels
    bool bad = false;
    for (int u = blockIdx.x * 4 + wave; u < im.units; u += gridDim.x * 4) {
        const int y = u / im.upr, x = 64 * (u - y * im.upr) + lane;
        int cell = -1;
        if (x < im.w) {
            const int64_t pix = im.off + (int64_t)y * im.w + x;
            cell = pn_cell(gt[pix], pred[pix], G, S);
            bad |= cell < 0;
        }
        bool todo = cell >= 0;
        for (u64 open = __ballot(todo); open; open = __ballot(todo)) {
            const int c0 = __shfl(cell, __ffsll(open) - 1, 64);
            const bool same = todo && cell == c0;
            const u64 m = __ballot(same);
            if (c0 != held) {
                if (held >= 0) add(held, held_n);
                held = c0; held_n = 0;
            }
            held_n += __popcll(m);
            if (same) todo = false;
        }
    }
    if (held >= 0) add(held, held_n);
    if (__ballot(bad) && lane == 0) atomicOr(status, 2);
}

// G * S <= pn_lds_cells(): the image's table in the workgroup's LDS (dynamic: 4 G S bytes), flushed as one atomic per non-zero cell
__global__ __launch_bounds__(256) void pn_pair_lds_kernel(const int* __restrict__ pred, const int* __restrict__ gt, int G, int S,
                                                          const int* __restrict__ dims, const int64_t* __restrict__ pix_off, int64_t n_pix,
                                                          int* __restrict__ inter, int* __restrict__ status) {
    extern __shared__ int pn_bins[];
    const int b = blockIdx.y;
    pn_image im;
    if (!pn_image_of(dims, pix_off, b, n_pix, status, im)) return;
    if (blockIdx.x * 4 >= im.units) return;                           // the whole workgroup: no barrier has been passed
    const int cells = G * S;
    for (int i = threadIdx.x; i < cells; i += 256) pn_bins[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    pn_walk(pred, gt, im, G, S, status, [&](int cell, int n) { if (lane == 0) atomicAdd(&pn_bins[cell], n); });
    __syncthreads();
    int* __restrict__ mine = inter + (int64_t)b * cells;
    for (int i = threadIdx.x; i < cells; i += 256)
        if (pn_bins[i]) atomicAdd(&mine[i], pn_bins[i]);
}

// any G * S: the wave-aggregated counts go to the table in global memory
__global__ __launch_bounds__(256) void pn_pair_global_kernel(const int* __restrict__ pred, const int* __restrict__ gt, int G, int S,
                                                             const int* __restrict__ dims, const int64_t* __restrict__ pix_off,
                                                             int64_t n_pix, int* __restrict__ inter, int* __restrict__ status) {
    const int b = blockIdx.y;
    pn_image im;
    if (!pn_image_of(dims, pix_off, b, n_pix, status, im)) return;
    const int lane = threadIdx.x & 63;
    int* __restrict__ mine = inter + (int64_t)b * G * S;
    pn_walk(pred, gt, im, G, S, status, [&](int cell, int n) { if (lane == 0) atomicAdd(&mine[cell], n); });
}

// ---- matching -------------------------------------------------------------------------------------------------------------------------------
// One workgroup per image, no atomics: column and row sums, then the true positives (unique by IoU > 0.5: no two threads store to one
// slot), then the ground-truth side, then the predicted side.  The stores of a phase are read by the next behind a barrier.
__global__ __launch_bounds__(256) void pn_match_kernel(const int* __restrict__ inter, int G, int S, const int* __restrict__ pred_cat,
                                                       const int* __restrict__ gt_cat, const uint8_t* __restrict__ gt_crowd, int C,
                                                       int* __restrict__ pred_match, double* __restrict__ pred_iou,
                                                       int* __restrict__ gt_match, int* __restrict__ pred_area, int* __restrict__ gt_area) {
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int* __restrict__ in = inter + (int64_t)b * G * S;
    const int* __restrict__ pc = pred_cat + (int64_t)b * S;
    const int* __restrict__ gc = gt_cat + (int64_t)b * G;
    const uint8_t* __restrict__ gw = gt_crowd + (int64_t)b * G;
    int* __restrict__ pm = pred_match + (int64_t)b * S;
    double* __restrict__ pi = pred_iou + (int64_t)b * S;
    int* __restrict__ pa = pred_area + (int64_t)b * S;
    int* __restrict__ gm = gt_match + (int64_t)b * G;
    int* __restrict__ ga = gt_area + (int64_t)b * G;
    for (int s = threadIdx.x; s < S; s += 256) {                      // column sums: a thread per s, consecutive s in consecutive lanes
        int n = 0;
        for (int g = 0; g < G; ++g) n += in[(int64_t)g * S + s];
        pa[s] = n; pm[s] = 0; pi[s] = 0.0;
    }
    for (int g = wave; g < G; g += 4) {                               // row sums: a wave per g
        int n = 0;
        for (int s = lane; s < S; s += 64) n += in[(int64_t)g * S + s];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
        if (lane == 0) { ga[g] = n; gm[g] = 0; }
    }
    __syncthreads();
    for (int g = 1 + wave; g < G; g += 4) {
        const int cg = pn_cat(gc[g], C);
        if (cg < 0 || gw[g]) continue;                                // the whole wave
        const int area_g = ga[g];
        for (int s = 1 + lane; s < S; s += 64) {
            double iou;
            if (pn_tp(cg, pn_cat(pc[s], C), false, in[(int64_t)g * S + s], pa[s], area_g, in[s], iou)) { gm[g] = s; pm[s] = g; pi[s] = iou; }
        }
    }
    __syncthreads();
    for (int g = 1 + threadIdx.x; g < G; g += 256)
        if (pn_cat(gc[g], C) >= 0 && gm[g] == 0) gm[g] = gw[g] ? PN_CROWD : PN_FN;
    for (int s = 1 + threadIdx.x; s < S; s += 256) {
        const int cs = pn_cat(pc[s], C);
        if (cs < 0 || pa[s] <= 0 || pm[s] != 0) continue;
        int v = in[s];
        for (int g = G - 1; g >= 1; --g)                              // the category's crowd segment: the last in slot order
            if (gw[g] && pn_cat(gc[g], C) == cs) { v += in[(int64_t)g * S + s]; break; }
        pm[s] = pn_fp_ignored(v, pa[s]) ? PN_IGNORED : PN_FP;
    }
}

// ---- totals ---------------------------------------------------------------------------------------------------------------------------------
// One lane per category: it walks the images in increasing b and an image's slots in increasing g, then s, so that iou_sum[c] is added
// in that order whatever the launch looks like.
__global__ __launch_bounds__(256) void pn_accumulate_kernel(int B, int G, int S, const int* __restrict__ pred_cat,
                                                            const int* __restrict__ gt_cat, const int* __restrict__ pred_match,
                                                            const double* __restrict__ pred_iou, const int* __restrict__ gt_match, int C,
                                                            int zero_first, long long* __restrict__ counts, double* __restrict__ iou_sum) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    long long tp = 0, fp = 0, fn = 0;
    double sum = zero_first ? 0.0 : iou_sum[c];
    for (int b = 0; b < B; ++b) {
        const int64_t g0 = (int64_t)b * G, s0 = (int64_t)b * S;
        for (int g = 1; g < G; ++g) {
            if (gt_cat[g0 + g] != c) continue;
            const int m = gt_match[g0 + g];
            if (m > 0 && m < S) { ++tp; sum += pred_iou[s0 + m]; }
            else if (m == PN_FN) ++fn;
        }
        for (int s = 1; s < S; ++s)
            if (pred_cat[s0 + s] == c && pred_match[s0 + s] == PN_FP) ++fp;
    }
    if (zero_first) { counts[c] = tp; counts[C + c] = fp; counts[2 * C + c] = fn; }
    else { counts[c] += tp; counts[C + c] += fp; counts[2 * C + c] += fn; }
    iou_sum[c] = sum;
}

// ---- what the entries refuse ----------------------------------------------------------------------------------------------------------------
struct pn_range { const void* p; uint64_t bytes; };
// an output shares a byte with an input or with another output
template <size_t NI, size_t NO>
bool pn_outputs_meet(const pn_range (&in)[NI], const pn_range (&out)[NO]) {
    for (size_t o = 0; o < NO; ++o) {
        for (size_t i = 0; i < NI; ++i)
            if (mb_ranges_meet(out[o].p, out[o].bytes, in[i].p, in[i].bytes)) return true;
        for (size_t q = o + 1; q < NO; ++q)
            if (mb_ranges_meet(out[o].p, out[o].bytes, out[q].p, out[q].bytes)) return true;
    }
    return false;
}
bool pn_bad_tables(int32_t B, const int32_t* dims, const int64_t* pix_off, int64_t n_pix, int64_t max_pixels, const int32_t* status) {
    if (!dims || !pix_off || !status || mb_misaligned(4, dims, status) || mb_misaligned(8, pix_off)) return true;
    if (B < 1 || B > PN_MAX_B || n_pix < 1) return true;
    return max_pixels < 1 || max_pixels > (int64_t)PN_MAX_SIDE * PN_MAX_SIDE;
}
bool pn_bad_slots(int32_t G, int32_t S) { return G < 1 || S < 1 || (int64_t)G * S > PN_MAX_CELLS; }

bool pn_remap_bad(const void* raw, int32_t raw_is_rgb, int32_t B, const int32_t* dims, const int64_t* pix_off, int64_t n_pix,
                  int64_t max_pixels, const int32_t* keys, const int32_t* vals, const int64_t* tab_off, int64_t n_keys, const int32_t* out,
                  const int32_t* unknown, const int32_t* status) {
    if (!raw || !keys || !vals || !tab_off || !out || !unknown || pn_bad_tables(B, dims, pix_off, n_pix, max_pixels, status)) return true;
    if ((raw_is_rgb != 0 && raw_is_rgb != 1) || n_keys < 1) return true;
    if (mb_misaligned(4, keys, vals, out, unknown) || mb_misaligned(8, tab_off) || (!raw_is_rgb && mb_misaligned(4, raw))) return true;
    const uint64_t n = (uint64_t)n_pix, nb = (uint64_t)B;
    const pn_range in[] = {{raw, n * (raw_is_rgb ? 3 : 4)}, {dims, 8 * nb}, {pix_off, 8 * (nb + 1)}, {keys, 4 * (uint64_t)n_keys},
                           {vals, 4 * (uint64_t)n_keys}, {tab_off, 8 * (nb + 1)}};
    const pn_range outs[] = {{out, 4 * n}, {unknown, 4 * nb}, {status, 4}};
    return pn_outputs_meet(in, outs);
}
bool pn_pair_bad(const int32_t* pred, const int32_t* gt, int32_t B, int32_t G, int32_t S, const int32_t* dims, const int64_t* pix_off,
                 int64_t n_pix, int64_t max_pixels, const int32_t* inter, const int32_t* status) {
    if (!pred || !gt || !inter || pn_bad_tables(B, dims, pix_off, n_pix, max_pixels, status) || pn_bad_slots(G, S)) return true;
    if (mb_misaligned(4, pred, gt, inter)) return true;
    const uint64_t n = (uint64_t)n_pix, nb = (uint64_t)B;
    const pn_range in[] = {{pred, 4 * n}, {gt, 4 * n}, {dims, 8 * nb}, {pix_off, 8 * (nb + 1)}};
    const pn_range outs[] = {{inter, 4 * nb * G * S}, {status, 4}};
    return pn_outputs_meet(in, outs);
}
bool pn_match_bad(const int32_t* inter, int32_t B, int32_t G, int32_t S, const int32_t* pred_cat, const int32_t* gt_cat,
                  const uint8_t* gt_crowd, int32_t C, const int32_t* pred_match, const double* pred_iou, const int32_t* gt_match,
                  const int32_t* pred_area, const int32_t* gt_area) {
    if (!inter || !pred_cat || !gt_cat || !gt_crowd || !pred_match || !pred_iou || !gt_match || !pred_area || !gt_area) return true;
    if (B < 1 || B > PN_MAX_B || pn_bad_slots(G, S) || C < 1 || C > PN_MAX_C) return true;
    if (mb_misaligned(4, inter, pred_cat, gt_cat, pred_match, gt_match, pred_area, gt_area) || mb_misaligned(8, pred_iou)) return true;
    const uint64_t nb = (uint64_t)B, g = nb * G, s = nb * S;
    const pn_range in[] = {{inter, 4 * g * S}, {pred_cat, 4 * s}, {gt_cat, 4 * g}, {gt_crowd, g}};
    const pn_range outs[] = {{pred_match, 4 * s}, {pred_iou, 8 * s}, {gt_match, 4 * g}, {pred_area, 4 * s}, {gt_area, 4 * g}};
    return pn_outputs_meet(in, outs);
}
bool pn_accumulate_bad(int32_t B, int32_t G, int32_t S, const int32_t* pred_cat, const int32_t* gt_cat, const int32_t* pred_match,
                       const double* pred_iou, const int32_t* gt_match, int32_t C, const int64_t* counts, const double* iou_sum) {
    if (!pred_cat || !gt_cat || !pred_match || !pred_iou || !gt_match || !counts || !iou_sum) return true;
    if (B < 1 || B > PN_MAX_B || pn_bad_slots(G, S) || C < 1 || C > PN_MAX_C) return true;
    if (mb_misaligned(4, pred_cat, gt_cat, pred_match, gt_match) || mb_misaligned(8, pred_iou, counts, iou_sum)) return true;
    const uint64_t nb = (uint64_t)B, g = nb * G, s = nb * S;
    const pn_range in[] = {{pred_cat, 4 * s}, {gt_cat, 4 * g}, {pred_match, 4 * s}, {pred_iou, 8 * s}, {gt_match, 4 * g}};
    const pn_range outs[] = {{counts, 24 * (uint64_t)C}, {iou_sum, 8 * (uint64_t)C}};
    return pn_outputs_meet(in, outs);
}

// workgroups per image of a pixel kernel: one per four units of the largest image, `total` in all; the waves walk the rest in strides
int pn_grid_x(int64_t max_pixels, int images, int total) {
    const int64_t by_work = (max_pixels / 64 + PN_MAX_SIDE + 3) / 4;  // units <= h * w / 64 + h
    const int64_t want = (total + images - 1) / images;
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(by_work, want), 2048));
}

// ---- the host entries' loops ------------------------------------------------------------------------------------------------------------------
void pn_match_host(const int* in, int G, int S, const int* pc, const int* gc, const uint8_t* gw, int C, int* pm, double* pi, int* gm,
                   int* pa, int* ga) {
    for (int s = 0; s < S; ++s) {
        int n = 0;
        for (int g = 0; g < G; ++g) n += in[(int64_t)g * S + s];
        pa[s] = n; pm[s] = 0; pi[s] = 0.0;
    }
    for (int g = 0; g < G; ++g) {
        int n = 0;
        for (int s = 0; s < S; ++s) n += in[(int64_t)g * S + s];
        ga[g] = n; gm[g] = 0;
    }
    for (int g = 1; g < G; ++g) {
        const int cg = pn_cat(gc[g], C);
        if (cg < 0 || gw[g]) continue;
        for (int s = 1; s < S; ++s) {
            double iou;
            if (pn_tp(cg, pn_cat(pc[s], C), false, in[(int64_t)g * S + s], pa[s], ga[g], in[s], iou)) { gm[g] = s; pm[s] = g; pi[s] = iou; }
        }
    }
    for (int g = 1; g < G; ++g)
        if (pn_cat(gc[g], C) >= 0 && gm[g] == 0) gm[g] = gw[g] ? PN_CROWD : PN_FN;
    for (int s = 1; s < S; ++s) {
        const int cs = pn_cat(pc[s], C);
        if (cs < 0 || pa[s] <= 0 || pm[s] != 0) continue;
        int v = in[s];
        for (int g = G - 1; g >= 1; --g)
            if (gw[g] && pn_cat(gc[g], C) == cs) { v += in[(int64_t)g * S + s]; break; }
        pm[s] = pn_fp_ignored(v, pa[s]) ? PN_IGNORED : PN_FP;
    }
}

}  // namespace

extern "C" {

int cvlm_debug_pan_lds_cells(void) { return pn_lds_cells(); }

int cvlm_pan_remap(const void* raw, int32_t raw_is_rgb, int32_t B, const int32_t* dims, const int64_t* pix_offsets, int64_t n_pix,
                   int64_t max_pixels, const int32_t* keys, const int32_t* vals, const int64_t* table_offsets, int64_t n_keys, int32_t* out,
                   int32_t* unknown, int32_t* status, void* stream) {
    if (pn_remap_bad(raw, raw_is_rgb, B, dims, pix_offsets, n_pix, max_pixels, keys, vals, table_offsets, n_keys, out, unknown, status))
        return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pn_zero_kernel, dim3((B + 255) / 256), dim3(256), 0, st, (int*)unknown, (int64_t)B);
    CVLM_CHECK_LAUNCH();
    const dim3 grid(pn_grid_x(max_pixels, B, 8192), B);
    if (raw_is_rgb)
        hipLaunchKernelGGL(pn_remap_kernel<true>, grid, dim3(256), 0, st, raw, (const int*)dims, pix_offsets, n_pix, (const int*)keys,
                           (const int*)vals, table_offsets, n_keys, (int*)out, (int*)unknown, (int*)status);
    else
        hipLaunchKernelGGL(pn_remap_kernel<false>, grid, dim3(256), 0, st, raw, (const int*)dims, pix_offsets, n_pix, (const int*)keys,
                           (const int*)vals, table_offsets, n_keys, (int*)out, (int*)unknown, (int*)status);
    CVLM_CHECK_LAUNCH();
    return 0;
}

int cvlm_pan_pair_hist(const int32_t* pred, const int32_t* gt, int32_t B, int32_t G, int32_t S, const int32_t* dims,
                       const int64_t* pix_offsets, int64_t n_pix, int64_t max_pixels, int32_t zero_first, int32_t* inter, int32_t* status,
                       void* stream) {
    if (pn_pair_bad(pred, gt, B, G, S, dims, pix_offsets, n_pix, max_pixels, inter, status)) return CVLM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int cells = G * S;
    if (zero_first) {
        const int64_t n = (int64_t)B * cells;
        hipLaunchKernelGGL(pn_zero_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, st, (int*)inter, n);
        CVLM_CHECK_LAUNCH();
    }
    if (cells <= pn_lds_cells()) {
        const size_t lds = (size_t)4 * cells;
        if (lds > 48 * 1024) {
            static bool once[16] = {};
            if (cvlm_first_on_device(once)) {
                const hipError_t e = hipFuncSetAttribute((const void*)pn_pair_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                         4 * pn_lds_cells());
                if (e != hipSuccess) return (int)e;
            }
        }
        hipLaunchKernelGGL(pn_pair_lds_kernel, dim3(pn_grid_x(max_pixels, B, 1024), B), dim3(256), lds, st, (const int*)pred, (const int*)gt,
                           (int)G, (int)S, (const int*)dims, pix_offsets, n_pix, (int*)inter, (int*)status);
    } else {
        hipLaunchKernelGGL(pn_pair_global_kernel, dim3(pn_grid_x(max_pixels, B, 8192), B), dim3(256), 0, st, (const int*)pred, (const int*)gt,
                           (int)G, (int)S, (const int*)dims, pix_offsets, n_pix, (int*)inter, (int*)status);
    }
    CVLM_CHECK_LAUNCH();
    return 0;
}

int cvlm_pan_match(const int32_t* inter, int32_t B, int32_t G, int32_t S, const int32_t* pred_cat, const int32_t* gt_cat,
                   const uint8_t* gt_crowd, int32_t C, int32_t* pred_match, double* pred_iou, int32_t* gt_match, int32_t* pred_area,
                   int32_t* gt_area, void* stream) {
    if (pn_match_bad(inter, B, G, S, pred_cat, gt_cat, gt_crowd, C, pred_match, pred_iou, gt_match, pred_area, gt_area)) return CVLM_E_BADARG;
    hipLaunchKernelGGL(pn_match_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (const int*)inter, (int)G, (int)S, (const int*)pred_cat,
                       (const int*)gt_cat, gt_crowd, (int)C, (int*)pred_match, pred_iou, (int*)gt_match, (int*)pred_area, (int*)gt_area);
    CVLM_CHECK_LAUNCH();
    return 0;
}

int cvlm_pan_accumulate(int32_t B, int32_t G, int32_t S, const int32_t* pred_cat, const int32_t* gt_cat, const int32_t* pred_match,
                        const double* pred_iou, const int32_t* gt_match, int32_t C, int32_t zero_first, int64_t* counts, double* iou_sum,
                        void* stream) {
    if (pn_accumulate_bad(B, G, S, pred_cat, gt_cat, pred_match, pred_iou, gt_match, C, counts, iou_sum)) return CVLM_E_BADARG;
    hipLaunchKernelGGL(pn_accumulate_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, (int)B, (int)G, (int)S,
                       (const int*)pred_cat, (const int*)gt_cat, (const int*)pred_match, pred_iou, (const int*)gt_match, (int)C,
                       (int)zero_first, (long long*)counts, iou_sum);
    CVLM_CHECK_LAUNCH();
    return 0;
}

// ---- the same functions on host memory, image by image and pixel by pixel --------------------------------------------------------------
int cvlm_debug_pan_remap_host(const void* raw, int32_t raw_is_rgb, int32_t B, const int32_t* dims, const int64_t* pix_offsets, int64_t n_pix,
                              int64_t max_pixels, const int32_t* keys, const int32_t* vals, const int64_t* table_offsets, int64_t n_keys,
                              int32_t* out, int32_t* unknown, int32_t* status) {
    if (pn_remap_bad(raw, raw_is_rgb, B, dims, pix_offsets, n_pix, max_pixels, keys, vals, table_offsets, n_keys, out, unknown, status))
        return CVLM_E_BADARG;
    for (int b = 0; b < B; ++b) {
        unknown[b] = 0;
        const int h = dims[2 * b], w = dims[2 * b + 1];
        const int64_t off = pix_offsets[b], t0 = table_offsets[b], t1 = table_offsets[b + 1];
        if (!pn_image_ok(h, w, off, pix_offsets[b + 1], n_pix) || !pn_table_ok(t0, t1, n_keys)) { status[0] |= 1; continue; }
        for (int64_t i = off; i < off + (int64_t)h * w; ++i) {
            const int id = raw_is_rgb ? pn_rgb2id((const uint8_t*)raw + 3 * i) : ((const int32_t*)raw)[i];
            bool unk;
            out[i] = pn_remap(keys + t0, vals + t0, (int)(t1 - t0), id, unk);
            unknown[b] += unk;
        }
    }
    return 0;
}

int cvlm_debug_pan_pair_hist_host(const int32_t* pred, const int32_t* gt, int32_t B, int32_t G, int32_t S, const int32_t* dims,
                                  const int64_t* pix_offsets, int64_t n_pix, int64_t max_pixels, int32_t zero_first, int32_t* inter,
                                  int32_t* status) {
    if (pn_pair_bad(pred, gt, B, G, S, dims, pix_offsets, n_pix, max_pixels, inter, status)) return CVLM_E_BADARG;
    const int64_t cells = (int64_t)G * S;
    if (zero_first)
        for (int64_t i = 0; i < B * cells; ++i) inter[i] = 0;
    for (int b = 0; b < B; ++b) {
        const int h = dims[2 * b], w = dims[2 * b + 1];
        const int64_t off = pix_offsets[b];
        if (!pn_image_ok(h, w, off, pix_offsets[b + 1], n_pix)) { status[0] |= 1; continue; }
        for (int64_t i = off; i < off + (int64_t)h * w; ++i) {
            const int cell = pn_cell(gt[i], pred[i], G, S);
            if (cell < 0) status[0] |= 2;
            else ++inter[b * cells + cell];
        }
    }
    return 0;
}

int cvlm_debug_pan_match_host(const int32_t* inter, int32_t B, int32_t G, int32_t S, const int32_t* pred_cat, const int32_t* gt_cat,
                              const uint8_t* gt_crowd, int32_t C, int32_t* pred_match, double* pred_iou, int32_t* gt_match,
                              int32_t* pred_area, int32_t* gt_area) {
    if (pn_match_bad(inter, B, G, S, pred_cat, gt_cat, gt_crowd, C, pred_match, pred_iou, gt_match, pred_area, gt_area)) return CVLM_E_BADARG;
    for (int64_t b = 0; b < B; ++b)
        pn_match_host(inter + b * G * S, G, S, pred_cat + b * S, gt_cat + b * G, gt_crowd + b * G, C, pred_match + b * S, pred_iou + b * S,
                      gt_match + b * G, pred_area + b * S, gt_area + b * G);
    return 0;
}

int cvlm_debug_pan_accumulate_host(int32_t B, int32_t G, int32_t S, const int32_t* pred_cat, const int32_t* gt_cat,
                                   const int32_t* pred_match, const double* pred_iou, const int32_t* gt_match, int32_t C,
                                   int32_t zero_first, int64_t* counts, double* iou_sum) {
    if (pn_accumulate_bad(B, G, S, pred_cat, gt_cat, pred_match, pred_iou, gt_match, C, counts, iou_sum)) return CVLM_E_BADARG;
    if (zero_first) {
        for (int i = 0; i < 3 * C; ++i) counts[i] = 0;
        for (int i = 0; i < C; ++i) iou_sum[i] = 0.0;
    }
    for (int64_t b = 0; b < B; ++b) {                                 // per category the same order of additions as the kernel's lane
        for (int g = 1; g < G; ++g) {
            const int c = pn_cat(gt_cat[b * G + g], C);
            if (c < 0) continue;
            const int m = gt_match[b * G + g];
            if (m > 0 && m < S) { ++counts[c]; iou_sum[c] += pred_iou[b * S + m]; }
            else if (m == PN_FN) ++counts[2 * C + c];
        }
        for (int s = 1; s < S; ++s) {
            const int c = pn_cat(pred_cat[b * S + s], C);
            if (c >= 0 && pred_match[b * S + s] == PN_FP) ++counts[C + c];
        }
    }
    return 0;
}

}  // extern "C"
