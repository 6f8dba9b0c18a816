// Panoptic quality: the per-thread logic of the cvlm_pan_* kernels (panoptic.hip), written once for the device and for
// the sequential host entries cvlm_debug_pan_*_host, which run these same functions on the CPU.  No HIP call, no allocation.
//
//   - pn_image_ok / pn_units_per_row: §23's rules for an image's table entries and its units of 64 pixels;
//   - pn_rgb2id / pn_find: panopticapi's rgb2id and the binary search of a raw id in an image's sorted keys;
//   - pn_cell: the (gt, pred) cell of a pixel, or -1 where an index is out of range;
//   - pn_lds_cells: the table size up to which a workgroup keeps the pair counts in its LDS;
//   - pn_cat: a slot's category, or -1 where the slot is unused;
//   - pn_tp: the published test of a pair (same category, no crowd, IoU over the union without the void part > 0.5);
//   - pn_fp_ignored: the published test of an unmatched predicted segment against void and its category's crowd segment.
#pragma once
#include <stdint.h>

#include "maskbits.h"

#define PN_HD CC_HD

constexpr int PN_MAX_B = 65535;                                       // images of a call: a grid's y index
constexpr int PN_MAX_C = 65536;                                       // categories
constexpr int PN_MAX_CELLS = 1 << 24;                                 // G * S: a cell index is an int with room to spare
constexpr int PN_MAX_SIDE = 16384;                                    // h and w of an image, as §19 to §23 have them
#ifndef CVLM_PN_LDS_CELLS                                             // a probe build measures another bound: make EXTRA=-DCVLM_PN_LDS_CELLS=...
#define CVLM_PN_LDS_CELLS 40960
#endif
constexpr int PN_LDS_CELLS = CVLM_PN_LDS_CELLS;                       // 160 KiB of int32 counters, a CU's whole LDS: measured, DESIGN.md §24

PN_HD int pn_lds_cells() { return PN_LDS_CELLS; }

// Image b of a call with n_pix pixels of maps: its size is a size and its slice [off, end) is its h * w pixels inside [0, n_pix)
PN_HD bool pn_image_ok(int h, int w, int64_t off, int64_t end, int64_t n_pix) {
    if (h < 1 || w < 1 || h > PN_MAX_SIDE || w > PN_MAX_SIDE) return false;
    return off >= 0 && end <= n_pix && end - off == (int64_t)h * w;
}
PN_HD int pn_units_per_row(int w) { return (w + 63) >> 6; }

// image b's slice [t0, t1) of the key / value tables
PN_HD bool pn_table_ok(int64_t t0, int64_t t1, int64_t n_keys) { return t0 >= 0 && t0 <= t1 && t1 <= n_keys && t1 - t0 < ((int64_t)1 << 31); }

PN_HD int pn_rgb2id(const uint8_t* px) { return (int)px[0] + 256 * (int)px[1] + 65536 * (int)px[2]; }

// index of `id` in keys[0 .. n), ascending, or -1
PN_HD int pn_find(const int32_t* keys, int n, int id) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && keys[lo] == id ? lo : -1;
}

// One pixel of the remap: raw id -> dense index; unknown = "a non-zero id that the table does not hold"
PN_HD int pn_remap(const int32_t* keys, const int32_t* vals, int n, int id, bool& unknown) {
    unknown = false;
    if (id == 0) return 0;
    const int at = pn_find(keys, n, id);
    if (at < 0) { unknown = true; return 0; }
    return vals[at];
}

PN_HD int pn_cell(int g, int s, int G, int S) { return (unsigned)g < (unsigned)G && (unsigned)s < (unsigned)S ? g * S + s : -1; }

PN_HD int pn_cat(int cat, int C) { return cat >= 0 && cat < C ? cat : -1; }

// Step 2 for the pair (g, s), both >= 1: inter = inter[g][s], void_s = inter[0][s].  -> true with its IoU where the pair is a TP
PN_HD bool pn_tp(int cat_g, int cat_s, bool crowd_g, int inter, int pred_area, int gt_area, int void_s, double& iou) {
    if (cat_g < 0 || cat_s < 0 || crowd_g || cat_g != cat_s || inter <= 0) return false;
    const int64_t uni = (int64_t)pred_area + gt_area - inter - void_s;
    iou = (double)inter / (double)uni;
    return iou > 0.5;
}

// Step 4 for an unmatched predicted segment with pixels: v = its pixels on void and on its category's crowd segment
PN_HD bool pn_fp_ignored(int v, int pred_area) { return (double)v / (double)pred_area > 0.5; }

// pred_match / gt_match codes
constexpr int PN_FP = -1, PN_IGNORED = -2, PN_FN = -1, PN_CROWD = -2;
