// Packed edge maps: the per-pixel logic of cvlm_edge_pack, written once for the device kernel (edgepack.hip) and for the
// sequential host entry cvlm_debug_edge_pack_host, which runs these same functions pixel by pixel on the CPU.  No HIP call, no
// allocation.
//
// v(y, x) is the align_corners = False bilinear value of a plane at an output pixel, in float32 with one rounding per written
// operation: `#pragma clang fp contract(off)` covers the coordinate AND the blend, so no product is fused into a sum and the value is a
// function of this text, not of the compiler (bilinear_kernel of rowops.hip pins the coordinate only; its blend is the compiler's).
//   s      = (float)n_in / (float)n_out, divided ON THE HOST by the launcher and handed to the kernel
//   f(o)   = max(s * ((float)o + 0.5f) - 0.5f, 0)                the product rounded before the subtraction
//   i0     = (int)f, i1 = i0 + (i0 < n_in - 1), l = f - (float)i0
//   row(y') = (1 - lx) * p[y'][x0] + lx * p[y'][x1]
//   v      = (1 - ly) * row(y0) + ly * row(y1)
// The same formulas shrink a plane (n_out < n_in): two taps per axis, no area averaging.  i0 is capped at n_in - 1: a float32
// coordinate stops resolving single pixels beyond 2^22 of them per row, and there the cap, not the cast, keeps the index inside the
// plane; wherever (int)f is a pixel of the plane the cap changes nothing.
#pragma once
#include <stdint.h>

#include "maskbits.h"

#define EP_HD CC_HD

// The tile of one workgroup: EP_TW output columns (a wave's 64 lanes x 4 pixels: 8 words) x EP_TH output rows, and the floats of LDS
// the staged instance may fill with a tile's source footprint: 19 KiB, eight workgroups to a CU's 160 KiB.  The model's 4 x reads
// 66 x 18 = 1188 floats per tile, 2 x 130 x 34 = 4420 (ep_fits_lds bounds it by 132 x 36 = 4752); from scale 1 on the direct instance runs.
constexpr int EP_TW = 256, EP_TH = 64, EP_LDS_FLOATS = 4864;

struct ep_tap { int i0, i1; float l; };

EP_HD float ep_src(float scale, int o) {
#pragma clang fp contract(off)
    const float f = scale * ((float)o + 0.5f) - 0.5f;
    return f < 0.f ? 0.f : f;
}

EP_HD ep_tap ep_coord(float scale, int o, int n_in) {
    const float f = ep_src(scale, o);
    ep_tap t;
    t.i0 = f >= (float)(n_in - 1) ? n_in - 1 : (int)f;
    t.i1 = t.i0 + (t.i0 < n_in - 1 ? 1 : 0);
    t.l = f - (float)t.i0;
    return t;
}

EP_HD float ep_lerp(float l, float a, float b) {
#pragma clang fp contract(off)
    const float wa = 1.0f - l;
    const float pa = wa * a;
    const float pb = l * b;
    return pa + pb;
}

EP_HD float ep_value(float v00, float v01, float v10, float v11, float lx, float ly) {
    return ep_lerp(ly, ep_lerp(lx, v00, v01), ep_lerp(lx, v10, v11));
}

// NaN compares false, +inf true
EP_HD uint32_t ep_above(float v, float threshold) { return v > threshold ? 1u : 0u; }

// The source indices the output indices [o_first, o_last] read along one axis: [lo, hi], both inside [0, n_in).  f is monotone in o.
EP_HD void ep_footprint(float scale, int o_first, int o_last, int n_in, int& lo, int& hi) {
    lo = ep_coord(scale, o_first, n_in).i0;
    hi = ep_coord(scale, o_last, n_in).i1;
}

// The launcher's choice between the two instances, a pure function of the four (positive) sizes: true when a bound on the source
// footprint of any tile fits EP_LDS_FLOATS.  Along one axis a tile of T outputs reads at most floor(f_last) + 1 - floor(f_first) + 1
// <= ceil(s (T - 1)) + 2 source indices; + 3 on s T covers the roundings of f, and the plane's own size caps it.  The bound decides
// speed only: a workgroup of the staged instance measures its own footprint and reads the plane directly if it is larger.
inline bool ep_fits_lds(int hin, int win, int hout, int wout) {
    const double sy = (double)hin / hout, sx = (double)win / wout;
    int64_t cols = (int64_t)(sx * EP_TW) + 4, rows = (int64_t)(sy * EP_TH) + 4;   // floor + 1 >= ceil
    if (cols > win) cols = win;
    if (rows > hin) rows = hin;
    return cols * rows <= EP_LDS_FLOATS;
}
