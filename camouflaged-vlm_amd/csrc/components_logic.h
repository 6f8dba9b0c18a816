// Connected components of packed masks: the per-thread logic of cvlm_mask_components, written once for the device
// kernels (components.hip) and for the sequential host entry cvlm_debug_mask_components_host, which runs these same functions word by
// word on the CPU.  No HIP call, no allocation.  cvlm_mask_holes runs the same logic on the complement: see cc_fetch.
//
// A plane is H rows of W / 32 words; a word never straddles a row.  In memory a word is in numpy.packbits' order (what cvlm_mask_pack
// stores); cc_unpack (maskbits.h) turns it into bit i = pixel i of the word, so that a horizontal RUN is a maximal group of consecutive
// set bits.  Every run is named by the plane index of its first pixel.  Two runs never start on adjacent pixels (inside a word a clear bit
// separates them; a word boundary separates an odd index from the next even one), so run start i owns slot i >> 1 of three arrays of
// H * W / 2 entries: parent (union-find), area and box.  Invariant of the forest: parent[i >> 1] <= i, and equal exactly at a root, so
// the root of a region is its lowest run start -- its lowest pixel index, the `seed` of the interface.
#pragma once
#include <stdint.h>

#include "maskbits.h"

struct cc_box { int x0, y0, x1, y1; };                            // inclusive; 16 bytes

// ---- runs of a word ---------------------------------------------------------------------------------------------------------------------
// bits [s, e) of a word, 0 <= s < e <= 32
CC_HD uint32_t cc_span(int s, int e) { return (e >= 32 ? 0xffffffffu : (1u << e) - 1u) & ~((1u << s) - 1u); }
// the run of `w` that holds set bit b: its first bit, and one past its last
CC_HD int cc_run_start(uint32_t w, int b) {
    const uint32_t zeros_below = ~w & ((1u << b) - 1u);
    return zeros_below ? 32 - __builtin_clz(zeros_below) : 0;
}
CC_HD int cc_run_end(uint32_t w, int b) {
    const uint32_t zeros_above = b >= 31 ? 0u : (~w & (0xffffffffu << (b + 1)));
    return zeros_above ? __builtin_ctz(zeros_above) : 32;
}
// the lowest run of a non-zero `rest` (what is left of `w` once the runs below have been taken off): [s, e); takes it off `rest`
CC_HD void cc_next_run(uint32_t w, uint32_t& rest, int& s, int& e) {
    s = __builtin_ctz(rest);
    e = cc_run_end(w, s);
    rest &= ~cc_span(s, e);
}

// ---- union-find -----------------------------------------------------------------------------------------------------------------------
// While the join pass runs, other threads lower parents at any time.  A value read here may be out of date but is always an ancestor
// the node had: every change replaces a parent by a lower member of the same final region.  Loads go to the coherent level (L2).
CC_HD int cc_load(const int* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return *p;
#endif
}
CC_HD int cc_atomic_min(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicMin(p, v);
#else
    const int old = *p;
    if (v < old) *p = v;
    return old;
#endif
}

// Root of run start i.  Every iteration lowers i (parent <= i, and != i here): at most i steps, no waiting on anyone.
CC_HD int cc_find(const int* parent, int i) {
    for (int p = cc_load(parent + (i >> 1)); p != i; p = cc_load(parent + (i >> 1))) i = p;
    return i;
}

// Join the regions of run starts a and b.  The larger of the two roots is pointed at the smaller by an atomic minimum; if that node
// had meanwhile stopped being a root the minimum returns its other parent `old` < a, whose region must now meet b's as well: go on
// from there.  Every iteration lowers a or b; nothing waits.
CC_HD void cc_union(int* parent, int a, int b) {
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }             // a is the larger
        const int old = cc_atomic_min(parent + (a >> 1), b);
        if (old == a) return;                                      // a was a root and now hangs below b
        a = cc_find(parent, old);                                  // old < a
        b = cc_find(parent, b);
    }
}

// ---- the word fetch -------------------------------------------------------------------------------------------------------------------
// Every pass reads its words through cc_fetch.  flip = 0 (CC_SET) labels the SET pixels, cvlm_mask_components; flip = ~0 (CC_CLEAR)
// labels the CLEAR ones, the background regions of cvlm_mask_holes: the same runs, rule and forest on the complement.
// W % 32 == 0, so a complemented word has no tail bits to mask.
constexpr uint32_t CC_SET = 0u, CC_CLEAR = 0xffffffffu;
CC_HD uint32_t cc_fetch(const uint32_t* bits, int wi, uint32_t flip) { return cc_unpack(bits[wi]) ^ flip; }

// ---- pass 1: every run of word wi becomes a region of its own ----------------------------------------------------------------------------
// bits: the plane's stored words; wi = y * wpr + c.
CC_HD void cc_seed_word(const uint32_t* bits, int wi, int wpr, int* parent, int* area, cc_box* box, uint32_t flip = CC_SET) {
    const uint32_t w = cc_fetch(bits, wi, flip);
    const int y = wi / wpr, xw = (wi - y * wpr) * 32, base = wi * 32;
    for (uint32_t rest = w; rest;) {
        int s, e;
        cc_next_run(w, rest, s, e);
        const int k = (base + s) >> 1;
        parent[k] = base + s;
        area[k] = e - s;
        box[k] = cc_box{xw + s, y, xw + e - 1, y};
    }
}

// ---- pass 2: the neighbour rule ---------------------------------------------------------------------------------------------------------
// Word wi joins (a) its run at bit 0 with the run at bit 31 of the previous word of the row, (b) each of its runs with every run of
// the word above that it touches -- shares a column with (4), or a column or a diagonal (8: the run widened by one bit each way) --,
// and (c) for 8, its corner bits with the facing corner bit of the words above-left and above-right, unless the word above already
// links them.  Runs of the row above that continue into neighbouring words are joined there by (a) of their own words.
CC_HD void cc_join_word(const uint32_t* bits, int wi, int wpr, int connectivity, int* parent, uint32_t flip = CC_SET) {
    const uint32_t w = cc_fetch(bits, wi, flip);
    if (!w) return;
    const int y = wi / wpr, c = wi - y * wpr, base = wi * 32;
    if ((w & 1u) && c > 0) {
        const uint32_t left = cc_fetch(bits, wi - 1, flip);
        if (left >> 31) cc_union(parent, base, base - 32 + cc_run_start(left, 31));
    }
    if (y == 0) return;
    const uint32_t up = cc_fetch(bits, wi - wpr, flip);
    const int ubase = base - wpr * 32;
    for (uint32_t rest = w; rest && up;) {
        int s, e;
        cc_next_run(w, rest, s, e);
        uint32_t reach = cc_span(s, e);
        if (connectivity == 8) reach |= reach << 1 | reach >> 1;
        for (uint32_t t = reach & up; t;) {
            const int b = __builtin_ctz(t), us = cc_run_start(up, b), ue = cc_run_end(up, b);
            cc_union(parent, base + s, ubase + us);
            t &= ~cc_span(us, ue);
        }
    }
    if (connectivity != 8) return;
    if ((w & 1u) && c > 0 && !(up & 1u)) {
        const uint32_t ul = cc_fetch(bits, wi - wpr - 1, flip);
        if (ul >> 31) cc_union(parent, base, ubase - 32 + cc_run_start(ul, 31));
    }
    if ((w >> 31) && c < wpr - 1 && !(up >> 31)) {
        const uint32_t ur = cc_fetch(bits, wi - wpr + 1, flip);
        if (ur & 1u) cc_union(parent, base + cc_run_start(w, 31), ubase + 32);
    }
}

// ---- pass 4: the order of the table -------------------------------------------------------------------------------------------------------
// Larger area first, ties to the lower seed: one 64-bit key, larger = earlier.  A region has area >= 1, so key 0 means "none".
CC_HD uint64_t cc_rank_key(int area, int seed) { return ((uint64_t)(uint32_t)area << 32) | (uint32_t)(0x7fffffff - seed); }
CC_HD int cc_key_seed(uint64_t key) { return 0x7fffffff - (int)(uint32_t)key; }

// ---- pass 5: the kept word ----------------------------------------------------------------------------------------------------------------
// Word wi with every run cleared whose region has fewer than min_area pixels.  parent is flat by now: a run start's parent is its root.
CC_HD uint32_t cc_keep_word(uint32_t w, int base, const int* parent, const int* area, int min_area) {
    uint32_t kept = w;
    for (uint32_t rest = w; rest;) {
        int s, e;
        cc_next_run(w, rest, s, e);
        const int root = parent[(base + s) >> 1];
        if (area[root >> 1] < min_area) kept &= ~cc_span(s, e);
    }
    return kept;
}

// ---- holes ----------------------------------------------------------------------------------------------------------------
// A background region is a hole exactly when its box misses the plane's border.
CC_HD bool cc_box_inside(const cc_box& b, int H, int W) { return b.x0 > 0 && b.y0 > 0 && b.x1 < W - 1 && b.y1 < H - 1; }
// The dual: foreground connectivity 8 makes the background 4-connected, and the reverse.
CC_HD int cc_dual(int connectivity) { return connectivity == 8 ? 4 : 8; }

// The bits of word wi that filling adds: every run of w = the word's CLEAR pixels whose region is a hole of fewer than fill_below
// pixels.  parent is flat by now.
CC_HD uint32_t cc_fill_word(uint32_t w, int base, const int* parent, const int* area, const cc_box* box, int H, int W, int fill_below) {
    uint32_t add = 0u;
    for (uint32_t rest = w; rest;) {
        int s, e;
        cc_next_run(w, rest, s, e);
        const int k = parent[(base + s) >> 1] >> 1;
        if (area[k] < fill_below && cc_box_inside(box[k], H, W)) add |= cc_span(s, e);
    }
    return add;
}
