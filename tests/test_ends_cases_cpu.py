"""The cases of the preprocessing and evaluation-tail edge tests (tests/ends_cases.py) without a GPU: every case lands on the kernel or
branch it names by the restated dispatch rule, the table covers every path, and the two oracles accept every case -- with the properties
the GPU tests rely on (clamped values at both ends, ties between nearest pixels, both branches of the four-pixel kernel in one launch)."""
import os
import re

import numpy as np
import pytest

import ends_cases as EC
from oracle import metrics_oracle as M
from oracle import preprocess_oracle as P
from camouflaged_vlm_amd import evaltail as E
from camouflaged_vlm_amd import hip

CSRC = os.path.join(os.path.dirname(os.path.abspath(hip.__file__)), "csrc")
BASE = 1 << 20                                                    # a 16-byte aligned address, as every case's buffers are


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_restated_rules_quote_the_sources():
    """the constants the restated predicates use are the ones the entry points compare against"""
    pre, ev = _src("preprocess.hip"), _src("evaltail.hip")
    assert "const int smem = (((W * C) + 31) & ~15) + 16 + (((n_out * C) + 31) & ~15) + 16;" in pre and "if (smem <= 60 * 1024)" in pre
    assert "if (axis == 1 && (C == 3 || C == 1) && (int64_t)N * H < (1 << 30))" in pre
    assert "if (axis == 0 && ((W * C) & 3) == 0 && (((uintptr_t)src | (uintptr_t)dst) & 3) == 0)" in pre
    assert "if (C == 3 && (cw & 3) == 0 && (((uintptr_t)dst) & 15) == 0)" in pre and "if ((((uintptr_t)p) & 3) == 0)" in pre
    assert "constexpr int WFM_SEG = 64, WFM_MAXSEG = 64;" in ev and "if (h <= WFM_SEG * WFM_MAXSEG)" in ev
    assert "const int smem_row = 4 * w * (int)sizeof(int);" in ev and "if (smem_row > 64 * 1024)" in ev
    assert len(re.findall(r"w > 8192 \|\| h > 16384", ev)) == 2                       # cvlm_mask_wfm and cvlm_prob_wfm
    assert ev.count("const bool vec = ((total & 15) == 0) &&") == 2                   # centroid and joint histogram


def test_every_resample_case_is_on_the_path_it_names():
    assert len({c.id for c in EC.RESAMPLE_CASES}) == len(EC.RESAMPLE_CASES)
    for c in EC.RESAMPLE_CASES:
        assert EC.resample_path(c.N, c.H, c.W, c.C, c.n_out, c.axis, BASE + c.src_off, BASE + c.dst_off) == c.path, c.id
    assert {c.path for c in EC.RESAMPLE_CASES} == set(EC.RESAMPLE_PATHS)
    for p in EC.RESAMPLE_PATHS:                                                        # saturation on every path
        assert any(c.pattern == "blocks" for c in EC.RESAMPLE_CASES if c.path == p), p
    for p, C in (("row3", 3), ("row1", 1)):
        row = [c for c in EC.RESAMPLE_CASES if c.path == p]
        assert {(c.W, c.n_out) for c in row} >= {(a, b) for a in (1, 2, 5, 16, 17, 341) for b in (1, 2, 5, 16, 17, 341)}
        assert {(c.src_off, c.dst_off) for c in row} >= {(1, 5), (7, 3), (15, 11)}
        # N = 3: source and destination rows at every offset modulo 16
        assert any(c.N == 3 and {(r * c.W * C) % 16 for r in range(c.N * c.H)} == set(range(16))
                   and {(r * c.n_out * C) % 16 for r in range(c.N * c.H)} == set(range(16)) for c in row), p
        # within 2 KB under the LDS bound, and a generic case within 1 KB over it
        assert any(EC.ROW_LDS_LIMIT - 2048 < EC.row_lds_bytes(c.W, C, c.n_out) <= EC.ROW_LDS_LIMIT for c in row), p
        assert any(c.C == C and EC.ROW_LDS_LIMIT < EC.row_lds_bytes(c.W, C, c.n_out) <= EC.ROW_LDS_LIMIT + 1024
                   for c in EC.RESAMPLE_CASES if c.path == "generic_h"), p
    assert {c.C for c in EC.RESAMPLE_CASES if c.path == "generic_h" and c.N == 2} >= {2, 4}
    col4 = {(c.H, c.n_out) for c in EC.RESAMPLE_CASES if c.path == "col4" and c.N == 3}
    assert col4 >= {(H, n) for H in (1, 2, 3, 61) for n in (1, 7, 128)}
    for key in (("src_off", 2), ("dst_off", 2)):                                       # the same shapes two bytes off: generic vertical
        off = {(c.H, c.n_out) for c in EC.RESAMPLE_CASES if c.path == "generic_v" and getattr(c, key[0]) == key[1] and (c.W * c.C) % 4 == 0}
        assert off >= col4 & {(H, n) for H in (1, 2, 3, 61) for n in (1, 7, 128)}
    assert any((c.W * c.C) % 4 != 0 and c.N == 2 for c in EC.RESAMPLE_CASES if c.path == "generic_v")


def test_oracle_accepts_every_resample_case():
    """tables exist for every filter of a case and the oracle's pass runs on them; the block patterns clamp at both ends on every path"""
    for c in EC.RESAMPLE_CASES:
        src = EC.resample_input(c)
        assert src.shape == (c.N, c.H, c.W, c.C) and src.dtype == np.uint8
        for filt in c.filters:
            b, k = EC.resample_tables(c, filt)
            assert b.shape == (c.n_out, 2) and k.shape[0] == c.n_out and (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= c.n_in).all(), (c.id, filt)
            assert (b[:, 1] <= k.shape[1]).all()
            if max(c.W, c.n_out) > 1000:
                continue                                                               # the long rows: run once, by the GPU test
            want = EC.resample_reference(c, filt)
            assert want.shape == c.out_shape and want.dtype == np.uint8
            if c.pattern == "blocks":
                raw = EC.resample_unclamped(src[0], b, k, c.axis)
                assert np.array_equal(np.clip(raw, 0, 255), want[0])
                lo, hi = float((raw < 0).mean()), float((raw > 255).mean())
                assert lo > 0.02 and hi > 0.02, (c.id, lo, hi)
    board = EC.resample_input(EC.Resample("row3", 1, 40, 40, 3, 61, 1, pattern="blocks"))[0]
    out = P.resize_u8(board, 97, 61, "bicubic")                                        # the whole resize of the pattern: mostly 0 and 255
    assert 0.15 < float((out == 0).mean()) < 0.5 and 0.15 < float((out == 255).mean()) < 0.5


def test_every_tensor_case_is_on_the_path_it_names():
    assert len({c.id for c in EC.TENSOR_CASES}) == len(EC.TENSOR_CASES)
    for c in EC.TENSOR_CASES:
        path, word, byte = EC.tensor_path(c.N, c.H, c.W, c.C, c.top, c.left, c.ch, c.cw, BASE + c.src_off, BASE + c.dst_off)
        assert path == c.path, (c.id, path)
        assert c.top >= 0 and c.left >= 0 and c.top + c.ch <= c.H and c.left + c.cw <= c.W
        if c.both_branches:
            assert word > 0 and byte > 0, (c.id, word, byte)
        assert EC.tensor_reference(c).shape == (c.N, c.C, c.ch, c.cw)
    assert {c.path for c in EC.TENSOR_CASES} == set(EC.TENSOR_PATHS)
    gen = [c for c in EC.TENSOR_CASES if c.path == "generic"]
    assert {c.C for c in gen} >= {1, 3, 4} and any(c.C == 3 and c.cw % 4 == 0 and c.dst_off % 16 for c in gen) and any(c.cw % 4 for c in gen)
    for p in EC.TENSOR_PATHS:
        mine = [c for c in EC.TENSOR_CASES if c.path == p]
        assert any(c.top > 0 for c in mine) and any(c.top + c.ch == c.H and c.left + c.cw == c.W and (c.top or c.left) for c in mine), p
    assert any(c.both_branches and c.N == 2 and c.W == 503 and c.left % 2 for c in EC.TENSOR_CASES)


def test_pipeline_images_reach_the_byte_branch():
    S, R = EC.PIPELINE_SIZES
    for h, w in EC.PIPELINE_IMAGES:
        rh, rw = P.clip_resize_shape(h, w, R)
        top, left = P.center_crop_box(rh, rw, R)
        assert rw % 2 == 1 or rh % 2 == 1
        assert (top > 0) != (left > 0)
        path, word, byte = EC.tensor_path(1, rh, rw, 3, top, left, R, R, BASE, BASE)
        assert path == ("x4_byte" if rw % 4 else "x4_word")
    assert any(P.clip_resize_shape(h, w, R)[1] % 2 for h, w in EC.PIPELINE_IMAGES)


def test_every_wfm_case_is_on_the_path_it_names():
    assert len({c.id for c in EC.WFM_CASES}) == len(EC.WFM_CASES)
    for c in EC.WFM_CASES:
        assert EC.wfm_paths(c.h, c.w) == (c.col, c.row), c.id
    assert {(c.col, c.row) for c in EC.WFM_CASES} >= {("segmented", "lds_le_64k"), ("segmented", "lds_gt_64k"), ("tall", "lds_le_64k")}
    assert {c.col for c in EC.WFM_CASES} == {"segmented", "tall"} and {c.row for c in EC.WFM_CASES} == {"lds_le_64k", "lds_gt_64k"}
    shapes = {(c.h, c.w) for c in EC.WFM_CASES}
    assert shapes >= {(65, 64), (64, 65), (1024, 3), (1025, 3), (4096, 65), (4097, 8), (4100, 70), (3, 4096), (3, 4097), (8, 8192), (1, 1), (7, 7),
                      (3, 200)}
    assert any(c.N == 2 and (c.h, c.w) == (4100, 70) for c in EC.WFM_CASES)
    for kind in ("first_row", "last_row"):
        assert {c.col for c in EC.WFM_CASES if c.gt == kind} == {"segmented", "tall"}
        assert {c.h for c in EC.WFM_CASES if c.gt == kind} == {4096, 4100}
    assert {c.gt for c in EC.WFM_CASES} >= {"alt_cols", "corner", "empty", "full", "pairs", "far_apart"}
    assert {(c.h, c.w) for c in EC.WFM_CASES if c.gt in ("empty", "full")} >= {(65, 70)}
    assert EC.wfm_paths(3, EC.WFM_MAX_W) is not None and EC.wfm_paths(EC.WFM_MAX_H, 2) is not None
    for h, w in EC.WFM_REFUSED:
        assert EC.wfm_paths(h, w) is None
    assert set(EC.WFM_REFUSED) == {(3, 8193), (16385, 2)}


def _ties(fg):
    """pixels with two or more foreground pixels at the least distance (brute force)"""
    ys, xs = np.nonzero(fg)
    yy, xx = np.mgrid[0:fg.shape[0], 0:fg.shape[1]]
    d = (yy.reshape(-1, 1) - ys[None, :]) ** 2 + (xx.reshape(-1, 1) - xs[None, :]) ** 2
    return int(((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())


@pytest.mark.parametrize("c", EC.WFM_CASES, ids=lambda c: c.id)
def test_oracle_accepts_every_wfm_case(c):
    """scipy's transform runs on every case, the pieces of `wfm_parts` give metrics_oracle.wfm's value back, and the nearest pixel scipy
    reports is the one the kernels' stated rule picks (smaller row inside a column, then smaller column) -- on every pixel, ties included:
    the GPU test compares d2 and Et on all of them."""
    pre, prob, gt = EC.wfm_input(c)
    assert pre.shape == prob.shape == gt.shape == (c.N, c.h, c.w)
    assert set(np.unique(gt)) <= {0, 128, 129, 255}
    for n in range(c.N):
        fg = gt[n] > 128
        pred, g = M.prepare_data(pre[n], gt[n])
        parts = EC.wfm_parts(pred, g)
        rule = EC.edt_kernel_rule(fg)
        if c.gt == "empty":
            assert parts is None and rule is None and M.wfm(pred, g) == 0.0
            continue
        assert fg.any() and (c.gt != "full" or fg.all())
        sums, d2, et = parts
        assert abs(EC.wfm_value(sums) - M.wfm(pred, g)) < 1e-12
        assert EC.wfm_value(sums) == E.wfm_from_sums(sums)
        assert abs(EC.wfm_value(sums, 0.3) - M.wfm(pred, g, beta=0.3)) < 1e-12
        rd2, iy, ix = rule
        assert np.array_equal(rd2, d2), c.id
        assert np.array_equal(np.abs(pred - 1)[iy, ix], et), c.id                      # scipy's pixel carries the rule's E: same tie order
        if c.gt in ("sparse", "pairs", "alt_cols") and c.h * c.w <= 20000 and c.h * c.w > 1:
            assert _ties(fg) > 0, c.id
    if c.gt == "pairs":                                                                # ties inside a column: a row midway between two
        fg = gt[0] > 128
        col = np.nonzero(fg[:, 0])[0]
        assert ((np.diff(col) % 2) == 0).any()
    if c.gt in ("first_row", "last_row", "far_apart"):                                 # nearest rows more than a segment away
        fg = gt[0] > 128
        _, iy, _ = EC.edt_kernel_rule(fg)
        assert int(np.abs(iy - np.arange(c.h)[:, None]).max()) > (250 if c.gt == "far_apart" else c.h - 2)


def test_wfm_prob_preparation_and_alternating_columns():
    c = next(c for c in EC.WFM_CASES if c.gt == "alt_cols")
    _, prob, gt = EC.wfm_input(c)
    fg = gt[0] > 128
    has = fg.any(axis=0)
    assert has[0] and not has[1::2].any() and not has[64:68].any() and has[::2].sum() > 40
    pn = EC.prob_prepared(prob[0])
    assert pn.dtype == np.float32 and pn.min() == 0 and pn.max() == 1
    assert np.array_equal(pn, M.prepare_data(prob[0] * 255, gt[0])[0])


def test_hist_cases_and_their_vector_predicate():
    assert len({c.id for c in EC.HIST_CASES}) == len(EC.HIST_CASES)
    for c in EC.HIST_CASES:
        vec = EC.hist_vec(c, BASE + c.off, BASE + c.off)
        assert all(vec) == c.vec and (c.vec or not any(vec[1:]) or c.h * c.w % 16), (c.id, vec)
        pre, gt = EC.hist_input(c)
        for n in range(c.N):
            stats, hist = EC.counts_numpy(pre[n], gt[n])
            assert int(hist.sum()) == c.h * c.w and (stats[0] > 0) == (c.gt != "empty")
            if c.gt in ("last_px", "last_row"):
                assert stats[2] == stats[0] * (c.h - 1)
            if c.gt in ("last_px", "last_col"):
                assert stats[1] == stats[0] * (c.w - 1)
    hw16 = [c for c in EC.HIST_CASES if c.h * c.w % 16 == 0]
    assert {c.off for c in hw16} >= {0, 1, 8} and any(c.N == 3 for c in hw16)
    assert any(c.N == 3 and c.h * c.w % 16 for c in EC.HIST_CASES)
    assert any(c.w < 16 and c.vec for c in EC.HIST_CASES) and any(c.w < 16 and not c.vec for c in EC.HIST_CASES)
    assert any(c.h * c.w < 16 for c in EC.HIST_CASES)
    assert any(c.pre == "flat" and ((c.h * c.w + 15) // 16) % 64 for c in EC.HIST_CASES)


def test_mask_logits_are_exact_under_the_sigmoid():
    for src in EC.MASK_SOURCES:
        lg = EC.mask_logits(src)
        assert lg.shape == (EC.MASK_N,) + src and set(np.unique(lg)) <= {-40.0, 0.0, 40.0}
        s = M.sigmoid_f32(lg)
        assert set(np.unique(s[lg == 40])) <= {np.float32(1)} and set(np.unique(s[lg == 0])) <= {np.float32(0.5)}
        assert (s[lg == -40] < 1e-17).all()
        for dst in EC.MASK_TARGETS:
            h, w = dst or src
            for n in range(EC.MASK_N):
                assert M.mask_to_u8(lg[n], h, w).shape == (h, w)
    assert len({v for src in EC.MASK_SOURCES for v in np.unique(EC.mask_logits(src)).tolist()}) == 3


def test_oracle_accepts_every_cod_case():
    for name in EC.COD_CASES:
        prob, gt = EC.cod_input(name)
        got = M.calc_cod(prob, gt)
        assert all(np.isfinite(v) for v in got), (name, got)
        for k in range(len(prob)):
            g = (gt[k, 0] * 255).astype(np.uint8)
            stats, hist, mom, pn, _ = EC.cod_counts_numpy(prob[k, 0], g)
            assert 0 < stats[0] < g.size and int(hist.sum()) == g.size
            assert hist.sum(axis=(1, 2)).min() >= 2, name                             # every S-measure quadrant holds two pixels or more
    p, _ = EC.cod_input("constant")
    assert p.min() == p.max()
    p, _ = EC.cod_input("two_values")
    assert len(np.unique(p)) == 2
    p, _ = EC.cod_input("8x8")
    assert p.shape[-2:] == (8, 8)
    p, _ = EC.cod_input("n3_ranges")
    rng = [(float(p[k].min()), float(p[k].max())) for k in range(3)]
    assert rng[0][1] < rng[1][0] and rng[2] == (0.0, 1.0)
