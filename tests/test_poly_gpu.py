"""COCO polygon annotations on the device: cvlm_mask_poly_decode against the definition in doubles
(tests/poly_oracle.py, itself held against the published counts loop in tests/test_poly_cpu.py) and against the host entry on every
shape and polygon kind, on thousands of random polygons per call, on the edges where a fused multiply-add would change the walk, on
unions ragged in one call and in rounds, and on every refusal; replay into used outputs; Cascade.polygons_decode, SizedMasks.concat
and the round trip through cvlm_mask_rle_emit_w; ground_truth= of Cascade.infer_classes / decode / the drop-in made of polygons and
crowd regions.  Everything is integers and compared exactly.

Figures of the MI355X run this file was written with are in DESIGN.md §21."""
import numpy as np
import pytest
import torch

import gt_oracle as GO
import poly_oracle as PO
import rle_oracle as RO
import sized_oracle as SO
from test_gt_gpu import CLASSES, OTHER, SIZES, cas, gold, record_reads, tiny          # noqa: F401 (fixtures)
from test_poly_cpu import (SQUARE, TRI, bound_items, check_concat, check_refusal, concat_parts, contraction_items, refusal_cases)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def entries():
    from camouflaged_vlm_amd import hip
    return hip.mask_poly_decode, hip.mask_poly_decode_host


def check_both(items, want=None, **over):
    """One device call and one host call for the items: both equal the definition, and each other."""
    dec, dec_host = entries()
    got = PO.check_items(dec, items, dev=DEV, want=want, **over)
    host = PO.check_items(dec_host, items, want=want, **{k: v for k, v in over.items() if k != "ws_planes"})
    assert all(np.array_equal(a, b) for a, b in zip(got, host))
    return got


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", PO.SHAPES)
def test_decode_equals_the_definition_and_the_host_entry(h, w):
    """Every polygon kind as one plane of one call; the 1500-vertex circle takes two passes of the check loop's 1024 threads; 130 x 517
    has 2 101 stream words, more than one slab of the prefix pass.  Without statistics and off a 16-byte boundary the bits are the same."""
    items = [([xy], h, w) for xy in PO.kinds(h, w).values()]
    got = check_both(items)
    bare, a, _, status = PO.run_poly(entries()[0], items, dev=DEV, stats=False)
    assert status == 0 and a is None and all(np.array_equal(x, y) for x, y in zip(bare, got))
    off16 = check_both(items, guard=GO.GUARD + 4)
    assert all(np.array_equal(x, y) for x, y in zip(off16, got))


def test_known_answers_and_bounds():
    items = [([list(map(float, xy))], h, w) for xy, h, w, _ in PO.KNOWN]
    check_both(items, want=[PO.known_plane(rows, h, w) for _, h, w, rows in PO.KNOWN])
    items, full = bound_items()
    check_both(items, want=[np.full((h, w), f) for (_, h, w), f in zip(items, full)])


@pytest.mark.parametrize("family", ["uniform", "tenths", "ints"])
def test_random_polygons_in_one_call(family):
    """3000 planes of at most 40 x 40 in one launch sequence: the contraction test -- a fused ys + s * t shows here."""
    PO.check_items(entries()[0], PO.random_family(family, 3000, seed=5), dev=DEV)


def test_edges_a_fused_multiply_add_would_change():
    """The edges tests/test_poly_cpu.py finds with exact rationals: the definition's plane has pixel (0, 1) clear, a fused walk sets it."""
    items = contraction_items()
    assert len(items) == 6
    got = check_both(items)
    assert all(not np.unpackbits(g, axis=1)[0, 1] for g in got)


def test_unions_ragged_and_in_rounds():
    """2, 3 and 17 polygons per plane, overlapping, disjoint and nested, ragged with single-polygon planes in one call; a workspace of
    exactly one slot makes nine rounds of the nine planes, one of two slots five."""
    items = PO.union_items()
    whole = check_both(items)
    one = check_both(items, ws_planes=1)
    two = check_both(items, ws_planes=2)
    assert all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(whole, one, two))
    polys, h, w = items[3]
    assert np.array_equal(whole[3], SO.pack_rows(PO.plane_of(polys[0], h, w))) and whole[7].any()      # OR, not XOR


@pytest.mark.parametrize("name", list(refusal_cases()))
def test_decode_refuses_whole_planes(name):
    """status 1, the refused plane zero -- or untouched where its table is at fault --, area 0, box -1, its neighbours whole and every
    band untouched; the host entry refuses the same planes."""
    dec, dec_host = entries()
    got, area, box = check_refusal(dec, name, dev=DEV)
    _, h_area, h_box = check_refusal(dec_host, name)
    assert np.array_equal(area, h_area) and np.array_equal(box, h_box)


def test_decode_replays_into_used_outputs():
    """Every output is initialised by the call: a second call into the same tensors, and one after a call that refused a plane -- in
    its second polygon, when its accumulator already held the first --, gives the same bytes.  A workspace of three slots: rounds."""
    from camouflaged_vlm_amd import hip
    items = PO.union_items()
    sizes = [(h, w) for _, h, w in items]
    d, off, _, _ = SO.tables(sizes, 0)
    flat, po, pp = PO.tables(items, W=0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    P, mp = len(items), max(h * w for h, w in sizes)
    bits = torch.empty(int(off[-1]), dtype=torch.uint8, device=DEV)
    area, box, status = (torch.empty(s, dtype=torch.int32, device=DEV) for s in ((P,), (P, 4), (1,)))
    ws = torch.empty(hip.mask_poly_decode_workspace_bytes(3, mp), dtype=torch.uint8, device=DEV)
    bad = flat.copy()
    bad[int(po[1])] = np.nan
    seen = []
    for xy in (flat, flat, bad, flat):
        hip.mask_poly_decode(t(xy), t(po), t(pp), t(d), t(off), mp, bits, area, box, status, ws)
        seen.append((bits.cpu().numpy().copy(), area.cpu().tolist(), box.cpu().tolist(), status.item()))
    assert [s[3] for s in seen] == [0, 0, 1, 0] and seen[2][1][0] == 0 and seen[0][1][0] > 0
    for s in (seen[1], seen[3]):
        assert np.array_equal(s[0], seen[0][0]) and s[1:] == seen[0][1:]
    for p, (polys, h, w) in enumerate(items):
        lo, hi = int(off[p]), int(off[p + 1])
        assert np.array_equal(seen[0][0][lo:hi].reshape(h, -1), SO.pack_rows(PO.expected(polys, h, w)))


# ---- Python ----------------------------------------------------------------------------------------------------------------------------------------
LAUNCHERS = ("gemm", "layernorm", "topk_select", "patchify", "split_f32", "expand_blocks", "bilinear", "mask_pack", "mask_pack_sized",
             "mask_rle_count", "mask_rle_emit", "mask_rle_count_w", "mask_rle_emit_w", "mask_overlap", "mask_rle_decode", "mask_inter_sized",
             "mask_poly_decode")


def test_polygons_decode_round_trip_and_concat(cas, monkeypatch):
    """polygons_decode launches without a synchronisation; its planes are the definition's; rle_decode(mask_rle_sized(.)) gives them
    back; concat of two calls and of a call with rle_decode's planes equals decoding the joined list."""
    from camouflaged_vlm_amd.engine import SizedMasks
    anns, rles, truth = concat_parts()
    torch.cuda.synchronize()
    reads = record_reads(monkeypatch)
    whole = cas.polygons_decode(anns)
    monkeypatch.undo()
    assert reads == [], reads
    assert isinstance(whole, SizedMasks) and whole.level == 0 and whole.sizes == [tuple(a["size"]) for a in anns] and whole.status.numel() == 1
    whole.check()
    for p, (polys, h, w) in enumerate(PO.union_items()):
        m = PO.expected(polys, h, w)
        assert np.array_equal(whole.to_numpy(p), m) and int(whole.area[p]) == int(m.sum()) and whole.box[p].tolist() == SO.stats(m)[1]
    bare = cas.polygons_decode(anns, stats=False)
    assert bare.area is None and bare.box is None and torch.equal(bare.bits, whole.bits)
    back = cas.rle_decode(cas.mask_rle_sized(whole))
    back.check()
    assert torch.equal(back.bits, whole.bits) and torch.equal(back.area, whole.area) and torch.equal(back.box, whole.box)
    a, b, c = cas.polygons_decode(anns[:4]), cas.polygons_decode(anns[4:]), cas.rle_decode(rles)
    reads = record_reads(monkeypatch)
    joined = SizedMasks.concat([a, b])
    mixed = SizedMasks.concat([b, c, a])
    monkeypatch.undo()
    assert reads == [], reads
    check_concat(joined, [a, b], whole)
    check_concat(mixed, [b, c, a], None)
    for q, m in enumerate(truth):
        assert np.array_equal(mixed.to_numpy(len(b.sizes) + q), m)
    o = cas.mask_inter_sized(mixed, mixed, pairs=[(p, p) for p in range(len(mixed.sizes))])
    assert torch.equal(o.inter, mixed.area) and o.status.item() == 0


def test_bad_polygon_requests_raise_and_launch_nothing(cas):
    from camouflaged_vlm_amd import hip
    ok = {"size": [20, 30], "polygons": [TRI]}
    one = lambda **kw: [dict(ok, **kw)]
    calls = []
    saved = {n: getattr(hip, n) for n in LAUNCHERS}
    for n in saved:
        setattr(hip, n, lambda *a, _n=n, **k: calls.append(_n))
    try:
        for bad in (None, [], "ab", ok, [ok, 5], one(size=[0, 3]), one(size=[2, 16385]), one(size=[2.0, 3]), one(polygons=[]), one(polygons=TRI),
                    one(polygons=[TRI] * 4097), one(polygons=[TRI[:4]]), one(polygons=[TRI + [1.0]]), one(polygons=[[1.0, 2.0] * 65536]),
                    one(polygons=[[0.5, float("nan"), 1, 1, 2, 2]]), one(polygons=[[0.5, float("inf"), 1, 1, 2, 2]]),
                    one(polygons=[[0.5, 65536.5, 1, 1, 2, 2]]), one(polygons=[["1", "2", "3", "4", "5", "6"]]), one(polygons=[[True, 1, 2, 2, 3, 3]]),
                    one(polygons=[TRI, SQUARE, [65536.0, -65536.0, -65536.0, 65536.0] * 1500]), [ok] * 65536):
            with pytest.raises(ValueError):
                cas.polygons_decode(bad)
    finally:
        for n, f in saved.items():
            setattr(hip, n, f)
    assert calls == []
    good = cas.polygons_decode([ok])
    good.check()
    assert int(good.area[0]) == int(PO.plane_of(TRI, 20, 30).sum())


# ---- tiny geometry, exact ----------------------------------------------------------------------------------------------------------------------
def annotations(sizes, ids):
    """Per entry of ids an annotation at the size of its image: polygons -- a 40-gon and a triangle that overlaps it -- for the first
    and the last, a crowd region in run counts for those between -> (bool planes, the polygon annotations with their places, the
    run-length annotations with theirs)."""
    truth, polys, crowd = [], [], []
    for n, b in enumerate(ids):
        h, w = sizes[b]
        if n in (0, len(ids) - 1):
            ps = [PO.circle(40, w * 0.5, h * (0.4 + 0.1 * n), min(h, w) * (0.45 - 0.1 * n)), [w * 0.1, h * 0.2, w * 0.7, h * 0.5, w * 0.2, h * 0.9]]
            truth.append(PO.expected(ps, h, w))
            polys.append((n, {"size": [h, w], "polygons": ps}))
        else:
            m = np.zeros((h, w), dtype=bool)
            m[h // 5:h // 2, w // 4:w - 7] = True
            truth.append(m)
            crowd.append((n, {"size": [h, w], "counts": RO.plane_counts(m).tolist()}))
    return truth, polys, crowd


def check_call(cas, call, sizes, ids, K: int, masks: str = "bits"):
    """`call(**kw)` runs one entry point: with ground_truth= made of polygons_decode's and rle_decode's planes joined by concat -- the
    image ids reordered with them -- the result's `gt_overlaps` is the oracle on the call's own sized bits and every other field keeps
    the bits of the call without it.  -> the result."""
    from camouflaged_vlm_amd.engine import SizedMasks
    truth, polys, crowd = annotations(sizes, ids)
    gt = SizedMasks.concat([cas.polygons_decode([a for _, a in polys]), cas.rle_decode([a for _, a in crowd])])
    gt.check()
    order = [n for n, _ in polys] + [n for n, _ in crowd]
    truth, ids = [truth[n] for n in order], [ids[n] for n in order]
    plain = call(masks=masks, sizes=sizes, rle="sized")
    assert plain.gt_overlaps is None
    keep = {f: getattr(plain, f).clone() for f in OTHER if getattr(plain, f) is not None}
    keep.update({"sized." + f: getattr(plain.sized, f).clone() for f in ("bits", "area", "box", "offsets")})
    keep.update({"rle." + f: getattr(plain.rle, f).clone() for f in ("counts", "offsets", "n_runs")})
    h = call(masks=masks, sizes=sizes, rle="sized", ground_truth=(gt, ids))
    torch.cuda.synchronize()
    for f in OTHER:
        assert (getattr(h, f) is None) == (f not in keep), f
    for f, t in keep.items():                                                     # bit for bit, floats included
        obj = h
        for part in f.split("."):
            obj = getattr(obj, part)
        assert torch.equal(obj.contiguous().view(torch.uint8), t.contiguous().view(torch.uint8)), f
    o = h.gt_overlaps
    o.check()
    pairs = [(p, q) for p in range(len(sizes) * K) for q in range(len(ids)) if ids[q] == p // K]
    assert o.pairs.cpu().tolist() == [list(p) for p in pairs]
    got = [h.sized.to_numpy(p) for p in range(len(h.sized.sizes))]
    want = GO.inter_oracle(got, truth, pairs)
    assert np.array_equal(o.inter.cpu().numpy(), want) and want.min() >= 0
    assert o.area_a.cpu().tolist() == [int(got[p].sum()) for p, _ in pairs] and o.area_b.cpu().tolist() == [int(truth[q].sum()) for _, q in pairs]
    assert np.array_equal(o.iou(), GO.iou_formula(want, o.area_a.cpu().tolist(), o.area_b.cpu().tolist(), [False] * len(pairs)))
    return h


def test_infer_classes_ground_truth_of_polygons(tiny, cas, monkeypatch):
    _, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    classes = torch.tensor(CLASSES)
    call = lambda **kw: cas.infer_classes(inp, ci, cm, classes=classes, **kw)
    both = check_call(cas, call, SIZES, [0, 0, 1], 3, "both")
    bits = check_call(cas, call, SIZES, [0, 0, 1], 3, "bits")
    assert torch.equal(bits.gt_overlaps.inter, both.gt_overlaps.inter) and int(both.gt_overlaps.inter.max()) > 0


def test_decode_ground_truth_of_polygons(tiny, cas, monkeypatch):
    _, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    enc = cas.encode(inp, ci, cm)
    sizes = [SIZES[1], SIZES[0], SIZES[1]]                                        # one per decoded row
    check_call(cas, lambda **kw: cas.decode(enc, topk=3, images=[1, 0, 1], **kw), sizes, [1, 1, 2], 3, "both")
    check_call(cas, lambda **kw: cas.decode(enc, topk=3, images=[1, 0, 1], **kw), sizes, [2, 0, 0], 3, "bits")


def test_dropin_decodes_polygons(tiny, gold, golden_dir):
    import os
    import sys

    import camouflaged_vlm_amd as cv
    if cv.DROPIN_DIR not in sys.path:
        sys.path.insert(0, cv.DROPIN_DIR)
    import models
    from cocotrainers.mapleAlphaCLIP import CustomCLIP
    g, c, sd_np, (inp, ci, cm), dev = tiny
    with np.load(os.path.join(golden_dir, "tiny_cascade.npz")) as z:
        eot_train = z["eot_train"].tolist()
    clip = CustomCLIP(geometry=c, eot_train=eot_train, eot_test=gold["eot_test"].tolist())
    enc_cfg = dict(name="sam", img_size=g.inp_size, mlp_ratio=4, patch_size=16, qkv_bias=True, use_rel_pos=True,
                   window_size=14, out_chans=256, scale_factor=32, input_type="fft", freq_nums=0.25, prompt_type="highpass",
                   prompt_embed_dim=256, tuning_stage=1234, handcrafted_tune=True, embedding_tune=True, adaptor="adaptor",
                   embed_dim=g.embed_dim, depth=g.depth, num_heads=g.num_heads, global_attn_indexes=list(g.global_attn_indexes))
    model = models.make({"name": "sam_maskdecoder_edge", "args": {"inp_size": g.inp_size, "loss": "iou", "encoder_mode": enc_cfg}}).cuda()
    model.train_text_features = model.train_text_features[:c.n_cls_train]
    model.test_text_features = model.test_text_features[:c.n_cls_test]
    model.load_mapleAlphaCLIP(clip)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    model.eval()
    model.cascade().class_chunk = lambda: 4
    with torch.no_grad():
        check_call(model, lambda **kw: model.infer_classes(inp, ci, cm, topk=3, **kw), SIZES, [0, 0, 1], 3, "both")
        enc = model.encode_images(inp, ci, cm)
        check_call(model, lambda **kw: model.decode_classes(enc, topk=3, **kw), SIZES, [1, 0, 1], 3, "bits")
