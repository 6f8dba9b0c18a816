"""Boundary IoU and Boundary AP on the device: cvlm_mask_boundary_sized against the window definition
(tests/boundary_oracle.py) and against the host entry, bit for bit and count for count, on every width that crosses a word or a
64-pixel chunk, heights below and above the 32 rows a wave loads at once, every radius around 2 d + 1 = min(h, w), a radius of 463,
planes that span several row segments with runs that end at a seam, ragged planes in one call, guard bands, used outputs, a NULL
area, dirty pad bits and every refusal; cvlm_coco_match_boundary against the published loops over min(mask IoU, boundary IoU) and
against its host entry; Cascade.mask_boundary_sized / coco_match(boundary=) and the drop-in on the tiny cascade, where Boundary AP is
the oracle's to the last bit and differs from the mask AP of the same data.

Figures of the MI355X run this file was written with are in DESIGN.md §25."""
import numpy as np
import pytest
import torch

import boundary_oracle as BO
import match_oracle as MO
import rle_oracle as RO
import test_boundary_cpu as CPU
from test_labels_gpu import tracer  # noqa: F401  (fixture)
from test_match_cpu import SMALL_RNGS, ragged_groups, refusal_cases, shape_cases
from test_match_gpu import CLASSES, SIZES, cas, dropin, gold, oracle_groups, record_reads, tiny  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TABLES = CPU.TABLES


def entries():
    from camouflaged_vlm_amd import hip
    return hip.mask_boundary_sized, hip.mask_boundary_sized_host


def match_entries():
    from camouflaged_vlm_amd import hip
    return hip.coco_match_boundary, hip.coco_match_boundary_host


def same_bytes(res, host, area=True):
    for p, (a, b) in enumerate(zip(res["raw"], host["raw"])):
        assert np.array_equal(a, b), p
    assert not area or np.array_equal(res["area"], host["area"])
    assert res["status"] == host["status"]


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", BO.HEIGHTS)
def test_device_equals_the_oracle_and_the_host_entry(h):
    """Every width, every radius of the list and every content at one height; the planes of one width are ONE call, each plane at its
    own radius."""
    dev_fn, host_fn = entries()
    for w in BO.WIDTHS:
        named = BO.contents(h, w, seed=1000 * h + w)
        planes, radii = [], []
        for d in BO.radii_of(h, w):
            planes += [m for _, m in named]
            radii += [d] * len(named)
        res = BO.run(dev_fn, planes, radii, dev=DEV)
        assert res["status"] == 0
        BO.check(res, planes, radii)
        same_bytes(res, BO.run(host_fn, planes, radii))


def test_large_radius_and_row_segments():
    """40 x 1100 at d = 463 (nothing is eroded: 2 d + 1 > h); 389 rows at d = 3 and d = 1 (segments of 128 rows: seams at 128, 256, 384,
    a run that ends exactly at one and a run that starts at one); 500 rows at d = 40 (segments of 160 rows, four of them)."""
    rng = np.random.default_rng(27)
    wide = rng.random((40, 1100)) < 0.999
    wide[:, 5:1000] = True
    tall = np.zeros((389, 70), dtype=bool)
    tall[100:256, 2:60] = True
    tall[256:300, 30:69] = True
    tall[380:389, :] = True
    taller = rng.random((500, 40)) < 0.995
    taller[100:320] = True
    planes, radii = [wide, tall, taller, tall], [463, 3, 40, 1]
    dev_fn, host_fn = entries()
    res = BO.run(dev_fn, planes, radii, dev=DEV)
    assert res["status"] == 0
    BO.check(res, planes, radii)
    same_bytes(res, BO.run(host_fn, planes, radii))
    assert res["area"][0] == wide.sum() and 0 < res["area"][1] < tall.sum()


def test_ragged_planes_used_outputs_null_area_and_an_unaligned_base():
    planes, radii = CPU.ragged_planes()
    dev_fn, host_fn = entries()
    res = BO.run(dev_fn, planes, radii, dev=DEV)
    assert res["status"] == 0
    BO.check(res, planes, radii)
    other = [~p for p in planes]
    again = BO.run(dev_fn, other, radii, dev=DEV, outs=res["outs"])                    # into used outputs and a used workspace
    assert again["status"] == 0
    BO.check(again, other, radii)
    bare = BO.run(dev_fn, planes, radii, dev=DEV, area=False, shift=4, dirty_pads=True)       # bits 4 bytes off a 16-byte boundary
    assert bare["status"] == 0
    BO.check(bare, planes, radii, area=False)
    same_bytes(bare, BO.run(host_fn, planes, radii, area=False, shift=4, dirty_pads=True), area=False)


@pytest.mark.parametrize("name", [c[0] for c in CPU.refusals()[1]])
def test_refuses_whole_planes(name):
    sizes, cases = CPU.refusals()
    _, kw, radii, refused, untouched = next(c for c in cases if c[0] == name)
    rng = np.random.default_rng(29)
    planes = [rng.random(s) < 0.9 for s in sizes]
    dev_fn, host_fn = entries()
    res = BO.run(dev_fn, planes, radii, dev=DEV, **kw)
    assert res["status"] == 1
    BO.check(res, planes, radii, refused=refused, untouched=untouched)
    same_bytes(res, BO.run(host_fn, planes, radii, **kw))
    whole = BO.run(dev_fn, planes, [1] * 4, dev=DEV, outs=res["outs"])                  # the status is zeroed again
    assert whole["status"] == 0
    BO.check(whole, planes, [1] * 4)


def test_every_badarg_leaves_the_device_alone():
    CPU.test_every_badarg_of_the_boundary_entry()
    CPU.test_every_badarg_of_the_boundary_matching()
    torch.cuda.synchronize()


# ---- the matching -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in shape_cases()])
def test_boundary_matching_equals_the_oracle_and_the_host_entry(name):
    _, groups, kw = next(c for c in shape_cases() if c[0] == name)
    groups = [BO.with_boundary(g, 700 + i) for i, g in enumerate(groups)]
    dev_fn, host_fn = match_entries()
    res = BO.run_match(dev_fn, groups, dev=DEV, guard=16, **kw)
    assert res["status"] == 0
    BO.check_groups(res, groups, **kw)
    host = BO.run_match(host_fn, groups, **kw)
    again = BO.run_match(dev_fn, groups, dev=DEV, outs=res["outs"], **kw)             # a second call into used outputs
    for key in TABLES:
        assert np.array_equal(res[key], host[key]) and np.array_equal(res[key], again[key]), key
    assert again["status"] == 0


def test_boundary_matching_ragged_groups():
    groups = [BO.with_boundary(g, 800 + i) for i, g in enumerate(ragged_groups())]
    dev_fn, host_fn = match_entries()
    res = BO.run_match(dev_fn, groups, dev=DEV, guard=16, area_rngs=SMALL_RNGS, max_det=20)
    assert res["status"] == 0
    BO.check_groups(res, groups, area_rngs=SMALL_RNGS, max_det=20)
    host = BO.run_match(host_fn, groups, area_rngs=SMALL_RNGS, max_det=20)
    for key in TABLES:
        assert np.array_equal(res[key], host[key]), key


@pytest.mark.parametrize("name", [c[0] for c in refusal_cases()])
def test_boundary_matching_refuses_whole_groups(name):
    _, groups, tabs, refused = next(c for c in refusal_cases() if c[0] == name)
    groups = [BO.with_boundary(g, 900 + i) for i, g in enumerate(groups)]
    dev_fn, host_fn = match_entries()
    res = BO.run_match(dev_fn, groups, tabs=tabs, dev=DEV, guard=16, area_rngs=SMALL_RNGS)
    assert res["status"] == 1
    BO.check_groups(res, groups, area_rngs=SMALL_RNGS, refused=refused)
    host = BO.run_match(host_fn, groups, tabs=tabs, area_rngs=SMALL_RNGS)
    for key in TABLES:
        assert np.array_equal(res[key], host[key]), key
    whole = BO.run_match(dev_fn, groups, dev=DEV, outs=res["outs"], area_rngs=SMALL_RNGS)      # the status is zeroed again
    assert whole["status"] == (1 if "1024" in name else 0)


def test_a_match_the_boundary_takes_away():
    """A square of 60 x 60 against itself shifted by three pixels: mask IoU 3249 / 3951 = 0.82, boundary IoU at d = 2 far below 0.5 --
    matched by cvlm_coco_match at 0.5, unmatched by cvlm_coco_match_boundary."""
    from camouflaged_vlm_amd import hip
    a, b = np.zeros((100, 100), dtype=bool), np.zeros((100, 100), dtype=bool)
    a[10:70, 10:70] = True
    b[13:73, 13:73] = True
    ba, bb = BO.boundary(a, 2), BO.boundary(b, 2)
    g = dict(inter=np.array([[(a & b).sum()]]), det_area=np.array([a.sum()]), gt_area=np.array([b.sum()]),
             scores=np.array([0.5], dtype=np.float32), range_area=None, iscrowd=np.zeros(1, dtype=np.uint8),
             inter_b=np.array([[(ba & bb).sum()]]), det_area_b=np.array([ba.sum()]), gt_area_b=np.array([bb.sum()]))
    assert MO.ious_of(g["inter"], g["det_area"], g["gt_area"], g["iscrowd"])[0, 0] > 0.8 and 0.0 < BO.ious_min(g)[0, 0] < 0.5
    plain = MO.run_entry(hip.coco_match, MO.tables([g]), dev=DEV)
    res = BO.run_match(hip.coco_match_boundary, [g], dev=DEV)
    assert plain["dt_match"][0, 0, 0] == 0 and res["dt_match"][0, 0, 0] == -1
    assert plain["gt_match"][0, 0, 0] == 0 and res["gt_match"][0, 0, 0] == -1
    BO.check_groups(res, [g])


# ---- tiny geometry, exact -------------------------------------------------------------------------------------------------------------------------
def boundary_groups(req, det_planes, gt_planes, scores, ratio=0.02):
    """test_match_gpu's oracle_groups with the boundaries' integers beside the masks': numpy boundaries at each plane's own radius,
    intersections by & and sum."""
    bd = lambda m: BO.boundary(m, BO.boundary_radius(*m.shape, ratio))
    det_b, gt_b = [bd(m) for m in det_planes], [bd(m) for m in gt_planes]
    groups = oracle_groups(req, det_planes, gt_planes, scores)
    for e, grp in enumerate(groups):
        ds = req.det_perm[req.det_offsets[e]:req.det_offsets[e + 1]]
        gs = req.gt_perm[req.gt_offsets[e]:req.gt_offsets[e + 1]]
        grp.update(inter_b=np.array([[int((det_b[d] & gt_b[g]).sum()) for g in gs] for d in ds], dtype=np.int64).reshape(len(ds), len(gs)),
                   det_area_b=np.array([int(det_b[d].sum()) for d in ds], dtype=np.int64),
                   gt_area_b=np.array([int(gt_b[g].sum()) for g in gs], dtype=np.int64))
    return groups


def stats_of(req, groups, evaluate):
    cats = sorted({k[0] for k in req.keys}) if req.keys[0][0] is not None else [None]
    evals = [[[] for _ in MO.AREA_RNGS] for _ in cats]
    for key, grp in zip(req.keys, groups):
        for a, r in enumerate(evaluate(grp, max_det=req.max_det)):
            evals[cats.index(key[0])][a].append(r)
    return MO.summarize(MO.accumulate(evals, len(cats), 4))


def test_mask_boundary_sized_through_cascade_and_dropin(cas, dropin, monkeypatch):
    """Random planes of four sizes through rle_decode: the published radius, radius=, a ratio; no synchronisation; the result feeds
    mask_inter_sized, mask_rle_sized and concat; Boundary IoU of pairs is the oracle's."""
    from camouflaged_vlm_amd.engine import SizedMasks
    rng = np.random.default_rng(25)
    sizes = [(97, 131), (97, 131), (33, 31), (40, 70), (130, 257)]
    base = rng.random(sizes[0]) < 0.5
    planes = [base, base ^ (rng.random(sizes[0]) < 0.03)] + [rng.random(s) < 0.97 for s in sizes[2:]]
    for m in planes[2:]:
        m[:3] = False
    coco = [{"size": list(m.shape), "counts": RO.plane_counts(m).tolist()} for m in planes]
    a = cas.rle_decode(coco)
    torch.cuda.synchronize()
    reads = record_reads(monkeypatch)
    b = cas.mask_boundary_sized(a)
    monkeypatch.undo()
    assert reads == [], reads
    assert isinstance(b, SizedMasks) and b.sizes == a.sizes and b.level == a.level and torch.equal(b.offsets, a.offsets)
    b.check()
    radii = [BO.boundary_radius(h, w) for h, w in sizes]
    assert radii == [3, 3, 1, 2, 6]
    for p, m in enumerate(planes):
        want = BO.boundary(m, radii[p])
        assert np.array_equal(b.to_numpy(p), want), p
        assert b.area[p].item() == want.sum()
    assert torch.equal(b.box, a.box) and b.box.data_ptr() != a.box.data_ptr()
    fixed = cas.mask_boundary_sized(a, radius=[1, 2, 3, 4, 40])
    for p, d in enumerate([1, 2, 3, 4, 40]):
        assert np.array_equal(fixed.to_numpy(p), BO.boundary(planes[p], d)), p
    wide = dropin.mask_boundary_sized(a, dilation_ratio=0.05)
    for p, (h, w) in enumerate(sizes):
        assert np.array_equal(wide.to_numpy(p), BO.boundary(planes[p], BO.boundary_radius(h, w, 0.05))), p
    bare = cas.mask_boundary_sized(cas.rle_decode(coco, stats=False))
    assert bare.area is None and bare.box is None and torch.equal(bare.bits, b.bits)
    # what the result feeds
    iou = cas.mask_inter_sized(b, b, pairs=[(0, 1), (1, 0), (0, 0)]).iou()
    assert iou.tolist() == [BO.boundary_iou(planes[0], planes[1], 3), BO.boundary_iou(planes[1], planes[0], 3), 1.0]
    assert 0.0 < iou[0] < 1.0
    back = cas.rle_decode(cas.mask_rle_sized(b).to_coco())
    assert all(np.array_equal(back.to_numpy(p), b.to_numpy(p)) for p in range(5)) and torch.equal(back.area, b.area)
    both = SizedMasks.concat([a, b])
    assert both.sizes == a.sizes + b.sizes and torch.equal(both.area, torch.cat([a.area, b.area]))
    # bad requests raise before anything is launched
    from camouflaged_vlm_amd import hip
    seen = []
    monkeypatch.setattr(hip, "mask_boundary_sized", lambda *x, **k: seen.append("mask_boundary_sized"))
    for bad in (dict(dilation_ratio=0.0), dict(radius=[1] * 4), dict(radius=[1] * 5, dilation_ratio=0.1), dict(radius=[1, 1, 1, 1, True]),
                dict(radius=0), dict(sized=a.bits)):
        kw = dict(dict(sized=a), **bad)
        with pytest.raises(ValueError, match="mask_boundary_sized"):
            cas.mask_boundary_sized(kw.pop("sized"), **kw)
    assert seen == []


def test_boundary_ap_end_to_end_on_the_tiny_cascade(tiny, cas, dropin, tracer, monkeypatch):
    """Annotations made from the call's own rle="sized" output give Boundary AP = 1.  With one annotation eroded by one pixel, Boundary
    AP is the oracle's -- numpy boundaries, numpy intersections, the published loops over the minimum -- to the last bit, and is not
    the mask AP of the same data (on hypotheses with a solid block each: see below why)."""
    from camouflaged_vlm_amd import cocoeval
    _, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    h = cas.infer_classes(inp, ci, cm, classes=torch.tensor(CLASSES), masks="bits", sizes=SIZES, rle="sized")
    planes = [h.sized.to_numpy(p) for p in range(6)]
    image, cat = [0, 0, 0, 1, 1, 1], [c for row in CLASSES for c in row]
    full = [p for p in range(6) if planes[p].any()]
    assert len(full) >= 3
    dicts = h.rle.to_coco()
    gts = cas.rle_decode([dicts[p] for p in full])
    scores = h.sized.area.to(torch.float32)
    kw = dict(scores=scores, det_image=image, gt_image=[image[p] for p in full], det_category=cat, gt_category=[cat[p] for p in full])
    torch.cuda.synchronize()
    with tracer.Recorder() as log:
        plain = cas.coco_match(h.sized, gts, **kw)
        n_plain = len(log)
        m = cas.coco_match(h.sized, gts, boundary=0.02, **kw)
        torch.cuda.synchronize()
    names = [e if isinstance(e, str) else e[0] for e in log]
    assert names[:n_plain] == ["mask_inter_sized", "coco_match"]                              # what it launched before §25
    assert names[n_plain:] == ["mask_inter_sized", "mask_boundary_sized", "mask_boundary_sized", "mask_inter_sized", "coco_match_boundary"]
    assert plain.boundary_overlaps is None and m.boundary_overlaps is not None
    m.check()
    stats = cocoeval.summarize(cocoeval.accumulate(m))
    assert stats[0] == stats[1] == stats[2] == 1.0 and stats[8] == 1.0
    for key in TABLES:
        assert torch.equal(getattr(m, key), getattr(plain, key)), key                           # identical planes: both IoUs are 1
    # The synthetic weights give speckle: no pixel of a hypothesis has a whole (2 d + 1)^2 window at d = 8 or 16, so the boundary of
    # every plane above is the plane itself and the two metrics cannot differ on them, whatever is eroded.  The second half therefore
    # gives each hypothesis a solid block of its own, through rle_decode; one annotation is its detection eroded by one pixel -- the
    # first for which the ORACLE's two metrics differ.
    from camouflaged_vlm_amd.engine import match_request
    assert all(not BO.erode(m, BO.boundary_radius(*m.shape)).any() for m in planes)
    solid = []
    for p, m in enumerate(planes):
        hh, ww = m.shape
        d = m.copy()
        d[hh // 8 + 3 * p:7 * hh // 8 - 3 * p, ww // 8 + 2 * p:7 * ww // 8 - 2 * p] = True
        solid.append(d)
    coco = lambda ms: [{"size": list(g.shape), "counts": RO.plane_counts(g).tolist()} for g in ms]
    dets = cas.rle_decode(coco(solid))
    s = np.linspace(0.9, 0.4, 6).astype(np.float32)
    kw = dict(scores=torch.from_numpy(s).to(DEV), det_image=image, gt_image=image, det_category=cat, gt_category=cat)
    req = match_request(dets.sizes, dets.sizes, det_image=image, gt_image=image, det_category=cat, gt_category=cat, scores=s)
    chosen = None
    for p in range(6):
        gt_planes = [BO.erode(solid[q], 1) if q == p else solid[q] for q in range(6)]
        groups = boundary_groups(req, solid, gt_planes, s)
        want_b, want_m = stats_of(req, groups, BO.evaluate_group), stats_of(req, groups, MO.evaluate_group)
        if want_b != want_m:
            chosen = (gt_planes, groups, want_b, want_m)
            break
    assert chosen is not None, "no one-pixel erosion tells the two metrics apart on these planes"
    gt_planes, groups, want_b, want_m = chosen
    gts = cas.rle_decode(coco(gt_planes))
    mb = cas.coco_match(dets, gts, boundary=0.02, **kw)
    mb.check()
    assert mb.request.keys == req.keys and np.array_equal(mb.request.det_perm, req.det_perm)
    host = mb.to_host()
    BO.check_groups(host, groups)
    got_b = cocoeval.summarize(cocoeval.accumulate(mb))
    got_m = cocoeval.summarize(cocoeval.accumulate(cas.coco_match(dets, gts, **kw)))
    assert got_b == want_b and got_m == want_m, (got_b, want_b, got_m, want_m)                  # to the last bit
    assert got_b != got_m
    other = dropin.coco_match(dets, gts, boundary=0.02, **kw)
    for key in TABLES:
        assert torch.equal(getattr(other, key), getattr(mb, key)), key
    # bad requests raise before anything is launched
    with tracer.Recorder() as log:
        for bad in (0.0, -1.0, float("nan"), True, "0.02", 30.0):
            with pytest.raises(ValueError, match="coco_match"):
                cas.coco_match(dets, gts, boundary=bad, **kw)
    assert log == []
