"""COCO matching without a GPU: the oracle (tests/match_oracle.py: the published loops) against known answers and
against its own sort-free restatement; cvlm_debug_coco_match_host -- the kernel's per-thread functions run sequentially -- against the
oracle on every group shape of the GPU list; every ValueError of match_request with the launchers replaced by a recorder; every
CVLM_E_BADARG; the exports; cocoeval.accumulate / summarize against the oracle.  Everything up to accumulate is integers or bytes and
compared exactly; accumulate is float64 and compared exactly too, since it is the same operations in the same order."""
import ctypes

import numpy as np
import pytest
import torch

import match_oracle as MO

SHAPES = [(0, 3, 100), (3, 0, 100), (0, 0, 100), (1, 1, 100), (5, 4, 100), (7, 3, 3), (33, 31, 100), (64, 65, 100), (130, 70, 100)]
SMALL_RNGS = [[0, 1e10], [0, 15], [15, 25], [25, 1e10]]            # for pixel areas 1 .. 40: every annotation is ignored somewhere
RNGS8 = SMALL_RNGS + [[10, 30], [0, 0], [40, 40], [5, 1e10]]
THRS16 = [0.05, 0.1, 0.25, 1 / 3, 0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95, 0.99, 1.0]


def make_group(D, G, seed, scores="levels", refused_pair=False, range_area=False):
    """A random group with small integer areas, so that IoU ties and exact threshold hits abound."""
    rng = np.random.default_rng(seed)
    da, ga = rng.integers(1, 41, D), rng.integers(1, 41, G)
    inter = np.array([[rng.integers(0, min(da[d], ga[g]) + 1) for g in range(G)] for d in range(D)], dtype=np.int64).reshape(D, G)
    if refused_pair and D and G:
        inter[rng.integers(0, D), rng.integers(0, G)] = -1
    if scores == "equal":
        s = np.full(D, 0.5, dtype=np.float32)
    elif scores == "special":
        s = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 0.25, 1.0], dtype=np.float32), D)
    else:
        s = (rng.integers(0, 4, D) / 4).astype(np.float32)
    ra = None
    if range_area:                                                   # the file's own "area": doubles, some exactly on a range's end
        ra = rng.choice(np.array([0.0, 14.5, 15.0, 15.5, 25.0, 25.000001, 1024.0, 1024.5, 9216.0, 1e10, 2e10]), G)
    return dict(inter=inter, det_area=da, scores=s, gt_area=ga, range_area=ra, iscrowd=(rng.random(G) < 0.25).astype(np.uint8))


def threshold_group(below: int):
    """Ten detections of 20 pixels, annotation k of k pixels (10 .. 19) inside detection k - 10: IoU = k / 20, exactly on the ten default
    thresholds; below = 1 takes one pixel of each intersection away: (k - 1) / 21."""
    ga = np.arange(10, 20)
    inter = np.diag(ga - below)
    return dict(inter=inter, det_area=np.full(10, 20), scores=np.linspace(1, 0.1, 10).astype(np.float32), gt_area=ga, range_area=None,
                iscrowd=np.zeros(10, dtype=np.uint8))


def crowd_group():
    """One crowd annotation of 40 pixels and one plain one; four detections inside the crowd, the best of them also on the plain one."""
    return dict(inter=np.array([[10, 8], [12, 0], [9, 0], [0, 0]]), det_area=np.array([10, 12, 12, 30]),
                scores=np.array([0.9, 0.8, 0.7, 0.6], dtype=np.float32), gt_area=np.array([40, 8]), range_area=None,
                iscrowd=np.array([1, 0], dtype=np.uint8))


def shape_cases():
    """(name, groups, keyword arguments of the match) for every (D, G) of the list, with every kind of value."""
    cases = []
    for i, (D, G, md) in enumerate(SHAPES):
        for kind in ("levels", "equal", "special"):
            cases.append((f"{D}x{G}-{kind}", [make_group(D, G, 100 + i, kind, refused_pair=kind == "special", range_area=kind == "equal")],
                          dict(area_rngs=SMALL_RNGS, max_det=md)))
    cases.append(("thresholds", [threshold_group(0), threshold_group(1)], dict(area_rngs=SMALL_RNGS)))
    cases.append(("crowd", [crowd_group()], dict(area_rngs=SMALL_RNGS)))
    cases.append(("T1-A1", [make_group(33, 31, 7)], dict(iou_thrs=[0.5], area_rngs=[[0, 1e10]])))
    cases.append(("T16-A8", [make_group(64, 65, 8), make_group(5, 4, 9, range_area=True)], dict(iou_thrs=THRS16, area_rngs=RNGS8)))
    cases.append(("default-ranges", [make_group(12, 9, 10, range_area=True)], {}))
    return cases


def ragged_groups():
    """37 groups of every small shape in one call."""
    rng = np.random.default_rng(37)
    kinds = ("levels", "equal", "special")
    return [make_group(int(rng.integers(0, 40)) if e % 5 else 0, int(rng.integers(0, 40)) if e % 7 else 0, 500 + e, kinds[e % 3],
                       refused_pair=e % 4 == 0, range_area=e % 2 == 0) for e in range(37)]


def refusal_cases():
    """(name, doctored tables of three groups, the refused groups): every way a group is refused, the neighbours whole."""
    groups = [make_group(5, 4, 1), make_group(6, 3, 2), make_group(4, 4, 3)]
    base = MO.tables(groups)
    cases = []

    def doctored(name, refused, **change):
        tabs = {k: v.copy() for k, v in base.items()}
        for key, (idx, val) in change.items():
            tabs[key][idx] = val
        cases.append((name, groups, tabs, refused))

    doctored("det offsets run backwards", (0, 1), det_offsets=(1, 12))         # group 0 has 12 rows for a block of 5 x 4; group 1 is [12, 11)
    doctored("gt offsets leave the table", (2,), gt_offsets=(3, 12))
    doctored("negative det offset", (0,), det_offsets=(0, -1))
    doctored("pair block too short", (1, 2), pair_offsets=(2, 37))
    doctored("pair block leaves the table", (2,), pair_offsets=(3, 55))
    doctored("negative pair offset", (0,), pair_offsets=(0, -1))
    big = [make_group(1025, 1, 4), make_group(2, 2, 5)]
    cases.append(("more than 1024 detections", big, MO.tables(big), (0,)))
    big = [make_group(2, 2, 5), make_group(1, 1025, 6)]
    cases.append(("more than 1024 annotations", big, MO.tables(big), (1,)))
    return cases


def host_entry():
    from camouflaged_vlm_amd import hip
    return hip.coco_match_host


# ---- the oracle against known answers ----------------------------------------------------------------------------------------------------
def test_oracle_detections_equal_to_annotations_give_ap_one():
    evals = [[[] for _ in MO.AREA_RNGS] for _ in range(2)]
    for k in range(2):
        for img in range(3):
            area = np.array([500, 2000, 20000, 900])                  # small, medium, large, small
            grp = dict(inter=np.diag(area), det_area=area, scores=np.array([0.9, 0.8, 0.7, 0.6], dtype=np.float32), gt_area=area,
                       range_area=None, iscrowd=np.zeros(4, dtype=np.uint8))
            for a, r in enumerate(MO.evaluate_group(grp)):
                assert (r["dtm"] == r["order"][None, :]).all()
                evals[k][a].append(r)
    acc = MO.accumulate(evals, 2, 4, max_dets=(1, 10, 100))
    assert (acc["precision"][..., 2] == 1.0).all()
    stats = MO.summarize(acc)
    assert stats[:6] == [1.0] * 6 and stats[8:] == [1.0] * 4
    assert stats[6] == 0.25                                           # AR@1: one of four annotations per image


def test_oracle_no_detection_gives_recall_zero():
    grp = dict(inter=np.zeros((0, 2)), det_area=np.zeros(0), scores=np.zeros(0, dtype=np.float32), gt_area=np.array([500, 600]),
               range_area=None, iscrowd=np.zeros(2, dtype=np.uint8))
    evals = [[[r] for r in MO.evaluate_group(grp)]]
    acc = MO.accumulate(evals, 1, 4)
    assert (acc["recall"][:, 0, 0, :] == 0).all() and (acc["recall"][:, 0, 1, :] == 0).all()
    assert (acc["recall"][:, 0, 2, :] == -1).all()                    # no medium annotation: the cell is skipped
    assert (acc["precision"][:, :, 0, 0, :] == 0).all()
    stats = MO.summarize(acc)
    assert stats[0] == 0.0 and stats[8] == 0.0 and stats[4] == -1.0


def test_oracle_hand_worked_group():
    """Three detections, two annotations, one crowd (crowd_group without its last detection), area range all, t = 0.5 and 0.95.
    IoUs: d0 (10 px): crowd 10/10 = 1, plain 8/(10 + 8 - 8) = 0.8;  d1 (12 px): crowd 12/12 = 1, plain 0;  d2 (12 px): crowd 9/12 = 0.75.
    t = 0.5: d0 takes the plain annotation (not ignored beats ignored); d1 and d2 both take the crowd and are ignored.
    t = 0.95: d0 cannot take the plain one (0.8), so it takes the crowd and is ignored; d1 too; d2 (0.75) stays unmatched, not ignored."""
    g = crowd_group()
    g = dict(g, inter=g["inter"][:3], det_area=g["det_area"][:3], scores=g["scores"][:3])
    assert np.array_equal(MO.ious_of(g["inter"], g["det_area"], g["gt_area"], g["iscrowd"]), np.array([[1, 0.8], [1, 0], [0.75, 0]]))
    r = MO.evaluate_group(g, iou_thrs=[0.5, 0.95], area_rngs=[[0, 1e10]])[0]
    assert r["order"].tolist() == [0, 1, 2] and r["gt_ig"].tolist() == [True, False]
    assert r["dtm"].tolist() == [[1, 0, 0], [0, 0, -1]]
    assert r["dt_ig"].tolist() == [[False, True, True], [True, True, False]]
    assert r["gtm"].tolist() == [[2, 0], [1, -1]]                     # the crowd keeps the LAST detection that took it


def test_oracle_thresholds_are_hit_exactly():
    for k in range(10, 20):
        assert k / 20 >= MO.IOU_THRS[k - 10] > (k - 1) / 21
    assert MO.IOU_THRS[8] == 0.8999999999999999
    on, below = (MO.evaluate_group(threshold_group(b), area_rngs=[[0, 1e10]])[0] for b in (0, 1))
    for d in range(10):                                               # detection d has IoU (10 + d) / 20: matched at thresholds 0 .. d
        assert (on["dtm"][:d + 1, d] == d).all() and (on["dtm"][d + 1:, d] == -1).all()
        assert below["dtm"][d, d] == -1                               # one pixel short of threshold d
        for j in range(10):
            assert (below["dtm"][j, d] == d) == (21 * (10 + j) <= 20 * (9 + d))       # (9 + d) / 21 >= (10 + j) / 20 in integers


def test_argmax_form_equals_the_published_loop():
    n = 0
    for it in range(600):
        rng = np.random.default_rng(it)
        g = make_group(int(rng.integers(0, 9)), int(rng.integers(0, 7)), 9000 + it, ("levels", "equal", "special")[it % 3],
                       refused_pair=it % 5 == 0, range_area=it % 4 == 0)
        md = [1, 3, 100][it % 3]
        for x, y in zip(MO.evaluate_group(g, area_rngs=SMALL_RNGS, max_det=md), MO.evaluate_group(g, area_rngs=SMALL_RNGS, max_det=md, form=MO.argmax_form)):
            for key in ("order", "dtm", "dt_ig", "gtm", "gt_ig"):
                assert np.array_equal(x[key], y[key]), (it, key)
            n += 1
    assert n == 2400


# ---- the host entry against the oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in shape_cases()])
def test_host_entry_equals_the_oracle(name):
    _, groups, kw = next(c for c in shape_cases() if c[0] == name)
    res = MO.run_entry(host_entry(), MO.tables(groups), guard=16, **kw)
    assert res["status"] == 0
    MO.check_groups(res, groups, **kw)
    again = MO.run_entry(host_entry(), MO.tables(groups), outs=res["outs"], **kw)        # into used outputs
    for key in ("dt_order", "dt_match", "dt_ignore", "gt_match", "gt_ignore"):
        assert np.array_equal(res[key], again[key])


def test_host_entry_ragged_groups():
    groups = ragged_groups()
    res = MO.run_entry(host_entry(), MO.tables(groups), area_rngs=SMALL_RNGS, max_det=20, guard=16)
    assert res["status"] == 0
    MO.check_groups(res, groups, area_rngs=SMALL_RNGS, max_det=20)


@pytest.mark.parametrize("name", [c[0] for c in refusal_cases()])
def test_host_entry_refuses_whole_groups(name):
    _, groups, tabs, refused = next(c for c in refusal_cases() if c[0] == name)
    res = MO.run_entry(host_entry(), tabs, area_rngs=SMALL_RNGS, guard=16)
    assert res["status"] == 1
    MO.check_groups(res, groups, area_rngs=SMALL_RNGS, refused=refused)


# ---- CVLM_E_BADARG and the exports --------------------------------------------------------------------------------------------------------
def test_every_badarg():
    from camouflaged_vlm_amd import hip
    lib = hip.load()
    g = [make_group(3, 2, 1)]
    tabs = MO.tables(g)
    T, A, ND, NG, N = 10, 4, 3, 2, 6
    keep = {k: torch.from_numpy(v.copy()) for k, v in tabs.items()}
    keep.update(iou_thrs=torch.from_numpy(MO.IOU_THRS.copy()), area_rngs=torch.tensor(MO.AREA_RNGS, dtype=torch.float64),
                dt_order=torch.zeros(ND + 1, dtype=torch.int32), dt_match=torch.zeros(A * T * ND + 1, dtype=torch.int32),
                dt_ignore=torch.zeros(A * T * ND, dtype=torch.uint8), gt_match=torch.zeros(A * T * NG + 1, dtype=torch.int32),
                gt_ignore=torch.zeros(A * NG, dtype=torch.uint8), status=torch.zeros(2, dtype=torch.int32))
    order = ["det_offsets", "gt_offsets", "pair_offsets", "E", "inter", "N", "det_area", "score", "ND", "gt_area", "gt_range_area", "gt_crowd",
             "NG", "iou_thrs", "T", "area_rngs", "A", "max_det", "dt_order", "dt_match", "dt_ignore", "gt_match", "gt_ignore", "status"]
    good = {k: v.data_ptr() for k, v in keep.items()}
    good.update(E=1, N=N, ND=ND, NG=NG, T=T, A=A, max_det=100)

    def call(dev: bool, **change):
        args = [dict(good, **change)[k] for k in order]
        return lib.cvlm_coco_match(*args, None) if dev else lib.cvlm_debug_coco_match_host(*args)

    assert call(False) == 0
    bad = [{k: None} for k in order if k not in ("E", "N", "ND", "NG", "T", "A", "max_det")]
    bad += [{k: good[k] + 2} for k in ("det_offsets", "gt_offsets", "inter", "det_area", "score", "gt_area", "dt_order", "dt_match", "gt_match", "status")]
    bad += [{k: good[k] + 4} for k in ("pair_offsets", "gt_range_area", "iou_thrs", "area_rngs")]
    bad += [dict(E=0), dict(E=(1 << 20) + 1), dict(N=-1), dict(N=(1 << 20) + 1), dict(ND=-1), dict(ND=(1 << 20) + 1), dict(NG=-1),
            dict(NG=(1 << 20) + 1), dict(T=0), dict(T=17), dict(A=0), dict(A=9), dict(max_det=0)]
    for change in bad:
        for dev in (False, True):                                     # refused before the device is touched: no GPU is needed
            assert call(dev, **change) == -1, change
    # a table of no rows may be NULL
    zeros32, zeros64 = torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
    assert call(False, N=0, inter=None, ND=0, det_area=None, score=None, dt_order=None, dt_match=None, dt_ignore=None,
                det_offsets=zeros32.data_ptr(), pair_offsets=zeros64.data_ptr()) == 0


def test_exports_at_abi_12():
    from camouflaged_vlm_amd import hip
    lib = hip.load()
    assert lib.cvlm_abi_version() == hip.ABI_VERSION == 12
    for name in ("cvlm_coco_match", "cvlm_debug_coco_match_host"):
        assert name in hip.EXPORTS and hasattr(lib, name)
        assert hip.ABI[name][0] is ctypes.c_int32
    assert "cvlm_coco_match" in hip._STREAMED and "cvlm_debug_coco_match_host" not in hip._STREAMED


# ---- match_request ----------------------------------------------------------------------------------------------------------------------------
GOOD = dict(det_sizes=[(4, 5)] * 3, gt_sizes=[(4, 5)] * 2, det_image=[1, 0, 1], gt_image=[1, 1], det_category=[7, 7, 3], gt_category=[7, 3],
            iscrowd=[0, 1], gt_area=[12.5, 3], scores=[0.1, 0.2, 0.3])

BAD_REQUESTS = {
    "det_image too short": dict(det_image=[1, 0]),
    "det_image not ints": dict(det_image=[1, 0.5, 1]),
    "det_image a bool": dict(det_image=[1, True, 1]),
    "gt_image a string": dict(gt_image="ab"),
    "one category only": dict(gt_category=None),
    "the other category only": dict(det_category=None),
    "category not ints": dict(det_category=[7, "x", 3]),
    "gt_category too long": dict(gt_category=[7, 3, 3]),
    "iscrowd too short": dict(iscrowd=[0]),
    "iscrowd not numbers": dict(iscrowd=["a", "b"]),
    "gt_area negative": dict(gt_area=[12.5, -1]),
    "gt_area infinite": dict(gt_area=[np.inf, 3]),
    "gt_area NaN": dict(gt_area=[np.nan, 3]),
    "gt_area too short": dict(gt_area=[3]),
    "scores NaN": dict(scores=[0.1, np.nan, 0.3]),
    "scores too short": dict(scores=[0.1, 0.2]),
    "scores not numbers": dict(scores=["a", "b", "c"]),
    "iou_thrs empty": dict(iou_thrs=[]),
    "iou_thrs zero": dict(iou_thrs=[0.0, 0.5]),
    "iou_thrs above one": dict(iou_thrs=[0.5, 1.5]),
    "iou_thrs seventeen": dict(iou_thrs=[0.5] * 17),
    "iou_thrs not flat": dict(iou_thrs=[[0.5]]),
    "area_rngs backwards": dict(area_rngs=[[0, 1e10], [5, 1]]),
    "area_rngs nine": dict(area_rngs=[[0, 1]] * 9),
    "area_rngs not pairs": dict(area_rngs=[0, 1e10]),
    "area_rngs empty": dict(area_rngs=[]),
    "max_det zero": dict(max_det=0),
    "max_det a float": dict(max_det=100.0),
    "max_det a bool": dict(max_det=True),
    "two sizes in a group": dict(gt_sizes=[(4, 5), (5, 4)], gt_category=[7, 7]),
    "a detection of another size": dict(det_sizes=[(4, 5), (4, 5), (4, 6)], det_category=[7, 7, 7]),
    "more than 1024 detections": dict(det_sizes=[(4, 5)] * 1025, det_image=[1] * 1025, det_category=[7] * 1025, scores=[0.5] * 1025),
    "more than 1024 annotations": dict(gt_sizes=[(4, 5)] * 1025, gt_image=[1] * 1025, gt_category=[7] * 1025, iscrowd=None, gt_area=None),
    # 1024 x 1024 + 1 x 1 = 2^20 + 1 pairs, no group over the cap
    "more than 2^20 pairs": dict(det_sizes=[(4, 5)] * 2049, det_image=[0] * 1024 + [1] * 1024 + [2], det_category=None, scores=[0.5] * 2049,
                                 gt_sizes=[(4, 5)] * 2049, gt_image=[0] * 1024 + [1] * 1024 + [2], gt_category=None, iscrowd=None, gt_area=None),
    "nothing at all": dict(det_sizes=[], gt_sizes=[], det_image=[], gt_image=[], det_category=None, gt_category=None, iscrowd=None, gt_area=None,
                           scores=None),
}


MESSAGES = {"more than 2^20 pairs": "pairs, at most", "more than 1024 detections": "at most 1024", "more than 1024 annotations": "at most 1024",
            "two sizes in a group": "one image has one size", "a detection of another size": "one image has one size",
            "nothing at all": "no detection and no annotation", "scores NaN": "NaN", "gt_area NaN": "finite", "one category only": "both"}


@pytest.fixture
def launches(monkeypatch):
    """Every launcher coco_match could reach, replaced by a recorder."""
    from camouflaged_vlm_amd import hip
    seen = []
    for name in ("coco_match", "coco_match_host", "mask_inter_sized"):
        monkeypatch.setattr(hip, name, lambda *a, _n=name, **k: seen.append(_n))
    return seen


def request(**change):
    from camouflaged_vlm_amd.maskpost import match_request
    kw = dict(GOOD, **change)
    return match_request(kw.pop("det_sizes"), kw.pop("gt_sizes"), **kw)


@pytest.mark.parametrize("name", list(BAD_REQUESTS))
def test_bad_requests_raise_and_launch_nothing(name, launches):
    with pytest.raises(ValueError, match=MESSAGES.get(name, "coco_match")):
        request(**BAD_REQUESTS[name])
    assert launches == []


def test_request_tables(launches):
    from camouflaged_vlm_amd import engine, maskpost
    assert engine.match_request is maskpost.match_request and engine.Cascade.coco_match is maskpost.MaskUtilities.coco_match
    r = request()
    assert r.keys == [(3, 1), (7, 0), (7, 1)]                         # sorted by (category, image)
    assert r.det_perm.tolist() == [2, 1, 0] and r.gt_perm.tolist() == [1, 0]
    assert r.det_offsets.tolist() == [0, 1, 2, 3] and r.gt_offsets.tolist() == [0, 1, 1, 2] and r.pair_offsets.tolist() == [0, 1, 1, 2]
    assert r.pairs.tolist() == [[2, 1], [0, 0]] and r.pairs.dtype == np.int32
    assert r.crowd.tolist() == [1, 0] and r.range_area.tolist() == [3.0, 12.5] and r.scores.tolist() == [np.float32(0.3), np.float32(0.2), np.float32(0.1)]
    assert r.iou_thrs.tolist() == MO.IOU_THRS.tolist() and r.iou_thrs[8] == 0.8999999999999999
    assert r.area_rngs.tolist() == MO.AREA_RNGS and r.max_det == 100
    r = request(det_category=None, gt_category=None, scores=None, gt_area=None, iscrowd=None)
    assert r.keys == [(None, 0), (None, 1)] and r.det_perm.tolist() == [1, 0, 2] and r.pairs.tolist() == [[0, 0], [0, 1], [2, 0], [2, 1]]
    assert r.scores is None and r.range_area is None and r.crowd.tolist() == [0, 0]
    assert launches == []


# ---- accumulate / summarize against the oracle ----------------------------------------------------------------------------------------------
def host_matches(groups, keys, area_rngs=MO.AREA_RNGS, max_det=100):
    """What CocoMatches.to_host() gives for the groups (in the order of keys, which must be sorted), through the host entry."""
    assert keys == sorted(keys, key=lambda k: (k[0] is not None, k))
    tabs = MO.tables(groups)
    res = MO.run_entry(host_entry(), tabs, area_rngs=area_rngs, max_det=max_det)
    return dict(dt_order=res["dt_order"], dt_match=res["dt_match"], dt_ignore=res["dt_ignore"], gt_match=res["gt_match"],
                gt_ignore=res["gt_ignore"], score=tabs["score"], status=res["status"], keys=keys, det_offsets=tabs["det_offsets"],
                gt_offsets=tabs["gt_offsets"], det_perm=np.arange(len(tabs["score"])), gt_perm=np.arange(len(tabs["gt_area"])),
                iou_thrs=MO.IOU_THRS.copy(), area_rngs=np.asarray(area_rngs, dtype=np.float64), max_det=max_det)


def big_group(D, G, seed, equal_scores=False):
    """Areas across small / medium / large, so that every default range counts somewhere; many detections share a score."""
    rng = np.random.default_rng(seed)
    ga = rng.choice(np.array([200, 1000, 1024, 3000, 9216, 20000]), G)
    da = rng.choice(np.array([200, 1000, 1024, 3000, 9216, 20000]), D)
    inter = np.array([[rng.integers(0, min(da[d], ga[g]) + 1) if rng.random() < 0.5 else min(da[d], ga[g]) for g in range(G)]
                      for d in range(D)], dtype=np.int64).reshape(D, G)
    s = np.full(D, 0.5, dtype=np.float32) if equal_scores else (rng.integers(0, 5, D) / 4).astype(np.float32)
    return dict(inter=inter, det_area=da, scores=s, gt_area=ga, range_area=None, iscrowd=(rng.random(G) < 0.2).astype(np.uint8))


def oracle_accumulate(parts, cats, max_dets, max_det=100):
    """parts: lists of (key, group) in the order accumulate concatenates them."""
    evals = [[[] for _ in MO.AREA_RNGS] for _ in cats]
    for part in parts:
        for key, grp in part:
            for a, r in enumerate(MO.evaluate_group(grp, max_det=max_det)):
                evals[cats.index(key[0])][a].append(r)
    return MO.accumulate(evals, len(cats), 4, max_dets=max_dets)


def assert_same(acc, want):
    for key in ("precision", "recall", "scores"):
        assert acc[key].shape == want[key].shape and np.array_equal(acc[key], want[key]), key
    from camouflaged_vlm_amd import cocoeval
    assert cocoeval.summarize(acc) == MO.summarize(want)


def test_accumulate_equals_the_oracle():
    from camouflaged_vlm_amd import cocoeval
    # category 9 has annotations that are all crowd: npig == 0, its cells stay -1; equal scores across the groups of category 5
    no_count = dict(big_group(3, 2, 40), iscrowd=np.ones(2, dtype=np.uint8))
    one = [((2, 0), big_group(12, 7, 1)), ((2, 1), big_group(5, 9, 2)), ((5, 0), big_group(6, 4, 3, True)), ((5, 1), big_group(4, 4, 4, True)),
           ((9, 0), no_count)]
    two = [((2, 2), big_group(0, 3, 5)), ((2, 3), big_group(4, 0, 6)), ((5, 2), big_group(7, 5, 7, True)), ((11, 2), big_group(3, 3, 8))]
    parts = [one, two]
    hosts = [host_matches([g for _, g in p], [k for k, _ in p]) for p in parts]
    for max_dets in ((1, 10, 100), (1, 3, 100)):                      # 3 cuts the groups of 12, 5, 6, 4 and 7 detections
        acc = cocoeval.accumulate(hosts, max_dets=max_dets)
        assert acc["categories"] == [2, 5, 9, 11]
        want = oracle_accumulate(parts, [2, 5, 9, 11], max_dets)
        assert (want["precision"][:, :, 2] == -1).all() and (want["precision"][:, :, 0, 0, 2] > -1).all()
        assert_same(acc, want)
    single = cocoeval.accumulate(hosts[0])
    assert_same(single, oracle_accumulate([one], [2, 5, 9], (1, 10, 100)))
    # without categories: one K, the groups are images
    plain = [((None, i), big_group(8, 6, 20 + i)) for i in range(4)]
    acc = cocoeval.accumulate(host_matches([g for _, g in plain], [k for k, _ in plain]))
    assert acc["categories"] == [None]
    assert_same(acc, oracle_accumulate([plain], [None], (1, 10, 100)))


def test_accumulate_perfect_detections_and_refusals():
    from camouflaged_vlm_amd import cocoeval
    area = np.array([500, 2000, 20000, 900])
    grp = dict(inter=np.diag(area), det_area=area, scores=np.array([0.9, 0.8, 0.7, 0.6], dtype=np.float32), gt_area=area, range_area=None,
               iscrowd=np.zeros(4, dtype=np.uint8))
    h = host_matches([grp, grp], [(None, 0), (None, 1)])
    acc = cocoeval.accumulate(h)
    assert (acc["precision"][..., 2] == 1.0).all()
    stats = cocoeval.summarize(acc)
    assert stats[:6] == [1.0] * 6 and stats[6] == 0.25 and stats[7:] == [1.0] * 5
    for bad in (dict(max_dets=(10, 1, 100)), dict(max_dets=(1, 10, 101)), dict(max_dets=()), dict(max_dets=(0, 1, 2)), dict(rec_thrs=[[0.5]])):
        with pytest.raises(ValueError):
            cocoeval.accumulate(h, **bad)
    with pytest.raises(ValueError):
        cocoeval.accumulate([h, dict(h, max_det=50)])
    with pytest.raises(ValueError):
        cocoeval.accumulate([h, dict(h, keys=[(1, 0), (1, 1)])])
    with pytest.raises(ValueError):
        cocoeval.accumulate(dict(h, status=1))
    with pytest.raises(ValueError):
        cocoeval.accumulate([])
    with pytest.raises(ValueError):
        cocoeval.summarize(cocoeval.accumulate(h, max_dets=(1, 10)))
