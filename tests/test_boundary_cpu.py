"""Boundary IoU without a GPU: the radius table; the oracle (tests/boundary_oracle.py: the window definition) against
scipy's iterated erosion and against the consequences §25 states; cvlm_debug_mask_boundary_sized_host -- the kernels' per-thread
functions run sequentially, with the kernels' segments -- against the oracle on every shape, radius and content of the GPU list;
cvlm_debug_coco_match_boundary_host against the published loops over min(mask IoU, boundary IoU) on the tie-heavy groups of
tests/test_match_cpu.py; every ValueError of boundary_request with the launchers replaced by a recorder; every CVLM_E_BADARG; the
exports.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

import boundary_oracle as BO
import match_oracle as MO
from test_match_cpu import SMALL_RNGS, ragged_groups, refusal_cases, shape_cases

TABLES = ("dt_order", "dt_match", "dt_ignore", "gt_match", "gt_ignore")


def host_entry():
    from camouflaged_vlm_amd import hip
    return hip.mask_boundary_sized_host


def host_match():
    from camouflaged_vlm_amd import hip
    return hip.coco_match_boundary_host


# ---- the radius and the oracle ---------------------------------------------------------------------------------------------------------------
RADII = {(480, 640): 16, (427, 640): 15, (1024, 1024): 29, (100, 75): 2, (1, 1): 1, (16384, 16384): 463,
         (300, 125): 6,       # 0.02 * 325 = 6.5: half to even
         (700, 240): 15}      # 0.02 * 740 = 14.8: no tie; beside it (1500, 800) = 0.02 * 1700 = 34 exactly


def test_boundary_radius_is_the_published_one():
    from camouflaged_vlm_amd import engine
    for (h, w), d in RADII.items():
        assert engine.boundary_radius(h, w) == BO.boundary_radius(h, w) == d, (h, w)
    assert engine.boundary_radius(1500, 800) == 34 and engine.boundary_radius(60, 25) == 1       # 1.3
    assert engine.boundary_radius(480, 640, 0.05) == 40 and engine.boundary_radius(100, 75, 0.1) == 12       # 12.5: half to even
    assert engine.boundary_radius(3, 4, 0.1) == 1                     # 0.5 rounds to 0: at least 1
    assert isinstance(engine.boundary_radius(480, 640), int)


def test_oracle_equals_scipy_iterated_erosion():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(25)
    for n in range(40):
        h, w = int(rng.integers(1, 50)), int(rng.integers(1, 70))
        d = int(rng.integers(1, 9))
        x = rng.random((h, w)) < (0.98 if n % 2 else 0.8)
        want = ndimage.binary_erosion(x, np.ones((3, 3), dtype=bool), iterations=d, border_value=0)
        assert np.array_equal(BO.erode(x, d), want), (h, w, d)


def test_oracle_has_the_stated_consequences():
    rng = np.random.default_rng(26)
    for h, w, d in ((33, 65, 2), (40, 40, 5), (9, 70, 4), (70, 9, 4), (21, 21, 10), (21, 21, 11)):
        x = rng.random((h, w)) < 0.97
        ero, b = BO.erode(x, d), BO.boundary(x, d)
        assert not (ero & ~x).any()
        assert not ero[:d].any() and not ero[h - d:].any() and not ero[:, :d].any() and not ero[:, w - d:].any()
        if 2 * d + 1 > min(h, w):
            assert np.array_equal(b, x)
        ys, xs = np.nonzero(x)
        yb, xb = np.nonzero(b)
        assert (ys.min(), ys.max(), xs.min(), xs.max()) == (yb.min(), yb.max(), xb.min(), xb.max())
        assert not BO.boundary(np.zeros((h, w), dtype=bool), d).any()
    full = np.ones((20, 30), dtype=bool)
    frame = full.copy()
    frame[3:17, 3:27] = False
    assert np.array_equal(BO.boundary(full, 3), frame)                # a full plane: the frame of width d
    assert np.array_equal(BO.erode(np.ones((7, 9), dtype=bool), 3), np.pad(np.ones((1, 3), dtype=bool), 3))     # 2 d + 1 = min(h, w)


# ---- the host entry against the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", BO.HEIGHTS)
def test_host_entry_equals_the_oracle(h):
    """Every width, every radius of the list and every content at one height: the contents of one (width, radius) are one call."""
    for w in BO.WIDTHS:
        named = BO.contents(h, w, seed=1000 * h + w)
        planes = [m for _, m in named]
        for d in BO.radii_of(h, w):
            res = BO.run(host_entry(), planes, [d] * len(planes))
            assert res["status"] == 0
            BO.check(res, planes, [d] * len(planes))


def test_host_entry_large_radius_and_seams():
    rng = np.random.default_rng(27)
    wide = rng.random((40, 1100)) < 0.999
    wide[:, 5:1000] = True
    tall = np.zeros((389, 70), dtype=bool)                            # d = 3: segments of 128 rows, seams at 128, 256, 384
    tall[100:256, 2:60] = True                                        # ends exactly at a seam
    tall[256:300, 30:69] = True                                       # starts exactly at one
    tall[380:389, :] = True
    taller = rng.random((500, 40)) < 0.995                            # d = 40: segments of 160 rows
    taller[100:320] = True
    planes, radii = [wide, tall, taller, tall], [463, 3, 40, 1]
    res = BO.run(host_entry(), planes, radii)
    assert res["status"] == 0
    BO.check(res, planes, radii)
    assert res["area"][0] == wide.sum() and 0 < res["area"][1] < tall.sum()


def ragged_planes():
    rng = np.random.default_rng(28)
    planes = [rng.random(s) < 0.9 for s in BO.RAGGED]
    radii = [1, 2, 1, 16, 17, BO.boundary_radius(97, 131), 1]
    return planes, radii


def test_host_entry_ragged_planes_second_call_null_area_and_dirty_pads():
    planes, radii = ragged_planes()
    res = BO.run(host_entry(), planes, radii)
    assert res["status"] == 0
    BO.check(res, planes, radii)
    other = [~p for p in planes]
    again = BO.run(host_entry(), other, radii, outs=res["outs"])    # into used outputs and a used workspace
    assert again["status"] == 0
    BO.check(again, other, radii)
    bare = BO.run(host_entry(), planes, radii, area=False, shift=4, dirty_pads=True)
    BO.check(bare, planes, radii, area=False)


def refusals():
    """(name, keyword arguments of BO.run, radii, refused planes, untouched planes) on four planes."""
    sizes = [(5, 40), (9, 33), (4, 64), (3, 7)]
    _, off, nbytes, _ = BO.tables(sizes)
    dims = np.asarray(sizes, dtype=np.int32)
    shifted, odd, beyond, negative = off.copy(), off.copy(), off.copy(), off.copy()
    shifted[1] += 4
    odd[1] += 2
    beyond[4] = nbytes + 4
    negative[0] = -4
    zero_h, big_w = dims.copy(), dims.copy()
    zero_h[2, 0] = 0
    big_w[0, 1] = 16385
    ok = [1, 1, 1, 1]
    return sizes, [("a bad offset", dict(offsets=shifted), ok, (0, 1), ()),
                   ("an offset off a word", dict(offsets=odd), ok, (), (0, 1)),
                   ("a slice that leaves the buffer", dict(offsets=beyond), ok, (), (3,)),
                   ("a negative offset", dict(offsets=negative), ok, (), (0,)),
                   ("radius 0", {}, [1, 0, 1, 1], (1,), ()),
                   ("radius 16385", {}, [1, 1, 1, 16385], (3,), ()),
                   ("a negative radius", {}, [-1, 1, 1, 1], (0,), ()),
                   ("height 0", dict(dims=zero_h), ok, (2,), ()),
                   ("width 16385", dict(dims=big_w), ok, (0,), ())]


@pytest.mark.parametrize("name", [c[0] for c in refusals()[1]])
def test_host_entry_refuses_whole_planes(name):
    sizes, cases = refusals()
    _, kw, radii, refused, untouched = next(c for c in cases if c[0] == name)
    rng = np.random.default_rng(29)
    planes = [rng.random(s) < 0.9 for s in sizes]
    res = BO.run(host_entry(), planes, radii, **kw)
    assert res["status"] == 1
    BO.check(res, planes, radii, refused=refused, untouched=untouched)
    whole = BO.run(host_entry(), planes, [1] * 4, outs=res["outs"])                     # the status is zeroed again
    assert whole["status"] == 0
    BO.check(whole, planes, [1] * 4)


# ---- the boundary matching's host entry -------------------------------------------------------------------------------------------------------
def test_minimum_of_two_ious_by_hand():
    """One detection, one annotation: mask IoU 9 / 11 passes the seven thresholds 0.5 .. 0.8; a boundary IoU of 3 / 6 passes 0.5 alone;
    a refused boundary pair matches nothing; a boundary intersection of 0 gives IoU 0; a boundary IoU of 1 leaves the mask's."""
    base = dict(inter=np.array([[9]]), det_area=np.array([10]), gt_area=np.array([10]), scores=np.array([0.5], dtype=np.float32),
                range_area=None, iscrowd=np.zeros(1, dtype=np.uint8), det_area_b=np.array([4]))
    for ib, gab, upto in ((3, 5, 1), (-1, 4, 0), (0, 4, 0), (4, 4, 7)):
        g = dict(base, inter_b=np.array([[ib]]), gt_area_b=np.array([gab]))
        res = BO.run_match(host_match(), [g])
        assert res["status"] == 0
        assert res["dt_match"][0, :, 0].tolist() == [0] * upto + [-1] * (10 - upto), ib
        BO.check_groups(res, [g])


@pytest.mark.parametrize("name", [c[0] for c in shape_cases()])
def test_host_match_equals_the_oracle(name):
    _, groups, kw = next(c for c in shape_cases() if c[0] == name)
    groups = [BO.with_boundary(g, 700 + i) for i, g in enumerate(groups)]
    res = BO.run_match(host_match(), groups, guard=16, **kw)
    assert res["status"] == 0
    BO.check_groups(res, groups, **kw)
    if sum(g["inter"].size for g in groups) > 100:                    # the minimum decides something the mask alone would not
        from camouflaged_vlm_amd import hip
        plain = MO.run_entry(hip.coco_match_host, MO.tables(groups), **kw)
        assert any(not np.array_equal(plain[k], res[k]) for k in TABLES)


def test_host_match_ragged_groups_and_refusals():
    groups = [BO.with_boundary(g, 800 + i) for i, g in enumerate(ragged_groups())]
    res = BO.run_match(host_match(), groups, area_rngs=SMALL_RNGS, max_det=20, guard=16)
    assert res["status"] == 0
    BO.check_groups(res, groups, area_rngs=SMALL_RNGS, max_det=20)
    for name, groups, tabs, refused in refusal_cases():
        groups = [BO.with_boundary(g, 900 + i) for i, g in enumerate(groups)]
        res = BO.run_match(host_match(), groups, tabs=tabs, area_rngs=SMALL_RNGS, guard=16)
        assert res["status"] == 1, name
        BO.check_groups(res, groups, area_rngs=SMALL_RNGS, refused=refused)


# ---- CVLM_E_BADARG and the exports --------------------------------------------------------------------------------------------------------
def test_every_badarg_of_the_boundary_entry():
    from camouflaged_vlm_amd import hip
    lib = hip.load()
    sizes = [(5, 40), (3, 7)]
    dims, off, nbytes, max_words = BO.tables(sizes, guard=0)
    big = torch.zeros(3 * nbytes + 64, dtype=torch.uint8)
    keep = dict(big=big, offsets=torch.from_numpy(off), dims=torch.from_numpy(dims), radius=torch.ones(3, dtype=torch.int32),
                area=torch.zeros(3, dtype=torch.int32), status=torch.zeros(2, dtype=torch.int32))
    base = big.data_ptr()
    good = dict(bits=base, n_bytes=nbytes, offsets=keep["offsets"].data_ptr(), dims=keep["dims"].data_ptr(), radius=keep["radius"].data_ptr(),
                P=2, max_words=max_words, workspace=base + nbytes, out_bits=base + 2 * nbytes, out_area=keep["area"].data_ptr(),
                status=keep["status"].data_ptr())
    order = list(good)

    def call(dev: bool, **change):
        args = [dict(good, **change)[k] for k in order]
        return lib.cvlm_mask_boundary_sized(*args, None) if dev else lib.cvlm_debug_mask_boundary_sized_host(*args)

    assert call(False) == 0 and call(False, out_area=None) == 0
    bad = [{k: None} for k in ("bits", "offsets", "dims", "radius", "workspace", "out_bits", "status")]
    bad += [{k: good[k] + 2} for k in ("bits", "dims", "radius", "workspace", "out_bits", "out_area", "status")]
    bad += [dict(offsets=good["offsets"] + 4), dict(P=0), dict(P=65536), dict(n_bytes=3), dict(n_bytes=0), dict(max_words=0),
            dict(max_words=16384 * 512 + 1)]
    bad += [dict(out_bits=base), dict(out_bits=base + nbytes - 4), dict(workspace=base + 4), dict(workspace=base + 2 * nbytes - 4),
            dict(out_bits=base + nbytes + 4), dict(workspace=base, bits=base + nbytes - 4)]
    for change in bad:
        for dev in (False, True):                                     # refused before the device is touched: no GPU is needed
            assert call(dev, **change) == -1, change
    assert call(False, out_bits=base + nbytes, workspace=base + 2 * nbytes) == 0          # ranges that touch do not meet


def test_every_badarg_of_the_boundary_matching():
    from camouflaged_vlm_amd import hip
    from test_match_cpu import make_group
    lib = hip.load()
    g = [BO.with_boundary(make_group(3, 2, 1), 1)]
    tabs = dict(MO.tables(g), **BO.boundary_tables(g))
    T, A, ND, NG, N = 10, 4, 3, 2, 6
    keep = {k: torch.from_numpy(v.copy()) for k, v in tabs.items()}
    keep.update(iou_thrs=torch.from_numpy(MO.IOU_THRS.copy()), area_rngs=torch.tensor(MO.AREA_RNGS, dtype=torch.float64),
                dt_order=torch.zeros(ND + 1, dtype=torch.int32), dt_match=torch.zeros(A * T * ND + 1, dtype=torch.int32),
                dt_ignore=torch.zeros(A * T * ND, dtype=torch.uint8), gt_match=torch.zeros(A * T * NG + 1, dtype=torch.int32),
                gt_ignore=torch.zeros(A * NG, dtype=torch.uint8), status=torch.zeros(2, dtype=torch.int32))
    order = ["det_offsets", "gt_offsets", "pair_offsets", "E", "inter", "N", "det_area", "score", "ND", "gt_area", "gt_range_area", "gt_crowd",
             "NG", "iou_thrs", "T", "area_rngs", "A", "max_det", "inter_b", "det_area_b", "gt_area_b", "dt_order", "dt_match", "dt_ignore",
             "gt_match", "gt_ignore", "status"]
    good = {k: v.data_ptr() for k, v in keep.items()}
    good.update(E=1, N=N, ND=ND, NG=NG, T=T, A=A, max_det=100)

    def call(dev: bool, **change):
        args = [dict(good, **change)[k] for k in order]
        return lib.cvlm_coco_match_boundary(*args, None) if dev else lib.cvlm_debug_coco_match_boundary_host(*args)

    assert call(False) == 0
    bad = [{k: None} for k in ("inter_b", "det_area_b", "gt_area_b", "inter", "status", "iou_thrs")]
    bad += [{k: good[k] + 2} for k in ("inter_b", "det_area_b", "gt_area_b", "det_area")]
    bad += [dict(E=0), dict(T=17), dict(A=9), dict(max_det=0)]
    for change in bad:
        for dev in (False, True):
            assert call(dev, **change) == -1, change
    zeros32, zeros64 = torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
    assert call(False, N=0, inter=None, inter_b=None, ND=0, det_area=None, det_area_b=None, score=None, dt_order=None, dt_match=None,
                dt_ignore=None, det_offsets=zeros32.data_ptr(), pair_offsets=zeros64.data_ptr()) == 0


def test_exports_stay_at_abi_12():
    from camouflaged_vlm_amd import hip
    lib = hip.load()
    assert lib.cvlm_abi_version() == hip.ABI_VERSION == 12
    names = ("cvlm_mask_boundary_sized", "cvlm_debug_mask_boundary_sized_host", "cvlm_coco_match_boundary", "cvlm_debug_coco_match_boundary_host")
    for name in names:
        assert name in hip.EXPORTS and hasattr(lib, name) and hip.ABI[name][0] is ctypes.c_int32
    assert {n for n in names if n in hip._STREAMED} == {"cvlm_mask_boundary_sized", "cvlm_coco_match_boundary"}


# ---- boundary_request ---------------------------------------------------------------------------------------------------------------------------
SIZES = [(480, 640), (100, 75), (1, 1)]

BAD_REQUESTS = {
    "ratio zero": dict(dilation_ratio=0.0),
    "ratio negative": dict(dilation_ratio=-0.02),
    "ratio infinite": dict(dilation_ratio=float("inf")),
    "ratio NaN": dict(dilation_ratio=float("nan")),
    "ratio a bool": dict(dilation_ratio=True),
    "ratio a string": dict(dilation_ratio="0.02"),
    "ratio None": dict(dilation_ratio=None),
    "ratio that gives a radius above 16384": dict(dilation_ratio=30.0),
    "radius and a ratio": dict(radius=[1, 2, 3], dilation_ratio=0.05),
    "radius too short": dict(radius=[1, 2]),
    "radius too long": dict(radius=[1, 2, 3, 4]),
    "radius zero": dict(radius=[1, 0, 3]),
    "radius 16385": dict(radius=[1, 16385, 3]),
    "radius a bool": dict(radius=[1, True, 3]),
    "one radius a bool": dict(radius=True),
    "radius a float": dict(radius=[1, 2.0, 3]),
    "radius a string": dict(radius="123"),
    "one radius zero": dict(radius=0),
}


@pytest.fixture
def launches(monkeypatch):
    """Every launcher the boundary calls could reach, replaced by a recorder."""
    from camouflaged_vlm_amd import hip
    seen = []
    for name in ("mask_boundary_sized", "mask_boundary_sized_host", "coco_match_boundary", "coco_match", "mask_inter_sized"):
        monkeypatch.setattr(hip, name, lambda *a, _n=name, **k: seen.append(_n))
    return seen


@pytest.mark.parametrize("name", list(BAD_REQUESTS))
def test_bad_requests_raise_and_launch_nothing(name, launches):
    from camouflaged_vlm_amd import engine
    with pytest.raises(ValueError, match="mask_boundary_sized"):
        engine.boundary_request(SIZES, **BAD_REQUESTS[name])
    with pytest.raises(ValueError, match="coco_match"):
        engine.boundary_request(SIZES, who="coco_match", **BAD_REQUESTS[name])
    assert launches == []


def test_request_tables(launches):
    from camouflaged_vlm_amd import engine
    r = engine.boundary_request(SIZES)
    assert r.dtype == np.int32 and r.tolist() == [16, 2, 1]
    assert engine.boundary_request(SIZES, dilation_ratio=0.05).tolist() == [40, 6, 1]
    assert engine.boundary_request(SIZES, radius=[3, 16384, 1]).tolist() == [3, 16384, 1]
    assert engine.boundary_request(SIZES, radius=7).tolist() == [7, 7, 7]
    assert engine.boundary_request(SIZES, dilation_ratio=np.float32(0.5)).dtype == np.int32
    assert engine.boundary_request([(16384, 16384)]).tolist() == [463]
    assert engine.BOUNDARY_MAX_RADIUS == 16384 and engine.BOUNDARY_RATIO == 0.02
    assert launches == []
