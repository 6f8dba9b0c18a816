"""Contours of sized planes without a device: the definition (tests/contour_oracle.py, a sequential walk over unit
edges) against its stated consequences -- areas that sum to the popcount, ring counts that are scipy's component counts of the plane
and of its framed complement, the round trip through §21's rasteriser --, cvlm_debug_mask_contour_host (the kernels' maps and
successors, run sequentially) against the definition on every plane of the device list, every refusal, every CVLM_E_BADARG, every
ValueError of `contour_request` with the launchers replaced by a recorder, and `MaskContours` on host tensors."""
import ctypes

import numpy as np
import pytest
import torch
from scipy import ndimage

import contour_oracle as CO
import poly_oracle as PO

DENSITIES = (0.02, 0.2, 0.5, 0.8, 0.97)
STRUCT = {4: ndimage.generate_binary_structure(2, 1), 8: ndimage.generate_binary_structure(2, 2)}


def random_planes(n_per_density: int = 6, seed: int = 2600):
    rng = np.random.default_rng(seed)
    out = []
    for d in DENSITIES:
        for _ in range(n_per_density):
            h, w = int(rng.integers(1, 21)), int(rng.integers(1, 41))
            out.append(rng.random((h, w)) < d)
    return out


def xor_of_rings(rings, h: int, w: int) -> np.ndarray:
    out = np.zeros((h, w), dtype=bool)
    for r in rings:
        out ^= PO.plane_of(r.reshape(-1).astype(np.float64).tolist(), h, w)
    return out


# ---- the definition ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
def test_oracle_has_the_stated_consequences(connectivity):
    """1: the signed areas sum to the popcount.  2: outer rings = components under `connectivity`, holes = components of the framed
    complement under the other one, less the outside.  3: an outer ring's first edge heads east, a hole's south.  Even vertex counts,
    alternating horizontal and vertical segments."""
    for m in random_planes():
        rings = CO.rings_of(m, connectivity)
        areas = [CO.signed_area(r) for r in rings]
        assert sum(areas) == int(m.sum())
        outer, holes = sum(a > 0 for a in areas), sum(a < 0 for a in areas)
        assert outer + holes == len(rings)
        assert outer == ndimage.label(m, structure=STRUCT[connectivity])[1] == CO.components(m, connectivity)
        framed = np.ones((m.shape[0] + 2, m.shape[1] + 2), dtype=bool)
        framed[1:-1, 1:-1] = ~m
        assert holes == ndimage.label(framed, structure=STRUCT[12 - connectivity])[1] - 1 == CO.framed_holes(m, connectivity)
        for r, a in zip(rings, areas):
            assert len(r) >= 4 and len(r) % 2 == 0
            step = np.roll(r, -1, axis=0) - r
            assert ((step[:, 0] == 0) != (step[:, 1] == 0)).all()                    # every segment is horizontal or vertical
            assert (step[0::2, 1] == 0).all() != (step[0::2, 0] == 0).all()          # and they alternate
            east, south = step[0, 0] > 0 and step[0, 1] == 0, step[0, 1] > 0 and step[0, 0] == 0
            assert east if a > 0 else south


@pytest.mark.parametrize("connectivity", [4, 8])
def test_oracle_round_trip_through_the_polygon_rasteriser(connectivity):
    """4: each ring as one polygon of §21, the planes XORed, is the mask; without holes the OR of one annotation is the mask too."""
    seen_plain = 0
    for m in random_planes(4, seed=2601):
        h, w = m.shape
        rings = CO.rings_of(m, connectivity)
        assert np.array_equal(xor_of_rings(rings, h, w), m)
        if rings and all(CO.signed_area(r) > 0 for r in rings):
            seen_plain += 1
            assert np.array_equal(PO.expected([r.reshape(-1).astype(np.float64).tolist() for r in rings], h, w), m)
    assert seen_plain >= 3


def test_oracle_by_hand():
    one = np.ones((1, 1), dtype=bool)
    assert [r.tolist() for r in CO.rings_of(one, 8)] == [[[0, 0], [1, 0], [1, 1], [0, 1]]]
    pair = np.eye(2, dtype=bool)
    assert [r.tolist() for r in CO.rings_of(pair, 8)] == [[[0, 0], [1, 0], [1, 1], [2, 1], [2, 2], [1, 2], [1, 1], [0, 1]]]
    assert [r.tolist() for r in CO.rings_of(pair, 4)] == [[[0, 0], [1, 0], [1, 1], [0, 1]], [[1, 1], [2, 1], [2, 2], [1, 2]]]
    ring = np.ones((3, 3), dtype=bool)
    ring[1, 1] = False
    assert [r.tolist() for r in CO.rings_of(ring, 8)] == [[[0, 0], [3, 0], [3, 3], [0, 3]], [[1, 1], [1, 2], [2, 2], [2, 1]]]
    assert CO.flat(CO.rings_of(ring, 8))[2] == (1, 1)


# ---- the host entry ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("h", CO.HEIGHTS)
def test_host_entry_equals_the_oracle(h, connectivity):
    for w in CO.WIDTHS:
        planes = [m for _, m in CO.contents(h, w, seed=1000 * h + w)]
        res = CO.run(planes, connectivity, host=True)
        assert res["status"] == (0, 0)
        CO.check(res, planes, connectivity)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_host_entry_chain_comb_and_many_rings(connectivity):
    named = CO.big_cases()
    planes = [m for _, m in named]
    res = CO.run(planes, connectivity, host=True)
    assert res["status"] == (0, 0)
    CO.check(res, planes, connectivity)
    assert res["n_vertices"][0] == 1200 and tuple(res["n_rings"][0]) == ((1, 0) if connectivity == 8 else (300, 0))
    assert res["n_vertices"][1] > 1024 and tuple(res["n_rings"][1]) == (1, 0)
    assert res["n_rings"][2].sum() > 100


def test_host_entry_ragged_planes_second_call_and_dirty_pads():
    planes = CO.ragged_planes()
    res = CO.run(planes, 8, host=True)
    assert res["status"] == (0, 0)
    CO.check(res, planes, 8)
    dirty = CO.run(planes, 8, host=True, shift=4, dirty_pads=True)
    CO.same(res, dict(dirty, outs=None))
    empty = [np.zeros(p.shape, dtype=bool) for p in planes]
    again = CO.run(empty, 4, host=True, outs=res["outs"])                                # into used outputs: nothing is written, total is 0
    assert again["status"] == (0, 0) and again["n_vertices"].sum() == 0
    CO.check(again, empty, 4)


def refusals():
    """(name, keyword arguments of CO.run, refused planes, planes one short, (count status, emit status)) on four planes."""
    sizes = [(5, 40), (9, 33), (4, 64), (3, 7)]
    _, off, nbytes, _ = CO.tables(sizes)
    dims = np.asarray(sizes, dtype=np.int32)
    shifted, odd, beyond, negative = off.copy(), off.copy(), off.copy(), off.copy()
    shifted[1] += 4
    odd[1] += 2
    beyond[4] = nbytes + 4
    negative[0] = -4
    zero_h, big_w = dims.copy(), dims.copy()
    zero_h[2, 0] = 0
    big_w[0, 1] = 16385
    return sizes, [("a shifted offset", dict(offsets=shifted), (0, 1), (), (1, 1)),
                   ("an odd offset", dict(offsets=odd), (0, 1), (), (1, 1)),
                   ("a negative offset", dict(offsets=negative), (0,), (), (1, 1)),
                   ("a slice past the buffer", dict(offsets=beyond), (3,), (), (1, 1)),
                   ("height 0", dict(dims=zero_h), (2,), (), (1, 1)),
                   ("width 16385", dict(dims=big_w), (0,), (), (1, 1)),
                   ("a vertex table one short for a middle plane", dict(short=1), (), (1,), (0, 1))]


@pytest.mark.parametrize("name", [c[0] for c in refusals()[1]])
def test_host_entry_refuses_whole_planes(name):
    sizes, cases = refusals()
    _, kw, refused, short, status = next(c for c in cases if c[0] == name)
    rng = np.random.default_rng(26)
    planes = [rng.random(s) < 0.7 for s in sizes]
    res = CO.run(planes, 8, host=True, **kw)
    assert res["status"] == status
    CO.check(res, planes, 8, refused=refused, short=short)
    whole = CO.run(planes, 8, host=True)                              # the status is zeroed by every call
    assert whole["status"] == (0, 0)
    CO.check(whole, planes, 8)


# ---- CVLM_E_BADARG and the exports --------------------------------------------------------------------------------------------------------
def test_every_badarg_of_the_contour_entries():
    from camouflaged_vlm_amd import hip
    lib = hip.load()
    sizes = [(5, 40), (3, 7)]
    dims, off, nbytes, max_words = CO.tables(sizes, guard=0)
    total, P = 12, 2
    need = lib.cvlm_mask_contour_workspace_bytes(P, total, max_words)
    assert need == 16 + 20 * P * (2 * max_words + 2) + 28 * total
    big = torch.zeros(nbytes + 4 * total + 16 + total + 16 + need + 64, dtype=torch.uint8)
    keep = dict(big=big, offsets=torch.from_numpy(off), dims=torch.from_numpy(dims), n_vertices=torch.zeros(3, dtype=torch.int32),
                vo=torch.tensor([0, 4, 8, 8], dtype=torch.int64), n_rings=torch.zeros(5, dtype=torch.int32),
                status=torch.zeros(2, dtype=torch.int32))
    base = big.data_ptr()
    base += -base % 16
    xy = base + (nbytes + 15) // 16 * 16
    start = xy + 4 * total
    ws = start + (total + 15) // 16 * 16
    planes = dict(bits=base, n_bytes=nbytes, offsets=keep["offsets"].data_ptr(), dims=keep["dims"].data_ptr(), P=P, connectivity=8)
    count = dict(planes, max_words=max_words, n_vertices=keep["n_vertices"].data_ptr(), status=keep["status"].data_ptr())
    emit = dict(planes, max_words=max_words, vertex_offsets=keep["vo"].data_ptr(), round_vertices=total, xy=xy, ring_start=start,
                n_rings=keep["n_rings"].data_ptr(), total=total, status=keep["status"].data_ptr(), workspace=ws, workspace_bytes=need)
    host = dict(planes, n_vertices=keep["n_vertices"].data_ptr(), vertex_offsets=keep["vo"].data_ptr(), xy=xy, ring_start=start,
                n_rings=keep["n_rings"].data_ptr(), total=total, status=keep["status"].data_ptr())

    def call(fn, good, stream, **change):
        args = [dict(good, **change)[k] for k in good]
        return fn(*args, None) if stream else fn(*args)

    c = lambda **ch: call(lib.cvlm_mask_contour_count, count, True, **ch)
    e = lambda **ch: call(lib.cvlm_mask_contour_emit, emit, True, **ch)
    h = lambda **ch: call(lib.cvlm_debug_mask_contour_host, host, False, **ch)
    assert h() == 0 and h(vertex_offsets=None, xy=None, ring_start=None, n_rings=None) == 0
    shared = [{k: None} for k in ("bits", "offsets", "dims")] + [{k: planes[k] + 2} for k in ("bits", "dims")]
    shared += [dict(offsets=planes["offsets"] + 4), dict(P=0), dict(P=65536), dict(n_bytes=3), dict(n_bytes=0)]
    shared += [dict(connectivity=v) for v in (0, 6, -8, 16)]
    sized = [dict(max_words=0), dict(max_words=16384 * 512 + 1)]
    for change in shared + sized + [dict(n_vertices=None), dict(status=None), dict(n_vertices=count["n_vertices"] + 2),
                                    dict(status=count["status"] + 2), dict(n_vertices=base), dict(status=base + nbytes - 4),
                                    dict(n_vertices=count["status"])]:
        assert c(**change) == -1, change
    outputs = [{k: None} for k in ("vertex_offsets", "xy", "ring_start", "n_rings", "status")]
    outputs += [{k: emit[k] + 2} for k in ("xy", "n_rings", "status")] + [dict(vertex_offsets=emit["vertex_offsets"] + 4), dict(total=-1)]
    outputs += [dict(xy=base), dict(xy=base + nbytes - 4), dict(ring_start=base + nbytes - 1), dict(ring_start=xy + 4 * total - 1),
                dict(n_rings=xy), dict(status=start)]
    for change in shared + outputs:
        assert e(**change) == -1, change
        assert h(**change) == -1, change
    for change in sized + [dict(workspace=None), dict(workspace=ws + 4), dict(workspace_bytes=need - 1), dict(workspace_bytes=0),
                           dict(round_vertices=-1), dict(round_vertices=P * (1 << 22) + 1), dict(round_vertices=total + 1),
                           dict(workspace=base), dict(workspace=xy + 4 * total - 16), dict(workspace=start)]:
        assert e(**change) == -1, change
    assert h(total=0, xy=None, ring_start=None, vertex_offsets=torch.zeros(3, dtype=torch.int64).data_ptr()) == 0       # empty tables need no outputs
    for bad in ((0, 1, 1), (65536, 1, 1), (1, -1, 1), (1, (1 << 22) + 1, 1), (1, 1, 0), (1, 1, 16384 * 512 + 1)):
        assert lib.cvlm_mask_contour_workspace_bytes(*bad) == -1, bad


def test_exports_stay_at_abi_12():
    from camouflaged_vlm_amd import hip
    lib = hip.load()
    assert lib.cvlm_abi_version() == hip.ABI_VERSION == 12
    names = ("cvlm_mask_contour_count", "cvlm_mask_contour_emit", "cvlm_debug_mask_contour_host")
    for name in names:
        assert name in hip.EXPORTS and hasattr(lib, name) and hip.ABI[name][0] is ctypes.c_int32
    assert hip.ABI["cvlm_mask_contour_workspace_bytes"][0] is ctypes.c_int64
    assert {n for n in names if n in hip._STREAMED} == {"cvlm_mask_contour_count", "cvlm_mask_contour_emit"}


# ---- contour_request, contour_rounds and MaskContours ---------------------------------------------------------------------------------------
SIZES = [(480, 640), (100, 75), (1, 1)]

BAD_REQUESTS = {
    "connectivity 6": dict(connectivity=6),
    "connectivity 0": dict(connectivity=0),
    "connectivity a bool": dict(connectivity=True),
    "connectivity a float": dict(connectivity=8.0),
    "connectivity a string": dict(connectivity="8"),
    "connectivity None": dict(connectivity=None),
    "no sizes": dict(sizes=[]),
    "sizes a string": dict(sizes="480x640"),
    "sizes no sequence": dict(sizes=480),
    "a size of three": dict(sizes=[(1, 2, 3)]),
    "a size a bool": dict(sizes=[(True, 4)]),
    "a size a float": dict(sizes=[(4.0, 4)]),
    "height 0": dict(sizes=[(0, 4)]),
    "width 16385": dict(sizes=[(4, 16385)]),
    "too many planes": dict(sizes=[(1, 1)] * 65536),
}


@pytest.fixture
def launches(monkeypatch):
    """Every launcher the contour call could reach, replaced by a recorder."""
    from camouflaged_vlm_amd import hip
    seen = []
    for name in ("mask_contour_count", "mask_contour_emit", "mask_contour_host"):
        monkeypatch.setattr(hip, name, lambda *a, _n=name, **k: seen.append(_n))
    return seen


@pytest.mark.parametrize("name", list(BAD_REQUESTS))
def test_bad_requests_raise_and_launch_nothing(name, launches):
    from camouflaged_vlm_amd import engine
    kw = dict(BAD_REQUESTS[name])
    sizes = kw.pop("sizes", SIZES)
    with pytest.raises(ValueError, match="mask_contours_sized"):
        engine.contour_request(sizes, **kw)
    with pytest.raises(ValueError, match="someone"):
        engine.contour_request(sizes, who="someone", **kw)
    assert launches == []


def test_the_call_refuses_what_is_no_sized_masks_before_any_launch(launches):
    from camouflaged_vlm_amd import engine
    util = engine.MaskUtilities.__new__(engine.MaskUtilities)
    host = engine.SizedMasks(bits=torch.zeros(4, dtype=torch.uint8), offsets=torch.tensor([0, 4]), area=None, box=None,
                             status=torch.zeros(1, dtype=torch.int32), sizes=[(1, 1)])
    for bad in (None, torch.zeros(4, dtype=torch.uint8), host):
        with pytest.raises(ValueError, match="mask_contours_sized"):
            engine.MaskUtilities.mask_contours_sized(util, bad)
    assert launches == []


def test_request_and_rounds(launches):
    from camouflaged_vlm_amd import engine, hip
    assert engine.contour_request(SIZES) == (SIZES, 8)
    assert engine.contour_request([[np.int32(3), np.int64(5)]], connectivity=np.int64(4)) == ([(3, 5)], 4)
    assert engine.CONTOUR_MAX_VERTS == 1 << 22
    need = hip.mask_contour_workspace_bytes
    one = need(1, 100, 8)
    nv = [100, 100, 100, 0, 100, 100, 100]
    assert engine.contour_rounds(nv, 8, 1 << 30, need) == [(0, 7, 600, need(7, 600, 8))]
    three = engine.contour_rounds(nv, 8, need(3, 300, 8), need)
    assert [(a, b, rv) for a, b, rv, _ in three] == [(0, 3, 300), (3, 6, 200), (6, 7, 100)]
    assert [r[:2] for r in engine.contour_rounds(nv, 8, one - 1, need)] == [(p, p + 1) for p in range(7)]      # a plane above the cap runs alone
    assert all(r[3] == need(r[1] - r[0], r[2], 8) for r in three)


def host_contours(planes, connectivity):
    """MaskContours on host tensors from the host entry: what the device call returns, without a device."""
    from camouflaged_vlm_amd import engine
    res = CO.run(planes, connectivity, host=True)
    total = int(res["vertex_offsets"][-1])
    xy = np.concatenate(res["xy"]).reshape(total, 2)
    return engine.MaskContours(xy=torch.from_numpy(xy), ring_start=torch.from_numpy(np.concatenate(res["ring_start"])),
                               vertex_offsets=torch.from_numpy(res["vertex_offsets"]), n_vertices=torch.from_numpy(res["n_vertices"].astype(np.int32)),
                               n_rings=torch.from_numpy(res["n_rings"]), sizes=[p.shape for p in planes], connectivity=connectivity,
                               status=torch.zeros(1, dtype=torch.int32))


@pytest.mark.parametrize("connectivity", [4, 8])
def test_to_coco_feeds_polygons_request(connectivity):
    from camouflaged_vlm_amd import engine
    rng = np.random.default_rng(2602)
    planes = [rng.random(s) < 0.6 for s in CO.RAGGED]
    for m in planes:
        m[0, 0] = True                                                # polygons_request takes no plane without a polygon
    mc = host_contours(planes, connectivity)
    mc.check()
    coco = mc.to_coco()
    assert [d["size"] for d in coco] == [list(s) for s in CO.RAGGED]
    xy, poly_offsets, plane_polys, sizes = engine.polygons_request(coco)                 # accepts its own output
    assert sizes == [tuple(s) for s in CO.RAGGED] and plane_polys.tolist() == np.concatenate([[0], np.cumsum(mc.n_rings.sum(1).numpy())]).tolist()
    for d, m in zip(coco, planes):
        h, w = d["size"]
        assert np.array_equal(xor_of_rings([np.asarray(p).reshape(-1, 2) for p in d["polygons"]], h, w), m)
    rings = mc.rings()
    assert rings.dtype == torch.int64 and rings[0] == 0 and rings[-1] == mc.xy.shape[0] and rings.numel() == int(mc.n_rings.sum()) + 1
    areas = mc.signed_areas()
    outer = mc.to_coco(holes=False)
    for p, m in enumerate(planes):
        assert areas[p].sum() == m.sum()
        assert (int((areas[p] > 0).sum()), int((areas[p] < 0).sum())) == tuple(mc.n_rings[p].tolist())
        assert len(outer[p]["polygons"]) == int(mc.n_rings[p, 0])
        assert all(CO.signed_area(np.asarray(q).reshape(-1, 2)) > 0 for q in outer[p]["polygons"])
    refused = engine.MaskContours(**{**mc.__dict__, "status": torch.ones(1, dtype=torch.int32)})
    with pytest.raises(RuntimeError, match="mask_contours_sized"):
        refused.check()
    with pytest.raises(RuntimeError, match="mask_contours_sized"):
        refused.to_coco()
