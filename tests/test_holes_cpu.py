"""CPU: holes of packed masks -- the scipy oracle (tests/holes_oracle.py) against a plain flood fill of the complement
from the border and against scipy.ndimage.binary_fill_holes, cvlm_debug_mask_holes_host (the kernels' per-thread functions run
sequentially on the CPU) against the oracle on every operator case and on the reference's own planes and their complements
(tests/golden/demo_classes_digest.npz), the refusals of the entries (no GPU needed: they refuse before launching) and the host check
of the engine's arguments (engine.holes_request)."""
import dataclasses
import os
from collections import deque

import numpy as np
import pytest
import torch
from scipy import ndimage

from camouflaged_vlm_amd import hip, spec
from camouflaged_vlm_amd.engine import ClassHypotheses, holes_request
import compact_oracle as XO
import holes_oracle as HO


def host_holes(bits: np.ndarray, H: int, W: int, connectivity: int, M: int, fill_below: int) -> dict:
    """cvlm_debug_mask_holes_host into sentinel-filled outputs -> the oracle's dict."""
    P = bits.shape[0]
    b = torch.from_numpy(np.ascontiguousarray(bits))
    out = dict(n_holes=torch.full((P,), -7, dtype=torch.int32))
    if M:
        out["holes"] = torch.full((P, M, 6), -7, dtype=torch.int32)
    if fill_below:
        out.update(n_filled=torch.full((P,), -7, dtype=torch.int32), filled_bits=torch.full_like(b, 0xa5),
                   filled_area=torch.full((P,), -7, dtype=torch.int32))
    hip.mask_holes_host(b, H, W, connectivity, fill_below, **out)
    return {k: v.numpy() for k, v in out.items()}


def assert_equal(got: dict, want: dict, what) -> None:
    assert set(got) <= set(want), what
    for k, v in got.items():
        assert v.dtype == want[k].dtype and np.array_equal(v, want[k]), (what, k)


def flood_holes(plane: np.ndarray, connectivity: int):
    """The plainest definition there is: flood the clear pixels from the border at the dual connectivity; what stays dry is holes,
    taken apart by a raster scan with a breadth-first fill -> (rows (area, x0, y0, x1, y1, seed) sorted by (-area, seed), dry bool)."""
    H, W = plane.shape
    steps = [(0, 1), (0, -1), (1, 0), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if connectivity == 4 else [])

    def fill(start, seen):
        todo, px = deque(start), []
        while todo:
            cy, cx = todo.popleft()
            px.append((cy, cx))
            for dy, dx in steps:
                ny, nx = cy + dy, cx + dx
                if 0 <= ny < H and 0 <= nx < W and not plane[ny, nx] and not seen[ny, nx]:
                    seen[ny, nx] = True
                    todo.append((ny, nx))
        return px
    wet = np.zeros_like(plane)
    border = [(y, x) for y in range(H) for x in range(W) if (y in (0, H - 1) or x in (0, W - 1)) and not plane[y, x]]
    for y, x in border:
        wet[y, x] = True
    fill(border, wet)
    dry = ~plane & ~wet
    seen, rows = wet.copy(), []
    for y in range(H):
        for x in range(W):
            if plane[y, x] or seen[y, x]:
                continue
            seen[y, x] = True
            px = fill([(y, x)], seen)
            ys, xs = [p[0] for p in px], [p[1] for p in px]
            rows.append((len(px), min(xs), min(ys), max(xs), max(ys), y * W + x))
    return sorted(rows, key=lambda r: (-r[0], r[5])), dry


def test_oracle_equals_flood_fill_and_binary_fill_holes():
    rng = np.random.default_rng(5)
    planes = [rng.random((8, 32)) < d for d in (0.3, 0.4, 0.5, 0.55, 0.6, 0.7, 0.8, 0.9, 0.95)]
    planes += [np.zeros((8, 32), bool), np.ones((8, 32), bool), HO.operator_cases()["rings"][1]]
    assert len(planes) == 12
    total = 0
    for plane in planes:
        for conn in (4, 8):
            want, dry = flood_holes(plane, conn)
            total += len(want)
            _, _, rows = HO.hole_regions(plane, conn)
            assert rows.tolist() == [list(r) for r in want]
            got = HO.holes(HO.pack(plane[None]), 8, 32, conn, M=3, fill_below=2)
            assert got["n_holes"][0] == len(want) and got["n_filled"][0] == sum(r[0] < 2 for r in want)
            assert got["holes"][0].tolist() == [list(r) for r in want[:3]] + [list(HO.FILLER)] * max(0, 3 - len(want))
            every = HO.holes(HO.pack(plane[None]), 8, 32, conn, M=1, fill_below=8 * 32)        # fill_below >= H * W: every hole
            assert np.array_equal(XO.unpack(every["filled_bits"], 8, 32)[0], plane | dry)
            structure = ndimage.generate_binary_structure(2, 1 if conn == 8 else 2)
            assert np.array_equal(plane | dry, ndimage.binary_fill_holes(plane, structure=structure))
            if conn == 8:
                assert np.array_equal(plane | dry, ndimage.binary_fill_holes(plane))            # its default structure
    assert total > 50


def _fill_belows(bits, H, W, conn):
    largest = int(HO.holes(bits, H, W, conn, 1, 0)["holes"][:, 0, 0].max())
    return (0, 1, 3, largest + 1)                                                 # the last: one above the largest hole


@pytest.mark.parametrize("name", sorted(HO.operator_cases()))
def test_host_entry_equals_oracle_on_operator_cases(name):
    planes = HO.operator_cases()[name]
    P, H, W = planes.shape
    bits = HO.pack(planes)
    for conn in (4, 8):
        for M in (1, 5):
            for fill_below in _fill_belows(bits, H, W, conn):
                assert_equal(host_holes(bits, H, W, conn, M, fill_below), HO.holes(bits, H, W, conn, M, fill_below),
                             (name, conn, M, fill_below))
        assert_equal(host_holes(bits, H, W, conn, 1, H * W), HO.holes(bits, H, W, conn, 1, H * W), (name, conn, "every hole"))
    got = host_holes(bits, H, W, 8, 0, 0)                                         # no table, nothing filled: the count alone
    assert list(got) == ["n_holes"] and np.array_equal(got["n_holes"], HO.holes(bits, H, W, 8, 1, 0)["n_holes"])


def test_operator_cases_are_what_they_claim():
    c = HO.operator_cases()
    full = lambda name, conn, M=1: HO.holes(HO.pack(c[name]), *c[name].shape[1:], conn, M, 0)
    n = lambda name, conn: full(name, conn)["n_holes"].tolist()
    top = lambda name, conn: full(name, conn)["holes"][:, 0, 0].tolist()
    assert n("one_word", 8) == n("one_word", 4) == [0, 0, 0]
    # ring, ring less a corner, rings against the border (twice), checkerboard, frame, closed ring touching the border
    assert n("rings", 8) == [1, 1, 0, 0, 90, 1, 1] and top("rings", 8) == [6, 6, 0, 0, 1, 180, 6]
    assert n("rings", 4) == [1, 0, 0, 0, 0, 1, 1] and top("rings", 4) == [6, 0, 0, 0, 0, 180, 6]
    assert n("pinhole", 8) == n("pinhole", 4) == [1, 0] and top("pinhole", 8) == [1, 0]
    assert n("seam", 8) == n("seam", 4) == [1] and top("seam", 8) == [3 * 7]
    assert n("whole_word", 8) == [1] and top("whole_word", 8) == [4 * 58]
    assert n("u_and_nested", 8) == n("u_and_nested", 4) == [1, 2]
    assert top("u_and_nested", 8) == [27 + 27 + 26 - 2, 26 * 26 - 12 * 12]
    nested = full("u_and_nested", 8, 2)["holes"][1]
    assert nested[1].tolist() == [10 * 10 - 4 * 4, 9, 9, 18, 18, 9 * 32 + 9]
    two = full("squares_three", 8, 2)["holes"][0]
    assert two[0].tolist() == [25, 4, 3, 8, 7, 3 * 64 + 4] and two[1].tolist() == [25, 50, 40, 54, 44, 40 * 64 + 50]
    assert n("squares_three", 8) == [2, 3] and full("squares_three", 8, 5)["holes"][1, 3:].tolist() == [list(HO.FILLER)] * 2
    assert n("plane_ends", 8) == n("plane_ends", 4) == [1, 0]
    counts = {conn: n("random", conn) for conn in (4, 8)}
    print("random 64 x 96 planes at densities 0.5 / 0.7 / 0.9: holes", counts)
    assert counts == {8: [378, 767, 461], 4: [21, 246, 375]}
    assert all(a > b for a, b in zip(counts[8], counts[4]))                       # a 4-connected background falls apart into more holes


def test_fill_below_one_reproduces_the_plane():
    planes = HO.operator_cases()["random"]
    P, H, W = planes.shape
    bits = HO.pack(planes)
    for conn in (4, 8):
        got = host_holes(bits, H, W, conn, 1, 1)
        assert np.array_equal(got["filled_bits"], bits) and np.array_equal(got["filled_area"], XO.stats(planes)[0])
        assert (got["n_filled"] == 0).all() and (got["n_holes"] > 0).all()


@pytest.fixture(scope="module")
def ref_bits(golden_dir):
    with np.load(os.path.join(golden_dir, "demo_classes_digest.npz")) as z:
        bits = z["mask_bits"]
    return np.ascontiguousarray(bits.reshape(-1, bits.shape[-1]))


def test_host_entry_equals_oracle_on_the_reference_planes_and_their_complements(ref_bits):
    """Also the figures that show the fixture is not degenerate for holes: a handful of small holes in each plane, thousands in each
    complement, most of them below 64 pixels, a unique largest one, and binary_fill_holes adds exactly the sum of the hole areas."""
    S = spec.DEMO_SAM.inp_size
    assert ref_bits.shape == (6, S * S // 8)
    both = np.concatenate([ref_bits, ~ref_bits])
    dense = XO.stats(XO.unpack(both[6:], S, S))[0] / (S * S)
    assert 0.80 <= dense.min() and dense.max() < 0.855                             # 80 to 85 % set
    for conn in (4, 8):
        want = HO.holes(both, S, S, conn, 5, 64)
        assert_equal(host_holes(both, S, S, conn, 5, 64), want, conn)
        big = int(want["holes"][:, 0, 0].max()) + 1
        assert_equal(host_holes(both, S, S, conn, 1, big), HO.holes(both, S, S, conn, 1, big), (conn, "one above the largest hole"))
        n, top = want["n_holes"], want["holes"][:, 0, 0]
        print(f"reference planes and complements, connectivity {conn}: n_holes {n.tolist()} largest {top.tolist()} "
              f"below 64 {want['n_filled'].tolist()}")
        assert n[:6].tolist() == ([6, 15, 11, 5, 14, 7] if conn == 8 else [5, 7, 9, 2, 4, 4])
        lo, hi = (8493, 9416) if conn == 8 else (8189, 9185)
        assert lo == n[6:].min() and n[6:].max() == hi
        assert (want["holes"][6:, 0, 0] > want["holes"][6:, 1, 0]).all()                  # a unique largest hole in every complement
        lo, hi = (225, 395) if conn == 8 else (236, 505)
        assert lo == top[6:].min() and top[6:].max() == hi
        if conn == 8:
            assert 12 == top[:6].min() and top[:6].max() == 48
            assert 7659 == want["n_filled"][6:].min() and want["n_filled"][6:].max() == 9055
        # binary_fill_holes adds exactly the sum of the hole areas
        every = HO.holes(both, S, S, conn, 1, S * S)
        structure = ndimage.generate_binary_structure(2, 1 if conn == 8 else 2)
        planes = XO.unpack(both, S, S)
        for p in range(12):
            filled = ndimage.binary_fill_holes(planes[p], structure=structure)
            assert np.array_equal(XO.unpack(every["filled_bits"][p:p + 1], S, S)[0], filled)
            lab, is_hole, rows = HO.hole_regions(planes[p], conn)
            assert int(filled.sum()) - int(planes[p].sum()) == int(rows[:, 0].sum()) == every["filled_area"][p] - int(planes[p].sum())


# ---- the entries refuse before they touch anything --------------------------------------------------------------------------------------
def test_mask_holes_refuses_bad_arguments_without_gpu():
    lib = hip.load()
    p = 4096
    ok = dict(bits=p, P=2, H=4, W=64, conn=8, M=3, fill_below=2, ws=p, ws_bytes=14 * 4 * 64, n_holes=p, holes=p, n_filled=p, filled_bits=p,
              filled_area=p)
    bad = [dict(bits=None), dict(n_holes=None), dict(bits=p + 2), dict(filled_bits=p + 2), dict(P=0), dict(P=-1), dict(P=65536), dict(H=0),
           dict(H=-4), dict(W=0), dict(W=-64), dict(W=48), dict(W=8), dict(H=2 ** 16, W=2 ** 15), dict(H=2 ** 20, W=2 ** 20),
           dict(conn=6), dict(conn=0), dict(conn=-8), dict(M=-1), dict(M=65), dict(M=0), dict(holes=None), dict(fill_below=-1),
           dict(fill_below=0), dict(n_filled=None), dict(filled_bits=None), dict(filled_area=None)]

    def device(**kw):
        a = dict(ok, **kw)
        return lib.cvlm_mask_holes(a["bits"], a["P"], a["H"], a["W"], a["conn"], a["M"], a["fill_below"], a["ws"], a["ws_bytes"],
                                   a["n_holes"], a["holes"], a["n_filled"], a["filled_bits"], a["filled_area"], None)

    def host(**kw):
        a = dict(ok, **kw)
        return lib.cvlm_debug_mask_holes_host(a["bits"], a["P"], a["H"], a["W"], a["conn"], a["M"], a["fill_below"], a["n_holes"],
                                              a["holes"], a["n_filled"], a["filled_bits"], a["filled_area"])
    for kw in bad:
        assert device(**kw) == -1, kw
        assert host(**kw) == -1, kw
    for kw in (dict(ws=None), dict(ws=p + 8), dict(ws_bytes=14 * 4 * 64 - 1), dict(ws_bytes=0), dict(ws_bytes=-1)):
        assert device(**kw) == -1, kw
    assert device(M=0, holes=None, fill_below=0, n_filled=None, filled_bits=None, filled_area=None, ws=None) == -1
    size = lib.cvlm_mask_holes_workspace_bytes
    assert size(1, 4, 64) == 14 * 4 * 64 and size(7, 32, 64) == 7 * 14 * 32 * 64 and size(65535, 1024, 1024) == 65535 * 14 * 2 ** 20
    for P, H, W in ((0, 4, 64), (65536, 4, 64), (1, 0, 64), (1, 4, 0), (1, 4, 48), (1, -4, 64), (1, 2 ** 16, 2 ** 15)):
        assert size(P, H, W) == -1, (P, H, W)
    with pytest.raises(RuntimeError):
        hip.mask_holes_workspace_bytes(1, 4, 48)


# ---- the host request -----------------------------------------------------------------------------------------------------------------------
def test_holes_request_accepts_and_refuses():
    assert holes_request(masks="logits") == (False, 0, 0, 8)                      # the default: nothing asked for
    assert holes_request(masks="bits") == (False, 0, 0, 8)
    assert holes_request(holes=4, fill_holes=16, masks="bits") == (True, 4, 16, 8)
    assert holes_request(holes=0, masks="both", connectivity=4) == (True, 0, 0, 4)
    assert holes_request(holes=64, masks="bits", side=1024) == (True, 64, 0, 8)
    assert holes_request(fill_holes=1, masks="bits") == (True, 0, 1, 8)
    assert holes_request(holes=np.int64(3), fill_holes=np.int32(2), masks="both") == (True, 3, 2, 8)
    assert holes_request(masks="bits", side=48) == (False, 0, 0, 8)               # nothing asked for: any width
    bad = [dict(holes=-1), dict(holes=65), dict(holes=1.0), dict(holes="1"), dict(holes=True),
           dict(fill_holes=-1), dict(fill_holes=1.5), dict(fill_holes=None), dict(fill_holes=True), dict(fill_holes=2 ** 31),
           dict(holes=1, masks="logits"), dict(fill_holes=1, masks="logits"), dict(holes=0, masks="logits"),
           dict(holes=1, side=48), dict(fill_holes=4, side=1000),
           dict(holes=1, connectivity=6), dict(connectivity=6), dict(connectivity="8"), dict(connectivity=True), dict(connectivity=None)]
    for kw in bad:
        with pytest.raises(ValueError):
            holes_request(**dict(dict(masks="bits"), **kw))
    with pytest.raises(ValueError, match="infer_classes"):
        holes_request(holes=99, masks="bits", who="infer_classes")


def test_class_hypotheses_hole_fields_are_optional():
    t = torch.zeros(1)
    h = ClassHypotheses(classes=t, pass1_logits=t, masks=t, edges=t, logits=t, pred=t)
    names = ("n_holes", "holes", "n_filled", "filled_bits", "filled_area")
    assert all(getattr(h, n) is None for n in names)
    assert [f.name for f in dataclasses.fields(h)] == ["classes", "pass1_logits", "masks", "edges", "logits", "pred"]
    h = ClassHypotheses(classes=t, pass1_logits=t, masks=None, edges=None, logits=t, pred=t, mask_bits=t, **{n: t for n in names})
    assert all(getattr(h, n) is t for n in names) and h.n_comp is None and h.kept_bits is None
