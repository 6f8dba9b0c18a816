"""COCO polygon annotations on the device without a GPU: the oracle (tests/poly_oracle.py) against the known answers
and against the published sort / difference / merge loop; cvlm_debug_mask_poly_decode_host -- the kernels' per-thread functions
(csrc/poly_logic.h, csrc/gt_logic.h) run sequentially -- against the oracle on every shape, polygon kind, random family, union and
refusal of the GPU tests; the search for edges on which a fused multiply-add would change the walk; the pure host check
`polygons_request`; `SizedMasks.concat`; every CVLM_E_BADARG of the new entries; the exports.  Everything is integers, compared exactly."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import gt_oracle as GO
import poly_oracle as PO
import rle_oracle as RO
import sized_oracle as SO
from camouflaged_vlm_amd import engine, hip, maskpost, rle
from camouflaged_vlm_amd.engine import SizedMasks, polygons_request

HOST = hip.mask_poly_decode_host


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------------
def test_the_oracle_gives_the_known_answers():
    for xy, h, w, rows in PO.KNOWN:
        want = PO.known_plane(rows, h, w)
        assert np.array_equal(PO.plane_of(xy, h, w), want), xy
        assert np.array_equal(rle.decode(PO.counts_literal(xy, h, w), h, w), want), xy
    assert [int(PO.plane_of(k[0], k[1], k[2]).sum()) for k in PO.KNOWN] == [9, 9, 10, 14, 20, 0]


def test_the_oracle_equals_the_published_counts_loop():
    """Pixel j is set iff an odd number of candidates lie at or before it == sort, difference, merge across zero counts, decode."""
    n = 0
    for fam in ("uniform", "tenths", "ints"):
        for polys, h, w in PO.random_family(fam, 400, seed=3):
            c = PO.counts_literal(polys[0], h, w)
            assert sum(c) == h * w and all(v > 0 for v in c[1:])
            assert np.array_equal(rle.decode(c, h, w), PO.plane_of(polys[0], h, w))
            n += 1
    for h, w in PO.SHAPES:
        for name, xy in PO.kinds(h, w).items():
            assert np.array_equal(rle.decode(PO.counts_literal(xy, h, w), h, w), PO.plane_of(xy, h, w)), (h, w, name)
    assert n == 1200


def test_the_result_does_not_depend_on_the_orientation():
    for h, w in PO.SHAPES:
        a, b = PO.orientation_pairs(h, w)
        assert np.array_equal(PO.plane_of(a, h, w), PO.plane_of(b, h, w))
        k = PO.kinds(h, w)
        assert not PO.plane_of(k["all_equal"], h, w).any() and PO.plane_of(k["covers"], h, w).all()
        for side in ("left", "right", "above", "below"):
            assert not PO.plane_of(k["outside_" + side], h, w).any(), side


# ---- the host entry --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", PO.SHAPES)
def test_host_entry_equals_the_oracle_on_every_kind(h, w):
    """The 1500-vertex circle has more edges than one pass of the kernel's edge loop takes."""
    items = [([xy], h, w) for xy in PO.kinds(h, w).values()]
    got = PO.check_items(HOST, items)
    bare, a, _, status = PO.run_poly(HOST, items, stats=False)
    assert status == 0 and a is None and all(np.array_equal(x, y) for x, y in zip(bare, got))
    PO.check_items(HOST, items, guard=GO.GUARD + 4)


@pytest.mark.parametrize("family", ["uniform", "tenths", "ints"])
def test_host_entry_equals_the_oracle_on_random_polygons(family):
    PO.check_items(HOST, PO.random_family(family, 3000, seed=5))


def test_host_entry_known_answers_and_unions():
    items = [([list(map(float, xy))], h, w) for xy, h, w, _ in PO.KNOWN]
    PO.check_items(HOST, items, want=[PO.known_plane(rows, h, w) for _, h, w, rows in PO.KNOWN])
    items = PO.union_items()
    assert sorted({len(ps) for ps, _, _ in items}) == [1, 2, 3, 17]
    got = PO.check_items(HOST, items)
    polys, h, w = items[3]                                            # one polygon inside another: union and XOR differ
    assert (PO.plane_of(polys[0], h, w) & PO.plane_of(polys[1], h, w)).sum() > 0
    assert np.array_equal(got[3], SO.pack_rows(PO.plane_of(polys[0], h, w)))
    assert got[7].any()                                               # the same polygon twice stays set


def contraction_edges(n_try: int = 6000, want: int = 6):
    """Edges (xs, ys, xe, ye) of scaled integers, |c| <= 2000, with a step t where a fused ys + s * t -- one rounding of the exact sum,
    in rationals -- truncates differently from the product and the sum rounded one after the other: dx even, t = dx / 2, dy odd, so
    that the real minor coordinate is a tie k + 0.5 and the slope's rounding error decides.  -> [(edge, t, v of two roundings, v fused)]."""
    rng = np.random.default_rng(11)
    out = []
    for _ in range(n_try):
        dx = 2 * int(rng.integers(1, 1000))
        dy = 2 * int(rng.integers(0, dx // 2)) + 1 if dx > 2 else 1
        if dy >= dx:
            continue
        t = dx // 2
        ys = 2 - (dy - 1) // 2                                        # ys + dy / 2 = 2.5: v is 3 or 2, which changes ceil((v - 2) / 5)
        s = float(dy) / float(dx)
        two = int((float(ys) + s * float(t)) + 0.5)
        fused = int(float(Fraction(ys) + Fraction(s) * t) + 0.5)
        if two != fused:
            xs = 7 - t                                                # t + xs = 7: the pair behind the step lies on pixel column 1
            out.append(((xs, ys, xs + dx, ys + dy), t, two, fused))
            if len(out) == want:
                break
    return out


def unscale(c: int) -> float:
    """A coordinate whose scaled integer is c."""
    return c / 5.0 if c >= 0 else (c - 0.75) / 5.0


def contraction_items():
    """One triangle per found edge on a plane of 8 x 8: the edge, then a vertex above its start."""
    items = []
    for (xs, ys, xe, ye), _, _, _ in contraction_edges():
        xy = [unscale(xs), unscale(ys), unscale(xe), unscale(ye), unscale(xs), unscale(ye + 40)]
        X, Y = PO.scaled(xy)
        assert X.tolist() == [xs, xe, xs, xs] and Y.tolist() == [ys, ye, ye + 40, ys]
        items.append(([xy], 8, 8))
    return items


def test_a_fused_multiply_add_would_change_the_walk():
    """The search space holds such edges; on them the definition (two roundings) and a fused evaluation give different planes, and
    the host entry gives the definition's."""
    found = contraction_edges()
    assert len(found) == 6 and all(abs(c) <= 2000 for e, _, _, _ in found for c in e)
    assert all((two, fused) == (3, 2) for _, _, two, fused in found)
    items = contraction_items()
    for (polys, h, w), (_, t, two, fused) in zip(items, found):
        u, v = PO.walk(polys[0])
        assert u[t] == 7 and u[t + 1] == 8 and v[t] == two            # the pair behind the step lies on pixel column 1
        other = v.copy()
        other[t] = fused
        assert not PO.plane_of(polys[0], h, w)[0, 1] and PO.plane_of(polys[0], h, w, uv=(u, other))[0, 1]
    PO.check_items(HOST, items)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
TRI = [0.5, 0.5, 20.5, 3.0, 7.0, 25.5]
SQUARE = [1.0, 1.0, 4.0, 1.0, 4.0, 4.0, 1.0, 4.0]


def refusal_cases():
    """name -> (items, overrides of run_poly, planes that must come out refused, planes whose slice is not stored).  Every good plane
    holds the same triangle, so that a table which hands a plane another plane's polygon changes nothing of what it must show."""
    sizes = [(1, 32), (5, 4), (33, 31), (32, 63)]
    good = [([TRI], h, w) for h, w in sizes]
    W = GO.WORD_GUARD
    po = np.arange(5, dtype=np.int64) * 6 + W
    total = int(po[-1]) + W
    out = {}

    def swap(p, polys):
        items = list(good)
        items[p] = (polys, good[p][1], good[p][2])
        return items
    out["nan"] = (swap(1, [[0.5, 0.5, float("nan"), 3.0, 7.0, 25.5]]), {}, [1], [])
    out["inf"] = (swap(1, [[0.5, 0.5, 20.5, float("-inf"), 7.0, 25.5]]), {}, [1], [])
    out["beyond_the_bound"] = (swap(2, [[0.5, 0.5, 65536.5, 3.0, 7.0, 25.5]]), {}, [2], [])
    out["below_the_bound"] = (swap(2, [[0.5, -65537.0, 20.5, 3.0, 7.0, 25.5]]), {}, [2], [])
    out["two_vertices"] = (swap(1, [[0.5, 0.5, 20.5, 3.0]]), {}, [1], [])
    out["odd_length"] = (swap(1, [TRI + [1.0]]), {}, [1], [])
    out["too_many_vertices"] = (swap(0, [[1.0, 2.0] * 65536]), {}, [0], [])
    out["over_the_point_cap"] = (swap(3, [[65536.0, -65536.0, -65536.0, 65536.0] * 1500]), {}, [3], [])
    out["second_polygon_bad"] = (swap(1, [TRI, [0.5, 0.5, float("nan"), 3.0, 7.0, 25.5], SQUARE]), {}, [1], [])
    out["last_polygon_short"] = (swap(2, [TRI, SQUARE, [1.0, 1.0, 2.0, 2.0]]), {}, [2], [])
    out["empty_plane_entry"] = (good, dict(plane_polys=[0, 1, 1, 2, 3]), [1], [])
    out["two_listed_where_every_plane_has_one"] = (good, dict(plane_polys=[0, 2, 2, 3, 4]), [0, 1], [])
    out["list_runs_backwards"] = (good, dict(plane_polys=[0, 1, 0, 3, 4]), [1, 2], [])
    out["list_beyond_Q"] = (good, dict(plane_polys=[0, 1, 2, 3, 5]), [3], [])
    out["list_below_zero"] = (good, dict(plane_polys=[-1, 1, 2, 3, 4]), [0], [])
    out["list_of_4097"] = (swap(1, [SQUARE] * 4097), {}, [1], [])
    back = po.copy()
    back[2] = back[1] - 5                                             # polygon 1 runs backwards, polygon 2 holds 17 doubles
    out["offsets_backwards"] = (good, dict(poly_offsets=back), [1, 2], [])
    below = po.copy()
    below[0] = -6
    out["offsets_below_zero"] = (good, dict(poly_offsets=below), [0], [])
    beyond = po.copy()
    beyond[-1] = total + 2
    out["offsets_beyond_total"] = (good, dict(poly_offsets=beyond), [3], [])
    out["total_cuts_the_last"] = (good, dict(total=int(po[-1]) - 1), [3], [])
    out["max_pixels_too_small"] = (good, dict(max_pixels=33 * 31 - 1), [2, 3], [])
    _, off, nb, _ = SO.tables(sizes)
    bad = off.copy()
    bad[2:] += 4
    out["table_slice_too_long"] = (good, dict(bit_offsets=bad), [1], [1])
    out["table_end_beyond"] = (good, dict(nbytes=int(off[-1]) - 4), [3], [3])
    for first in (-4, GO.GUARD + 2):
        bad = off.copy()
        bad[0] = first
        out[f"table_start_{first}"] = (good, dict(bit_offsets=bad), [0], [0])
    for size in ((0, 32), (1, -2), (1, 16385), (2 ** 31 - 1, 2 ** 31 - 1)):
        dims = [list(size)] + [[h, w] for _, h, w in good[1:]]
        out[f"size_{size}"] = (good, dict(dims=dims), [0], [0])
    return out


def check_refusal(entry, name, dev="cpu"):
    """status 1, the refused plane zero -- or untouched where its table is at fault --, area 0, box -1, its neighbours whole and every
    band untouched (PO.run_poly)."""
    items, over, refused, unstored = refusal_cases()[name]
    got, area, box, status = PO.run_poly(entry, items, dev=dev, **over)
    assert status == 1
    for p, (polys, h, w) in enumerate(items):
        if p in unstored:
            assert got[p] is None and area[p] == 0 and box[p].tolist() == [-1] * 4
        elif p in refused:
            GO.check_plane(got[p], area[p], box[p], None, h, w)
        else:
            GO.check_plane(got[p], area[p], box[p], PO.expected([TRI], h, w), h, w)
    return got, area, box


@pytest.mark.parametrize("name", list(refusal_cases()))
def test_host_entry_refuses_whole_planes(name):
    check_refusal(HOST, name)


def bound_items():
    """Inside the bounds, with answers that need no walk in Python: 24 edges of 655 361 points each, back and forth along y = 0 -- every
    boundary toggled an even number of times --; 65535 equal vertices; a rectangle with |c| = 65536 exactly, which covers the plane."""
    return [([[65536.0, 0.0, -65536.0, 0.0] * 12], 3, 5), ([[1.0, 2.0] * 65535], 3, 5),
            ([[65536.0, 65536.0, -65536.0, 65536.0, -65536.0, -65536.0, 65536.0, -65536.0]], 3, 5)], [False, False, True]


def test_the_bounds_themselves_are_taken():
    items, full = bound_items()
    assert all(PO.polygon_ok(ps[0]) for ps, _, _ in items) and not PO.polygon_ok([65536.0, 0.0, -65536.0, 0.0] * 13)
    PO.check_items(HOST, items, want=[np.full((h, w), f) for (_, h, w), f in zip(items, full)])


def test_host_entry_replays_into_used_outputs():
    """Every output is initialised by the call: a second call into the same tensors, and one after a call that refused a plane, gives
    the same bytes."""
    items = PO.union_items()
    sizes = [(h, w) for _, h, w in items]
    d, off, _, _ = SO.tables(sizes, 0)
    flat, po, pp = PO.tables(items, W=0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    P, mp = len(items), max(h * w for h, w in sizes)
    bits = torch.empty(int(off[-1]), dtype=torch.uint8)
    area, box, status = (torch.empty(s, dtype=torch.int32) for s in ((P,), (P, 4), (1,)))
    bad = flat.copy()
    bad[int(po[1])] = np.nan                                          # the second polygon of plane 0
    seen = []
    for xy in (flat, flat, bad, flat):
        HOST(t(xy), t(po), t(pp), t(d), t(off), mp, bits, area, box, status)
        seen.append((bits.numpy().copy(), area.tolist(), box.tolist(), status.item()))
    assert [s[3] for s in seen] == [0, 0, 1, 0] and seen[2][1][0] == 0 and seen[0][1][0] > 0
    for s in (seen[1], seen[3]):
        assert np.array_equal(s[0], seen[0][0]) and s[1:] == seen[0][1:]


# ---- the pure host checks ----------------------------------------------------------------------------------------------------------------------
def test_polygons_request_accepts_and_refuses():
    xy, po, pp, sizes = polygons_request([{"size": [8, 33], "polygons": [TRI, SQUARE]}, {"size": (np.int64(5), 4), "polygons": [np.asarray(TRI)]},
                                          {"size": [1, 1], "polygons": ([1, 1, 4, 1, 4, 4],)}])
    assert xy.dtype == np.float64 and po.dtype == np.int64 and pp.dtype == np.int32 and sizes == [(8, 33), (5, 4), (1, 1)]
    assert po.tolist() == [0, 6, 14, 20, 26] and pp.tolist() == [0, 2, 3, 4] and xy.tolist() == TRI + SQUARE + TRI + [1, 1, 4, 1, 4, 4]
    edge = {"size": [3, 3], "polygons": [[65536.0, 65536.0, -65536.0, -65536.0, -65536.0, 65536.0], [1.0, 2.0] * 65535]}
    assert polygons_request([edge])[1].tolist() == [0, 6, 6 + 2 * 65535]
    ok = {"size": [2, 3], "polygons": [TRI]}
    one = lambda **kw: [dict(ok, **kw)]
    bad = [None, 7, "abc", {}, ok, [], [ok, 5], [{"size": [2, 3]}], [{"polygons": [TRI]}], one(size=[2]), one(size="23"), one(size=[2.0, 3]),
           one(size=[True, 3]), one(size=[0, 3]), one(size=[2, 16385]), one(polygons=[]), one(polygons=TRI), one(polygons="abc"), one(polygons=None),
           one(polygons=[TRI] * 4097), one(polygons=[[1.0, 2.0, 3.0, 4.0]]), one(polygons=[TRI + [1.0]]), one(polygons=[[]]),
           one(polygons=[[1.0, 2.0] * 65536]), one(polygons=[[0.5, float("nan"), 1, 1, 2, 2]]), one(polygons=[[0.5, float("inf"), 1, 1, 2, 2]]),
           one(polygons=[[0.5, 65536.5, 1, 1, 2, 2]]), one(polygons=[[0.5, -65537, 1, 1, 2, 2]]), one(polygons=[["1", "2", "3", "4", "5", "6"]]),
           one(polygons=[[True, 1, 2, 2, 3, 3]]), one(polygons=[[[1, 1], [2, 2], [3, 3]]]), one(polygons=[[1 + 0j, 1, 2, 2, 3, 3]]),
           one(polygons=["123456"]), one(polygons=[TRI, 5]), one(polygons=[TRI, [1.0, None, 2, 2, 3, 3]]),
           one(polygons=[[65536.0, -65536.0, -65536.0, 65536.0] * 1500])]
    for r in bad:
        with pytest.raises(ValueError):
            polygons_request(r)
    with pytest.raises(ValueError, match="SAM.polygons_decode"):
        polygons_request(None, who="SAM.polygons_decode")
    assert engine.polygons_request is maskpost.polygons_request and engine.Cascade.polygons_decode is maskpost.MaskUtilities.polygons_decode


def host_sized(anns=None, rles=None, stats=True) -> SizedMasks:
    """A SizedMasks in host memory through the host entries: what polygons_decode / rle_decode give on the device."""
    if anns is not None:
        xy, po, pp, sizes = polygons_request(anns)
    else:
        c, o, sizes = engine.rle_decode_request(rles)
    P = len(sizes)
    dims, offsets, _ = engine.sized_tables(sizes)
    t = torch.from_numpy
    out = SizedMasks(bits=torch.empty(int(offsets[P]), dtype=torch.uint8), offsets=t(offsets), area=torch.empty(P, dtype=torch.int32) if stats else None,
                     box=torch.empty(P, 4, dtype=torch.int32) if stats else None, status=torch.empty(1, dtype=torch.int32), sizes=sizes, level=0)
    mp = max(h * w for h, w in sizes)
    if anns is not None:
        HOST(t(xy), t(po), t(pp), t(dims), out.offsets, mp, out.bits, out.area, out.box, out.status)
    else:
        hip.mask_rle_decode_host(t(c), t(o), t(dims), out.offsets, mp, out.bits, out.area, out.box, out.status)
    return out


def concat_parts():
    anns = [{"size": [h, w], "polygons": ps} for ps, h, w in PO.union_items()]
    m = GO.planes(33, 31)["random_0.5"]
    rles = [{"size": [33, 31], "counts": RO.plane_counts(m).tolist()}, {"size": [8, 33], "counts": RO.plane_counts(GO.planes(8, 33)["checker"]).tolist()}]
    return anns, rles, [m, GO.planes(8, 33)["checker"]]


def check_concat(joined, parts, whole):
    """`joined` = concat(parts) holds the parts' planes in order; `whole` decoded the joined list in one call: the same tensors."""
    assert joined.sizes == [s for p in parts for s in p.sizes] and joined.level == 0 and joined.status.numel() == 1
    assert int(joined.offsets[-1]) == joined.bits.numel() and joined.offsets.dtype == torch.int64
    if whole is not None:
        for f in ("bits", "offsets", "area", "box"):
            assert torch.equal(getattr(joined, f), getattr(whole, f)), f
        assert int(joined.status) == int(whole.status) == 0


def test_concat_equals_decoding_the_joined_list():
    anns, rles, truth = concat_parts()
    a, b, c = host_sized(anns=anns[:4]), host_sized(anns=anns[4:]), host_sized(rles=rles)
    check_concat(SizedMasks.concat([a, b]), [a, b], host_sized(anns=anns))
    mixed = SizedMasks.concat((b, c, a))
    check_concat(mixed, [b, c, a], None)
    for q, m in enumerate(truth):
        assert np.array_equal(mixed.to_numpy(len(b.sizes) + q), m)
    assert np.array_equal(mixed.to_numpy(len(mixed.sizes) - 1), PO.expected(*PO.union_items()[3]))
    assert mixed.area.tolist() == b.area.tolist() + c.area.tolist() + a.area.tolist() and mixed.box.shape == (len(mixed.sizes), 4)
    assert SizedMasks.concat([a]).sizes == a.sizes
    refused = host_sized(anns=anns[:1])
    refused.status[0] = 1
    assert int(SizedMasks.concat([a, refused, b]).status) == 1
    with pytest.raises(RuntimeError, match="polygons_decode"):
        SizedMasks.concat([a, refused]).check()
    bare = host_sized(anns=anns[:2], stats=False)
    assert SizedMasks.concat([bare, bare]).area is None
    thresholded = SizedMasks(bits=a.bits, offsets=a.offsets, area=a.area, box=a.box, status=a.status, sizes=a.sizes, level=128)
    assert SizedMasks.concat([thresholded, thresholded]).level == 128 and SizedMasks.concat([thresholded, a]).level == 0
    for bad in (None, [], a, [a, None], [a, bare], [bare, a], "ab"):
        with pytest.raises(ValueError):
            SizedMasks.concat(bad)


# ---- CVLM_E_BADARG, before the device is touched ------------------------------------------------------------------------------------------------
def test_poly_entries_refuse_bad_arguments_without_gpu():
    lib = hip.load()
    p = 1 << 20
    one = lib.cvlm_mask_poly_decode_workspace_bytes(1, 64)
    assert one == 64 == 2 * lib.cvlm_mask_rle_decode_workspace_bytes(1, 64) and lib.cvlm_mask_poly_decode_workspace_bytes(3, 65) == 3 * 64
    for P, mp in ((0, 64), (65536, 64), (1, 0), (1, 2 ** 28 + 1)):
        assert lib.cvlm_mask_poly_decode_workspace_bytes(P, mp) == -1
    base = dict(xy=p, total=8, po=p + 4096, pp=p + 6144, dims=p + 8192, bo=p + 12288, P=1, Q=1, mp=64, bits=p + 16384, nb=8, area=p + 20480,
                box=p + 24576, status=p + 28672, ws=p + 65536, wsb=one)
    order = ("xy", "total", "po", "pp", "dims", "bo", "P", "Q", "mp", "bits", "nb", "area", "box", "status")
    bad = [dict(xy=None), dict(po=None), dict(pp=None), dict(dims=None), dict(bo=None), dict(bits=None), dict(status=None), dict(area=None),
           dict(box=None), dict(xy=p + 4), dict(pp=p + 6146), dict(dims=p + 8194), dict(bits=p + 16385), dict(area=p + 20482), dict(box=p + 24577),
           dict(status=p + 28674), dict(po=p + 4100), dict(bo=p + 12292), dict(P=0), dict(P=65536), dict(Q=0), dict(Q=-1), dict(Q=4097),
           dict(total=0), dict(nb=3), dict(mp=0), dict(mp=2 ** 28 + 1)]
    for kw in bad:
        k = dict(base, **kw)
        args = [k[n] for n in order]
        assert lib.cvlm_debug_mask_poly_decode_host(*args) == -1, kw
        assert lib.cvlm_mask_poly_decode(*args, k["ws"], k["wsb"], None) == -1, kw
    args = [base[n] for n in order]
    for ws, wsb in ((None, one), (p + 65544, one), (p + 65536, one - 16)):
        assert lib.cvlm_mask_poly_decode(*args, ws, wsb, None) == -1, (ws, wsb)


def test_poly_symbols_are_exported_at_abi_12():
    lib = hip.load()
    assert hip.ABI_VERSION == 12 and lib.cvlm_abi_version() == 12
    for name in ("cvlm_mask_poly_decode", "cvlm_mask_poly_decode_workspace_bytes", "cvlm_debug_mask_poly_decode_host"):
        assert name in hip.EXPORTS and hasattr(lib, name)
    assert hip._SIGNATURES["cvlm_mask_poly_decode"] == hip._SIGNATURES["cvlm_debug_mask_poly_decode_host"] + "pls"
