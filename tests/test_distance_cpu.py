"""Distance maps and surface distances without a GPU: the oracle (tests/distance_oracle.py) -- brute force against the
scipy form on 150 small planes, the reach rule, a tolerance count against scipy's dilation by the disc, the metric conventions for
every combination of empty and non-empty surfaces --; cvlm_debug_mask_distance_sized_host and cvlm_debug_mask_surface_totals_host --
the kernels' per-thread functions run sequentially -- against the oracle on the whole GPU list; every refusal; every CVLM_E_BADARG;
every ValueError of distance_request / surface_request with the launchers replaced by a recorder; the surface_tolerance table; the
exports.  Every comparison of integers is exact."""
import ctypes
import math

import numpy as np
import pytest
import torch

import boundary_oracle as BO
import distance_oracle as DO


def host_entries():
    from camouflaged_vlm_amd import hip
    return hip.mask_distance_sized_host, hip.mask_surface_totals_host


_CACHE = {}


def gpu_list():
    """distance_oracle.gpu_list with the unlimited map of every pattern, computed once for all the tests of a session."""
    if "list" not in _CACHE:
        planes, reaches, which, unique = DO.gpu_list()
        _CACHE["list"] = planes, reaches, which, [DO.d2_of(p) for p in unique]
    return _CACHE["list"]


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------------
def test_brute_force_equals_the_scipy_form():
    pytest.importorskip("scipy.ndimage")
    n = 0
    for h in (1, 2, 7, 20, 33):
        for w in (1, 31, 32, 33, 40, 65):
            for density in (0.0, 0.02, 0.5, 0.98, 1.0):
                x = np.random.default_rng(1000 * h + w).random((h, w)) < density
                assert np.array_equal(DO.brute(x), DO.edt(x)), (h, w, density)
                n += 1
    assert n == 150


def test_the_reach_rule():
    rng = np.random.default_rng(27)
    x = rng.random((33, 65)) < 0.01
    d2 = DO.d2_of(x)
    assert d2.max() > 49
    for R in (1, 2, 7, 100):
        cut = DO.d2_of(x, R)
        assert np.array_equal(cut[d2 <= R * R], d2[d2 <= R * R]) and (cut[d2 > R * R] == DO.FAR).all()
    assert np.array_equal(DO.d2_of(x, 0), d2) and (DO.d2_of(np.zeros((3, 4), dtype=bool)) == DO.FAR).all()
    assert 2 * 16383 ** 2 == 536805378 <= DO.MAX_REACH ** 2 < DO.FAR == 2 ** 31 - 1      # a reach of 23170 spans the largest plane's diagonal


def test_a_tolerance_count_is_a_dilation_by_the_disc():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(28)
    for r in (0, 1, 2, 3, 7):
        a, b = rng.random((40, 65)) < 0.1, rng.random((40, 65)) < 0.02
        yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
        disc = yy * yy + xx * xx <= r * r
        grown = ndimage.binary_dilation(np.pad(b, r), disc)[r:r + 40, r:r + 65]
        assert DO.totals(a, DO.d2_of(b), [r])["within"][0] == int((a & grown).sum()), r


def test_the_surface_is_the_boundary_at_radius_one():
    rng = np.random.default_rng(29)
    for shape in ((1, 1), (1, 40), (33, 65), (20, 7)):
        x = rng.random(shape) < 0.9
        assert np.array_equal(DO.surface(x), BO.boundary(x, 1)), shape


def test_the_metric_conventions_for_empty_surfaces():
    some = np.zeros((9, 9), dtype=bool)
    some[2:6, 3:7] = True
    none = np.zeros((9, 9), dtype=bool)
    tot = lambda a, b: (DO.totals(a, DO.d2_of(b), [0, 2]), DO.totals(b, DO.d2_of(a), [0, 2]))
    m = DO.metrics(*tot(none, none))
    assert m["hausdorff"] == m["assd"] == 0.0 and m["nsd"] == [1.0, 1.0] and m["precision"] == m["recall"] == m["f"] == [1.0, 1.0]
    m = DO.metrics(*tot(none, some))                                  # an empty prediction
    assert m["hausdorff"] == m["assd"] == math.inf and m["nsd"] == [0.0, 0.0]
    assert m["precision"] == [1.0, 1.0] and m["recall"] == [0.0, 0.0] and m["f"] == [0.0, 0.0]
    m = DO.metrics(*tot(some, none))                                  # an empty truth
    assert m["hausdorff"] == m["assd"] == math.inf and m["nsd"] == [0.0, 0.0]
    assert m["precision"] == [0.0, 0.0] and m["recall"] == [1.0, 1.0] and m["f"] == [0.0, 0.0]
    m = DO.metrics(*tot(some, some))
    assert m["hausdorff"] == m["assd"] == 0.0 and m["nsd"] == m["f"] == [1.0, 1.0]
    shifted = np.roll(some, 3, axis=1)                                # disjoint in part: no pixel within 0 of the other's far columns
    m = DO.metrics(*tot(some, shifted))
    assert m["hausdorff"] == 3.0 and 0.0 < m["nsd"][0] < m["nsd"][1] < 1.0 and 0.0 < m["assd"] < 3.0
    ab, ba = DO.totals(some, DO.d2_of(shifted, 1), [0]), DO.totals(shifted, DO.d2_of(some, 1), [0])
    assert ab["far"] > 0 and DO.metrics(ab, ba)["hausdorff"] == math.inf          # maps cut at a reach: no Hausdorff distance
    lone, other = none.copy(), none.copy()
    lone[0, 0] = other[8, 8] = True
    m = DO.metrics(*tot(lone, other))                                 # P + R = 0 with both surfaces non-empty
    assert m["f"] == [0.0, 0.0] and m["hausdorff"] == math.sqrt(128)


def test_surfeval_equals_the_plain_loops():
    from camouflaged_vlm_amd import surfeval
    rng = np.random.default_rng(30)
    planes = [rng.random((20, 33)) < d for d in (0.0, 0.05, 0.3, 0.0, 0.9)]
    pairs = [(p, q) for p in range(5) for q in range(5)]
    radii = [0, 1, 4]
    for reach in (0, 2):
        ab = [DO.totals(planes[p], DO.d2_of(planes[q], reach), radii) for p, q in pairs]
        ba = [DO.totals(planes[q], DO.d2_of(planes[p], reach), radii) for p, q in pairs]
        stack = lambda side: {k: np.asarray([t[k] for t in side]) for k in ("n", "far", "within", "max_d2", "sum_d2", "sum_d")}
        got = surfeval.surface_metrics(dict(ab=stack(ab), ba=stack(ba)))
        for i in range(len(pairs)):
            want = DO.metrics(ab[i], ba[i])
            for k, v in want.items():
                assert np.array_equal(np.asarray(got[k][i], dtype=np.float64), np.asarray(v, dtype=np.float64)), (reach, pairs[i], k)
    refused = {k: np.asarray([-1]) for k in ("n", "far", "max_d2", "sum_d2")}
    refused.update(within=np.full((1, 2), -1), sum_d=np.zeros(1))
    assert all(np.isnan(v).all() for v in surfeval.surface_metrics(dict(ab=refused, ba=refused)).values())


def test_surface_tolerance_table():
    from camouflaged_vlm_amd import engine
    for (h, w), r in {(480, 640): 7, (1024, 1024): 12, (1, 1): 1}.items():
        assert engine.surface_tolerance(h, w) == DO.surface_tolerance(h, w) == r, (h, w)
    assert engine.surface_tolerance(480, 640, 3) == 3 and engine.surface_tolerance(480, 640, 2.5) == 3 and engine.surface_tolerance(300, 400, 0.5) == 250
    assert isinstance(engine.surface_tolerance(480, 640), int)
    assert engine.DISTANCE_FAR == DO.FAR and engine.DISTANCE_MAX_REACH == DO.MAX_REACH and engine.SURFACE_MAX_T == 8


# ---- the host entries -----------------------------------------------------------------------------------------------------------------------
def test_host_distance_equals_the_oracle_on_the_gpu_list():
    planes, reaches, which, want = gpu_list()
    res = DO.run_distance(host_entries()[0], planes, reaches)
    assert res["status"] == 0
    DO.check_distance(res, planes, reaches, want=[want[i] for i in which])


def test_host_distance_on_the_planes_that_stress_the_passes():
    pytest.importorskip("scipy.ndimage")
    for name, plane in DO.stress_planes():
        res = DO.run_distance(host_entries()[0], [plane, plane], [0, 7])
        assert res["status"] == 0, name
        DO.check_distance(res, [plane, plane], [0, 7], want=[DO.edt(plane)] * 2)
    corner, wide = (DO.run_distance(host_entries()[0], [p], [0])["maps"][0] for _, p in DO.stress_planes()[:2])
    assert corner.max() == 178802 == 2 * 299 ** 2 and wide.max() == 16383 ** 2 + 1 and wide[0, 16383] == 16383 ** 2


def ragged_planes(seed: int = 27):
    rng = np.random.default_rng(seed)
    return [rng.random(s) < d for s, d in zip(DO.RAGGED, (1.0, 0.01, 0.5, 0.05, 0.2, 0.002, 0.0))]


def test_host_distance_on_ragged_planes_used_outputs_dirty_pads_and_an_unaligned_base():
    fn = host_entries()[0]
    planes, reaches = ragged_planes(), [0, 3, 0, 1, 0, 0, 5]
    res = DO.run_distance(fn, planes, reaches)
    assert res["status"] == 0
    DO.check_distance(res, planes, reaches)
    other = [~p for p in planes]
    used = DO.run_distance(fn, other, reaches[::-1], outs=res["outs"])
    assert used["status"] == 0
    DO.check_distance(used, other, reaches[::-1])
    dirty = DO.run_distance(fn, planes, reaches, shift=4, dirty_pads=True)
    DO.check_distance(dirty, planes, reaches)


REFUSAL_SIZES = [(5, 40), (33, 65), (3, 7)]


def refusals():
    """(name, keywords of run_distance, reaches, refused planes, untouched planes) on REFUSAL_SIZES: each kind of refused plane first,
    in the middle and last."""
    dims = np.asarray(REFUSAL_SIZES, dtype=np.int32)
    pix, n_pix = DO.pix_tables(REFUSAL_SIZES)
    out = []
    for p, where in enumerate(("first", "middle", "last")):
        for kind, change in (("h = 0", (0, None)), ("w = 16385", (None, 16385)), ("a size that is not the slice's", (dims[p, 0] + 1, None))):
            d = dims.copy()
            d[p] = [d[p, 0] if change[0] is None else change[0], d[p, 1] if change[1] is None else change[1]]
            out.append((f"{kind}, {where}", dict(dims=d), [0, 0, 0], (p,), ()))
        for R in (-1, DO.MAX_REACH + 1):
            reach = [2, 0, 1]
            reach[p] = R
            out.append((f"reach {R}, {where}", {}, reach, (p,), ()))
    before, beyond, seam = pix.copy(), pix.copy(), pix.copy()
    before[0] = -1
    beyond[3] = n_pix + 1
    seam[1] += 1
    out.append(("a pixel slice that starts before the map", dict(pix_offsets=before), [0, 0, 0], (), (0,)))
    out.append(("a pixel slice that ends beyond the map", dict(pix_offsets=beyond), [0, 0, 0], (), (2,)))
    out.append(("a pixel slice one entry long and its neighbour one short", dict(pix_offsets=seam), [0, 0, 0], (0, 1), ()))
    return out


@pytest.mark.parametrize("name", [c[0] for c in refusals()])
def test_host_distance_refuses_whole_planes(name):
    _, kw, reaches, refused, untouched = next(c for c in refusals() if c[0] == name)
    rng = np.random.default_rng(31)
    planes = [rng.random(s) < 0.1 for s in REFUSAL_SIZES]
    res = DO.run_distance(host_entries()[0], planes, reaches, **kw)
    assert res["status"] == 1
    DO.check_distance(res, planes, reaches, refused=refused, untouched=untouched)           # the neighbours are whole


def totals_cases(seed: int = 32):
    """(a planes, b planes, pairs, radii by T): random pairs of three sizes with empty planes on either side."""
    rng = np.random.default_rng(seed)
    sizes = [(33, 65), (33, 65), (33, 65), (7, 40), (7, 40), (130, 129), (130, 129), (1, 1), (1, 1)]
    a = [rng.random(s) < d for s, d in zip(sizes, (0.3, 0.0, 0.02, 0.5, 0.0, 0.1, 0.9, 1.0, 0.0))]
    b = [rng.random(s) < d for s, d in zip(sizes, (0.02, 0.4, 0.0, 0.0, 0.0, 0.01, 0.9, 1.0, 1.0))]
    same = lambda p, q: sizes[p] == sizes[q]
    pairs = [(p, q) for p in range(9) for q in range(9) if same(p, q)]
    base = (0, 1, 7, DO.MAX_REACH, 2, 3, 5, 100)
    return a, b, pairs, {T: [list(base[:T])] * len(pairs) for T in (1, 3, 8)}


@pytest.mark.parametrize("T", [1, 3, 8])
def test_host_totals_equal_the_plain_loops(T):
    a, b, pairs, radii = totals_cases()
    for reach in (0, 7):
        maps = [DO.d2_of(m, reach) for m in b]
        res = DO.run_totals(host_entries()[1], a, maps, pairs, radii[T])
        assert res["status"] == 0
        DO.check_totals(res, a, maps, pairs, radii[T])


def totals_refusals():
    """(name, keywords of run_totals, pairs, radii, refused pairs) on totals_cases' planes."""
    good = [(0, 1), (3, 4), (5, 6)]
    r = [[0, 2]] * 4
    one = lambda pair: good[:1] + [pair] + good[1:]
    sizes = [(33, 65), (33, 65), (33, 65), (7, 40), (7, 40), (130, 129), (130, 129), (1, 1), (1, 1)]
    pix, n_pix = DO.pix_tables(sizes)
    shifted = pix.copy()
    shifted[3] += 1                                                   # map 2 one entry long, map 3 one short
    dims = np.asarray(sizes, dtype=np.int32)
    grown = dims.copy()
    grown[3] = [8, 40]
    return [("planes of different sizes", {}, one((0, 3)), r, (1,)),
            ("a plane of a out of range", {}, one((9, 1)), r, (1,)),
            ("a negative plane of b", {}, one((0, -1)), r, (1,)),
            ("a radius above 23170", {}, one((1, 2)), [[0, 2], [0, DO.MAX_REACH + 1], [0, 2], [0, 2]], (1,)),
            ("a negative radius", {}, one((1, 2)), [[0, 2], [-1, 2], [0, 2], [0, 2]], (1,)),
            ("a map whose slice is not its size", dict(b_pix_offsets=shifted), one((1, 2)) + [(2, 3)], r + [[1, 1]], (1, 4)),
            ("a plane of a whose slice is not its size", dict(a_dims=grown), one((3, 3)), r, (1, 2))]


@pytest.mark.parametrize("name", [c[0] for c in totals_refusals()])
def test_host_totals_refuse_whole_pairs(name):
    _, kw, pairs, radii, refused = next(c for c in totals_refusals() if c[0] == name)
    a, b, _, _ = totals_cases()
    maps = [DO.d2_of(m) for m in b]
    res = DO.run_totals(host_entries()[1], a, maps, pairs, radii, **kw)
    assert res["status"] == 1
    DO.check_totals(res, a, maps, pairs, radii, refused=refused)


# ---- CVLM_E_BADARG and the exports --------------------------------------------------------------------------------------------------------
def test_every_badarg_of_the_distance_entry():
    from camouflaged_vlm_amd import hip
    lib = hip.load()
    sizes = [(5, 40), (3, 7)]
    dims, off, nbytes, max_words = BO.tables(sizes, guard=0)
    pix, n_pix = DO.pix_tables(sizes, band=0)
    need = DO.ws_need(n_pix)
    assert lib.cvlm_mask_distance_workspace_bytes(2, 200) == 800 >= need and lib.cvlm_mask_distance_workspace_bytes(1, 3) == 16
    for bad in ((0, 5), (65536, 5), (1, 0), (1, 16384 * 16384 + 1)):
        assert lib.cvlm_mask_distance_workspace_bytes(*bad) == -1, bad
    room = (nbytes + 15) // 16 * 16
    big = torch.zeros(room + need + 4 * n_pix + 64, dtype=torch.uint8)
    keep = dict(big=big, offsets=torch.from_numpy(off), dims=torch.from_numpy(dims), reach=torch.zeros(3, dtype=torch.int32),
                pix=torch.from_numpy(pix), status=torch.zeros(2, dtype=torch.int32))
    base = big.data_ptr()
    assert base % 16 == 0
    good = dict(bits=base, n_bytes=nbytes, offsets=keep["offsets"].data_ptr(), dims=keep["dims"].data_ptr(), reach=keep["reach"].data_ptr(),
                P=2, max_words=max_words, pix_offsets=keep["pix"].data_ptr(), n_pix=n_pix, workspace=base + room, ws_bytes=need,
                out_d2=base + room + need, status=keep["status"].data_ptr())
    order = list(good)

    def call(dev: bool, **change):
        args = [dict(good, **change)[k] for k in order]
        return lib.cvlm_mask_distance_sized(*args, None) if dev else lib.cvlm_debug_mask_distance_sized_host(*args)

    assert call(False) == 0
    bad = [{k: None} for k in ("bits", "offsets", "dims", "reach", "pix_offsets", "workspace", "out_d2", "status")]
    bad += [{k: good[k] + 2} for k in ("bits", "dims", "reach", "out_d2", "status")]
    bad += [dict(offsets=good["offsets"] + 4), dict(pix_offsets=good["pix_offsets"] + 4), dict(workspace=good["workspace"] + 8)]
    bad += [dict(P=0), dict(P=65536), dict(n_bytes=3), dict(n_pix=0), dict(max_words=0), dict(max_words=16384 * 512 + 1)]
    bad += [dict(out_d2=base), dict(out_d2=base + nbytes - 4), dict(workspace=base), dict(out_d2=good["workspace"]),
            dict(out_d2=good["workspace"] + need - 4), dict(status=good["out_d2"]), dict(status=good["workspace"]),
            dict(out_d2=good["dims"]), dict(workspace=base + 16)]
    for change in bad:
        for dev in (False, True):                                     # refused before the device is touched: no GPU is needed
            assert call(dev, **change) == -1, change
    for dev in (False, True):
        assert call(dev, ws_bytes=need - 16) == -3 and call(dev, ws_bytes=0) == -3                # CVLM_E_WORKSPACE


def test_every_badarg_of_the_totals_entry():
    from camouflaged_vlm_amd import hip
    lib = hip.load()
    sizes = [(5, 40), (3, 7)]
    dims, off, nbytes, max_words = BO.tables(sizes, guard=0)
    pix, n_pix = DO.pix_tables(sizes, band=0)
    N, T = 3, 2
    need = lib.cvlm_mask_surface_workspace_bytes(N)
    assert need == 8 * N * 256 and lib.cvlm_mask_surface_workspace_bytes(4096) == 8 * 4096 and lib.cvlm_mask_surface_workspace_bytes(1 << 24) == 8 << 24
    assert lib.cvlm_mask_surface_workspace_bytes(17) == (8 * 17 * 241 + 15) // 16 * 16
    assert lib.cvlm_mask_surface_workspace_bytes(0) == -1 and lib.cvlm_mask_surface_workspace_bytes((1 << 24) + 1) == -1
    i32 = lambda n: torch.zeros(n + 1, dtype=torch.int32)
    keep = dict(a_bits=torch.zeros(nbytes, dtype=torch.uint8), a_offsets=torch.from_numpy(off), a_dims=torch.from_numpy(dims),
                b_d2=i32(n_pix), b_pix_offsets=torch.from_numpy(pix), b_dims=torch.from_numpy(dims.copy()),
                pairs=torch.tensor([[0, 0], [1, 1], [0, 1]], dtype=torch.int32), radii=torch.ones(N, T, dtype=torch.int32),
                workspace=torch.zeros(need + 16, dtype=torch.uint8), n=i32(N), far=i32(N), within=i32(N * T), max_d2=i32(N),
                sum_d2=torch.zeros(N + 1, dtype=torch.int64), sum_d=torch.zeros(N + 1, dtype=torch.float64), status=i32(1))
    good = {k: v.data_ptr() for k, v in keep.items()}
    good.update(a_bytes=nbytes, Pa=2, b_n_pix=n_pix, Pb=2, N=N, T=T, max_words=max_words, ws_bytes=need)
    order = ["a_bits", "a_bytes", "a_offsets", "a_dims", "Pa", "b_d2", "b_pix_offsets", "b_n_pix", "b_dims", "Pb", "pairs", "N", "radii", "T",
             "max_words", "workspace", "ws_bytes", "n", "far", "within", "max_d2", "sum_d2", "sum_d", "status"]

    def call(dev: bool, **change):
        args = [dict(good, **change)[k] for k in order]
        return lib.cvlm_mask_surface_totals(*args, None) if dev else lib.cvlm_debug_mask_surface_totals_host(*args)

    assert call(False) == 0 and keep["status"][0] == 1 and keep["n"][:3].tolist() == [0, 0, -1]      # the pair of different sizes
    pointers = [k for k in order if k in keep]
    bad = [{k: None} for k in pointers]
    bad += [{k: good[k] + 2} for k in pointers if k not in ("a_offsets", "b_pix_offsets", "sum_d2", "sum_d", "workspace")]
    bad += [{k: good[k] + 4} for k in ("a_offsets", "b_pix_offsets", "sum_d2", "sum_d")] + [dict(workspace=good["workspace"] + 8)]
    bad += [dict(Pa=0), dict(Pa=65536), dict(Pb=0), dict(Pb=65536), dict(N=0), dict(N=(1 << 24) + 1), dict(T=0), dict(T=9), dict(a_bytes=3),
            dict(b_n_pix=0), dict(max_words=0), dict(max_words=16384 * 512 + 1)]
    bad += [dict(n=good["far"]), dict(within=good["n"] + 4), dict(max_d2=good["b_d2"]), dict(sum_d=good["sum_d2"]), dict(status=good["radii"]),
            dict(workspace=good["workspace"] + 16, n=good["workspace"] + need), dict(far=good["pairs"] + 8), dict(sum_d2=good["a_offsets"])]
    for change in bad:
        for dev in (False, True):
            assert call(dev, **change) == -1, change
    for dev in (False, True):
        assert call(dev, ws_bytes=need - 16) == -3


def test_exports_stay_at_abi_12():
    from camouflaged_vlm_amd import hip
    lib = hip.load()
    assert lib.cvlm_abi_version() == hip.ABI_VERSION == 12
    names = ("cvlm_mask_distance_sized", "cvlm_debug_mask_distance_sized_host", "cvlm_mask_surface_totals", "cvlm_debug_mask_surface_totals_host")
    for name in names:
        assert name in hip.EXPORTS and hasattr(lib, name) and hip.ABI[name][0] is ctypes.c_int32
    for name in ("cvlm_mask_distance_workspace_bytes", "cvlm_mask_surface_workspace_bytes"):
        assert name in hip.EXPORTS and hip.ABI[name][0] is ctypes.c_int64
    assert {n for n in names if n in hip._STREAMED} == {"cvlm_mask_distance_sized", "cvlm_mask_surface_totals"}
    assert hip.DT_FAR == DO.FAR


# ---- distance_request and surface_request ---------------------------------------------------------------------------------------------------
SIZES = [(480, 640), (100, 75), (1, 1)]

BAD_DISTANCE = {
    "no planes": dict(sizes=[]),
    "too many planes": dict(sizes=[(1, 1)] * 65536),
    "sizes a string": dict(sizes="480x640"),
    "a size of three": dict(sizes=[(480, 640, 3)]),
    "a side zero": dict(sizes=[(0, 640)]),
    "a side 16385": dict(sizes=[(480, 16385)]),
    "a side a bool": dict(sizes=[(True, 640)]),
    "a side a float": dict(sizes=[(480.0, 640)]),
    "reach negative": dict(reach=-1),
    "reach 23171": dict(reach=23171),
    "reach a bool": dict(reach=True),
    "reach a float": dict(reach=7.0),
    "reach a string": dict(reach="tolerance"),
    "reaches too short": dict(reach=[1, 2]),
    "one reach a bool": dict(reach=[1, False, 3]),
    "one reach 23171": dict(reach=[1, 23171, 3]),
}

BAD_SURFACE = {
    "no planes of a": dict(a_sizes=[]),
    "too many planes of b": dict(b_sizes=[(1, 1)] * 65536),
    "a side 16385": dict(a_sizes=[(480, 640), (100, 16385), (1, 1)]),
    "a side a bool": dict(b_sizes=[(480, 640), (100, 75), (True, 1)]),
    "no pairs and sides of different lengths": dict(b_sizes=SIZES[:2]),
    "no pairs and planes of different sizes": dict(b_sizes=[(480, 640), (75, 100), (1, 1)]),
    "pairs empty": dict(pairs=np.zeros((0, 2), dtype=np.int64)),
    "pairs of three": dict(pairs=[(0, 0, 0)]),
    "pairs of floats": dict(pairs=[(0.0, 0.0)]),
    "pairs of bools": dict(pairs=[(True, True)]),
    "a pair out of range": dict(pairs=[(0, 0), (3, 1)]),
    "a negative pair": dict(pairs=[(0, 0), (1, -1)]),
    "a pair of different sizes": dict(pairs=[(0, 0), (1, 2)]),
    "no tolerance": dict(tolerance=[]),
    "nine tolerances": dict(tolerance=[1] * 9),
    "tolerance a bool": dict(tolerance=True),
    "one tolerance a bool": dict(tolerance=[1, True]),
    "tolerance negative": dict(tolerance=-1),
    "tolerance 23171": dict(tolerance=23171),
    "tolerance 1.0": dict(tolerance=1.0),
    "tolerance 0.0": dict(tolerance=0.0),
    "tolerance 2.5": dict(tolerance=[2.5]),
    "tolerance NaN": dict(tolerance=float("nan")),
    "tolerance a string": dict(tolerance="0.008"),
    "tolerance None": dict(tolerance=None),
    "reach negative": dict(reach=-1),
    "reach 23171": dict(reach=23171),
    "reach a bool": dict(reach=True),
    "reach a float": dict(reach=7.0),
    "reach another string": dict(reach="radius"),
    "reach a list": dict(reach=[1, 2, 3]),
}


@pytest.fixture
def launches(monkeypatch):
    """Every launcher the distance calls could reach, replaced by a recorder."""
    from camouflaged_vlm_amd import hip
    seen = []
    for name in ("mask_distance_sized", "mask_distance_sized_host", "mask_surface_totals", "mask_surface_totals_host", "mask_boundary_sized"):
        monkeypatch.setattr(hip, name, lambda *a, _n=name, **k: seen.append(_n))
    return seen


@pytest.mark.parametrize("name", list(BAD_DISTANCE))
def test_bad_distance_requests_raise_and_launch_nothing(name, launches):
    from camouflaged_vlm_amd import engine
    kw = dict(dict(sizes=SIZES), **BAD_DISTANCE[name])
    with pytest.raises(ValueError, match="mask_distance_sized"):
        engine.distance_request(kw.pop("sizes"), **kw)
    kw = dict(dict(sizes=SIZES), **BAD_DISTANCE[name])
    with pytest.raises(ValueError, match="somebody"):
        engine.distance_request(kw.pop("sizes"), who="somebody", **kw)
    assert launches == []


@pytest.mark.parametrize("name", list(BAD_SURFACE))
def test_bad_surface_requests_raise_and_launch_nothing(name, launches):
    from camouflaged_vlm_amd import engine
    for who in ("mask_surface_distances", "somebody"):
        kw = dict(dict(a_sizes=SIZES, b_sizes=SIZES), **BAD_SURFACE[name])
        with pytest.raises(ValueError, match=who):
            engine.surface_request(kw.pop("a_sizes"), kw.pop("b_sizes"), who=who, **kw)
    assert launches == []


def test_bad_arguments_of_the_cascade_calls_raise_and_launch_nothing(launches):
    from camouflaged_vlm_amd import engine
    util = object.__new__(engine.MaskUtilities)
    for bad in (None, torch.zeros(4, dtype=torch.uint8), SIZES):
        with pytest.raises(ValueError, match="mask_distance_sized"):
            engine.MaskUtilities.mask_distance_sized(util, bad)
        with pytest.raises(ValueError, match="mask_surface_distances"):
            engine.MaskUtilities.mask_surface_distances(util, bad, bad)
    assert launches == []


def test_request_tables(launches):
    from camouflaged_vlm_amd import engine
    sizes, reach = engine.distance_request(SIZES)
    assert sizes == SIZES and reach.dtype == np.int32 and reach.tolist() == [0, 0, 0]
    assert engine.distance_request(SIZES, reach=0)[1].tolist() == [0, 0, 0] and engine.distance_request(SIZES, reach=23170)[1].tolist() == [23170] * 3
    assert engine.distance_request(SIZES, reach=[1, 0, np.int64(7)])[1].tolist() == [1, 0, 7]
    r = engine.surface_request(SIZES, SIZES)
    assert r.pairs.tolist() == [[0, 0], [1, 1], [2, 2]] and r.radii.dtype == np.int32 and r.radii.tolist() == [[7], [1], [1]]
    assert r.reach_a.tolist() == r.reach_b.tolist() == [0, 0, 0]
    r = engine.surface_request(SIZES, SIZES + SIZES, pairs=[(0, 3), (0, 0), (2, 5)], tolerance=[0, 0.008, 3, 0.05], reach="tolerance")
    assert r.radii.tolist() == [[0, 7, 3, 40], [0, 7, 3, 40], [0, 1, 3, 1]]
    assert r.reach_a.tolist() == [40, 1, 3] and r.reach_b.tolist() == [40, 1, 1, 40, 1, 3]      # an unnamed plane: 1, never the unlimited 0
    assert engine.surface_request(SIZES, SIZES, tolerance=0, reach="tolerance").reach_a.tolist() == [1, 1, 1]
    assert engine.surface_request(SIZES, SIZES, tolerance=np.float32(0.5), reach=5).radii.tolist() == [[400], [63], [1]]
    assert launches == []


def test_rounds_are_consecutive_pairs_under_the_cap():
    from camouflaged_vlm_amd import engine
    sizes = [(10, 10)] * 4 + [(20, 20)]
    pairs = np.asarray([(0, 1), (0, 2), (3, 3), (4, 4), (0, 0)], dtype=np.int32)
    whole = engine.surface_rounds(pairs, sizes, sizes, 1 << 30)
    assert whole == [(0, 5, [0, 3, 4], [0, 1, 2, 3, 4], 6 * 800)]
    assert engine.surface_rounds(pairs, sizes, sizes, 1) == [(i, i + 1, [int(p)], [int(q)], 6 * sizes[p][0] * sizes[p][1]) for i, (p, q) in enumerate(pairs)]
    two = engine.surface_rounds(pairs, sizes, sizes, 6 * 300)         # three small maps at a time
    assert [(r[0], r[1]) for r in two] == [(0, 3), (3, 4), (4, 5)] and two[0][2:] == ([0, 3], [1, 2, 3], 1800)
