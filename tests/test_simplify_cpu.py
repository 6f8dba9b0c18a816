"""Simplified contour rings without a device: the definition (tests/simplify_oracle.py, a recursive split in Python
ints) against its consequences -- T = 0 is the identity, the kept vertices are a subsequence from v_0 with the rings in order, every
vertex within T / 4 of the segment that brackets it, the rectangle and the one-pixel square --, hand cases, cvlm_debug_contour_simplify_host
(the kernels' key, keep test and anchor rule run sequentially) against the definition on everything the device tests run, every refusal
and every CVLM_E_BADARG, every ValueError of `simplify_request` with the launchers replaced by a recorder, and `MaskPolygons` on host
tensors.

The chord with coincident ends (P_i = P_j): two kept neighbours never coincide on a ring that has two distinct points -- when the later
of the two is tested, the earlier is an end of its chord and its distance 0, which no tolerance keeps -- so on crack contours that
branch of the key is reached only as the clamp of a revisited point against the chord's end.  The chain's ring does revisit every
diagonal point (asserted); the branch itself is reached on a ring whose vertices all coincide (asserted)."""
import ctypes

import numpy as np
import pytest
import torch

import contour_oracle as CO
import simplify_oracle as SO

T_ALL = (0, 1, 2, 4, 12, 65535)


# ---- the definition against its consequences ------------------------------------------------------------------------------------------------
def oracle_planes():
    rng = np.random.default_rng(34)
    planes = [m for _, m in CO.contents(20, 40, 3434)]
    planes += [rng.random(s) < d for d in (0.1, 0.3, 0.5, 0.7, 0.9) for s in ((20, 40), (7, 13))]
    return planes


@pytest.mark.parametrize("connectivity", [4, 8])
def test_the_definition_has_its_consequences(connectivity):
    for rings in SO.cached(("consequences", connectivity), lambda: SO.rings_of_planes(oracle_planes(), connectivity)):
        for T in T_ALL:
            want = SO.simplify_plane(rings, T)
            if T == 0:                                                # 1: the identity
                assert want["keep"].all() and want["dropped"] == 0 and want["xy"].shape[0] == sum(len(r) for r in rings)
            starts = []
            for ring in rings:
                kept, _, _ = SO.simplify_ring(ring, T)
                if not kept:
                    continue
                assert kept[0] == 0 and len(kept) >= 3 and kept == sorted(set(kept))           # 2: a subsequence from v_0
                assert SO.within(ring, kept, T)                                                   # 3: the Hausdorff bound, in integers
                starts.append(tuple(ring[0][::-1]))
            assert starts == sorted(starts)                                                       # 2: the rings keep their order
            out = CO.split(want["xy"], want["ring_start"])
            assert [tuple(r[0][::-1]) for r in out] == starts and sum(want["n_rings"]) == len(starts)


def rectangle(h, w, H=8, W=12):
    m = np.zeros((H, W), dtype=bool)
    m[1:1 + h, 1:1 + w] = True
    return m


def test_a_rectangle_keeps_its_corners_up_to_its_reach():
    """4: the far corner is B; the other two lie w h / sqrt(w^2 + h^2) from the diagonal, below the shorter side."""
    h, w = 6, 10
    ring = CO.rings_of(rectangle(h, w), 8)
    for T in range(0, 40):
        kept, _, _ = SO.simplify_ring(ring[0], T)
        assert (kept == [0, 1, 2, 3]) == (16 * (w * h) ** 2 > T * T * (w * w + h * h)), T
        assert kept in ([0, 1, 2, 3], [])
    assert SO.simplify_ring(ring[0], 20)[0] == [0, 1, 2, 3] and SO.simplify_ring(ring[0], 21)[0] == []       # 5.145 px


def test_a_single_pixel_is_kept_at_2_and_dropped_at_4():
    ring = CO.rings_of(rectangle(1, 1), 8)
    assert SO.simplify_ring(ring[0], 2)[0] == [0, 1, 2, 3]
    for T in (3, 4, 65535):
        assert SO.simplify_ring(ring[0], T)[0] == []
    want = SO.simplify_plane(ring, 4)
    assert want["dropped"] == 1 and want["n_rings"] == (0, 0) and want["xy"].shape[0] == 0 and not want["keep"].any()


def test_a_disc_shrinks_with_the_tolerance_and_stays_within_it():
    ring = CO.rings_of(SO.disc(20), 8)[0]
    counts = []
    for T in (0, 2, 4, 8, 12, 40):
        kept, depth, _ = SO.simplify_ring(ring, T)
        assert SO.within(ring, kept, T) and kept[0] == 0
        counts.append(len(kept))
    assert counts[0] == len(ring) and counts == sorted(counts, reverse=True) and counts[2] < len(ring) // 4 and counts[-1] >= 3


def test_a_diagonal_staircase_collapses():
    ring = CO.rings_of(SO.staircase(24), 4)
    assert len(ring) == 1 and len(ring[0]) == 96
    assert len(SO.simplify_ring(ring[0], 2)[0]) > 90                  # half a pixel: the steps stay
    assert len(SO.simplify_ring(ring[0], 4)[0]) == 4                  # one pixel: a thin parallelogram
    assert SO.simplify_ring(ring[0], 12)[0] == []                     # three: within reach of one segment


def test_the_chain_revisits_points_and_coincident_ends_are_reached_on_a_ring_of_one_point():
    ring = CO.rings_of(CO.chain(40), 8)
    assert len(ring) == 1 and len(ring[0]) == 160
    points = [tuple(p) for p in ring[0]]
    assert len(set(points)) == len(points) - 39                       # every inner diagonal point twice
    for T in T_ALL:
        kept, _, coincident = SO.simplify_ring(ring[0], T)
        assert not coincident and SO.within(ring[0], kept, T)
    dot = [np.asarray([[5, 7]] * 4, dtype=np.int64)]                  # no contour's ring: B = A, the chord (A, closing A)
    kept, _, coincident = SO.simplify_ring(dot[0], 0)
    assert coincident and kept == []
    for host_T in (0, 4):
        res = SO.run([dot, ring], [host_T, 2], host=True)
        assert res["status"] == (0, 0) and res["n_kept"][0] == 0 and not res["keep"][0].any() and tuple(res["n_rings"][0]) == (0, 0)
        assert np.array_equal(res["keep"][1], SO.simplify_plane(ring, 2)["keep"])


# ---- the host entry against the definition, on everything the device tests run ---------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("w", CO.WIDTHS)
def test_host_entry_on_every_width(w, connectivity):
    rings = SO.width_rings(w, connectivity)
    for T in SO.TOLERANCES:
        Ts = [T] * len(rings)
        res = SO.run(rings, Ts, host=True)
        assert res["status"] == (0, 0)
        SO.check(res, rings, Ts)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_host_entry_chain_comb_random_and_many_rings(connectivity):
    named = SO.big_rings(connectivity)
    rings = [r for _, r in named]
    depth = 0
    for T in SO.TOLERANCES:
        Ts = [T] * len(rings)
        res = SO.run(rings, Ts, host=True)
        assert res["status"] == (0, 0)
        SO.check(res, rings, Ts)
        depth = max(depth, max(SO.simplify_plane(r, T)["depth"] for r in rings))
    assert depth >= 8                                                 # the device's round loop is really iterated on these
    assert len(rings[0]) == (1 if connectivity == 8 else 300) and sum(len(r) for r in rings[0]) == 1200
    assert max(len(r) for r in rings[1]) > 1024 and len(rings[3]) > 500
    assert SO.simplify_plane(rings[3], 4)["dropped"] > 500


def test_host_entry_ragged_planes_mixed_tolerances_and_a_second_call():
    rings = SO.ragged_rings()
    Ts = [0, 2, 65535, 4, 1, 12, 3]
    res = SO.run(rings, Ts, host=True)
    assert res["status"] == (0, 0)
    SO.check(res, rings, Ts)
    moved = SO.run(rings, Ts, host=True, shift=4)                     # a base 4 bytes off 16
    SO.same(res, dict(moved, outs=None))
    other = [12, 0, 0, 2, 65535, 1, 4]
    again = SO.run(rings, other, host=True, outs=res["outs"])        # other tolerances into used outputs
    assert again["status"] == (0, 0)
    SO.check(again, rings, other)
    nothing = SO.run([[] for _ in rings], Ts, host=True)              # planes without a ring: total is 0
    assert nothing["status"] == (0, 0) and nothing["n_kept"].sum() == 0


def refusals():
    """(name, keyword arguments of SO.run, tolerances, refused planes, planes one short) on five planes: a refused plane at the first,
    a middle and the last position."""
    rings = SO.ragged_rings()[1:6]
    total = sum(len(r) for p in rings for r in p)
    vo = np.concatenate([[0], np.cumsum([sum(len(r) for r in p) for p in rings])]).astype(np.int64)
    good = [2, 4, 0, 2, 4]
    negative, beyond, backwards = vo.copy(), vo.copy(), vo.copy()
    negative[0] = -4
    beyond[5] = total + 4
    backwards[5] = vo[4] - 4                                          # the last plane: v1 < v0
    cases = [("a negative tolerance first", {}, [-1] + good[1:], (0,), ()),
             ("a tolerance of 65536 in the middle", {}, good[:2] + [65536] + good[3:], (2,), ()),
             ("a negative tolerance last", {}, good[:4] + [-(1 << 31)], (4,), ()),
             ("tolerances first, middle and last", {}, [65536, 2, -7, 4, 1 << 30], (0, 2, 4), ()),
             ("a slice that starts before the table", dict(vertex_offsets=negative), good, (0,), ()),
             ("a slice past the table", dict(vertex_offsets=beyond), good, (4,), ()),
             ("a slice that ends before it starts", dict(vertex_offsets=backwards), good, (4,), ()),
             ("a first vertex that starts no ring", dict(spoil_start=(0, 3)), good, (0, 3), ()),
             ("an output slice one short for a middle plane", dict(short=2), good, (), (2,))]
    return rings, good, cases


@pytest.mark.parametrize("name", [c[0] for c in refusals()[2]])
def test_host_entry_refuses_whole_planes(name):
    rings, good, cases = refusals()
    _, kw, Ts, refused, short = next(c for c in cases if c[0] == name)
    res = SO.run(rings, Ts, host=True, **kw)
    assert max(res["status"]) == 1 and res["status"][0] == (0 if short else 1)
    SO.check(res, rings, Ts, refused=refused, short=short)
    whole = SO.run(rings, good, host=True, outs=res["outs"])         # the status is zeroed by the next call
    assert whole["status"] == (0, 0)
    SO.check(whole, rings, good)


# ---- CVLM_E_BADARG and the exports --------------------------------------------------------------------------------------------------------
def test_every_badarg_of_the_simplify_entries():
    from camouflaged_vlm_amd import hip
    lib = hip.load()
    P, total, total_out = 2, 12, 12
    need = lib.cvlm_contour_simplify_workspace_bytes(P, total)
    assert need == 24 * total + 16 and lib.cvlm_contour_simplify_workspace_bytes(1, 0) == 16 and need % 16 == 0
    assert lib.cvlm_contour_simplify_workspace_bytes(3, 5) == 128 + 16
    big = torch.zeros(4 * total + 16 + 3 * 16 + 4 * total_out + 16 + need + 64, dtype=torch.uint8)
    held = dict(big=big, vo=torch.tensor([0, 4, 12, 12], dtype=torch.int64), oo=torch.tensor([0, 4, 12, 12], dtype=torch.int64),
                T=torch.tensor([2, 2, 2], dtype=torch.int32), n_kept=torch.zeros(3, dtype=torch.int32), rings=torch.zeros(5, dtype=torch.int32),
                status=torch.zeros(2, dtype=torch.int32))
    base = big.data_ptr()
    base += -base % 16
    xy, start = base, base + 4 * total                                # 48 bytes of vertices, then 16 each for ring_start, keep and ring_start_out
    keep, start_out = start + 16, start + 32
    xy_out = start + 48
    ws = xy_out + 4 * total_out
    ws += -ws % 16
    src = np.asarray([[0, 0], [3, 0], [3, 3], [0, 3], [5, 5], [9, 5], [9, 6], [7, 6], [7, 8], [9, 8], [9, 9], [5, 9]], dtype=np.int16)
    ctypes.memmove(xy, src.ctypes.data, 4 * total)
    ctypes.memmove(start, np.asarray([1, 0, 0, 0, 1] + [0] * 7, dtype=np.uint8).ctypes.data, total)
    rings = dict(xy=xy, ring_start=start, vertex_offsets=held["vo"].data_ptr(), total=total)
    mark = dict(rings, T=held["T"].data_ptr(), P=P, round_vertices=total, keep=keep, n_kept=held["n_kept"].data_ptr(),
                n_rings_out=held["rings"].data_ptr(), status=held["status"].data_ptr(), workspace=ws, workspace_bytes=need)
    emit = dict(rings, keep=keep, P=P, out_offsets=held["oo"].data_ptr(), xy_out=xy_out, ring_start_out=start_out, total_out=total_out,
                status=held["status"].data_ptr())
    host = dict(rings, T=held["T"].data_ptr(), P=P, keep=keep, n_kept=held["n_kept"].data_ptr(), n_rings_out=held["rings"].data_ptr(),
                out_offsets=held["oo"].data_ptr(), xy_out=xy_out, ring_start_out=start_out, total_out=total_out, status=held["status"].data_ptr())

    def call(fn, good, stream, **change):
        args = [dict(good, **change)[k] for k in good]
        return fn(*args, None) if stream else fn(*args)

    m = lambda **ch: call(lib.cvlm_contour_simplify_mark, mark, True, **ch)
    e = lambda **ch: call(lib.cvlm_contour_simplify_emit, emit, True, **ch)
    h = lambda **ch: call(lib.cvlm_debug_contour_simplify_host, host, False, **ch)
    assert h() == 0 and held["n_kept"].tolist()[:2] == [4, 8] and held["status"][0] == 0
    assert h(out_offsets=None, xy_out=None, ring_start_out=None, total_out=0) == 0
    assert h(out_offsets=None) == -1 and h(out_offsets=None, xy_out=None) == -1                  # the outputs come together or not at all
    shared = [{k: None} for k in ("xy", "ring_start", "vertex_offsets", "keep", "status")]
    shared += [dict(xy=xy + 2), dict(vertex_offsets=rings["vertex_offsets"] + 4), dict(status=mark["status"] + 2), dict(total=-1)]
    shared += [dict(P=0), dict(P=65536), dict(P=-1)]
    marks = [{k: None} for k in ("T", "n_kept", "n_rings_out")] + [{k: mark[k] + 2} for k in ("T", "n_kept", "n_rings_out")]
    marks += [dict(keep=xy), dict(keep=xy + 4 * total - 1), dict(keep=start + total - 1), dict(n_kept=xy), dict(n_rings_out=start - 4),
              dict(status=xy + 8), dict(n_kept=mark["T"]), dict(n_rings_out=rings["vertex_offsets"]), dict(n_kept=mark["n_rings_out"]),
              dict(status=mark["n_kept"] + 4), dict(status=mark["T"])]
    outs = [{k: None} for k in ("out_offsets", "xy_out", "ring_start_out")] + [dict(xy_out=xy_out + 2), dict(out_offsets=emit["out_offsets"] + 4)]
    outs += [dict(total_out=-1), dict(xy_out=xy), dict(xy_out=xy + 4 * total - 4), dict(ring_start_out=start + total - 1), dict(ring_start_out=keep),
             dict(xy_out=keep - 16), dict(ring_start_out=xy_out), dict(status=xy_out + 4), dict(status=emit["out_offsets"]),
             dict(ring_start_out=rings["vertex_offsets"] + 3)]
    for change in shared + marks:
        assert m(**change) == -1, change
        assert h(**change) == -1, change
    for change in shared + outs:
        assert e(**change) == -1, change
    for change in outs:
        assert h(**change) == -1, change
    for change in [dict(workspace=None), dict(workspace=ws + 4), dict(workspace_bytes=need - 1), dict(workspace_bytes=0), dict(round_vertices=-1),
                   dict(round_vertices=P * (1 << 22) + 1), dict(round_vertices=total + 1), dict(workspace=xy), dict(workspace=keep),
                   dict(workspace=xy + 4 * total - 16), dict(workspace=mark["n_kept"] - mark["n_kept"] % 16)]:
        assert m(**change) == -1, change
    empty = torch.zeros(3, dtype=torch.int64).data_ptr()
    assert h(total=0, xy=None, ring_start=None, keep=None, vertex_offsets=empty, total_out=0, xy_out=None, ring_start_out=None,
             out_offsets=empty) == 0                                  # empty tables need no vertices
    for bad in ((0, 1), (65536, 1), (1, -1), (1, (1 << 22) + 1)):
        assert lib.cvlm_contour_simplify_workspace_bytes(*bad) == -1, bad


def test_exports_stay_at_abi_12():
    from camouflaged_vlm_amd import hip
    lib = hip.load()
    assert lib.cvlm_abi_version() == hip.ABI_VERSION == 12
    names = ("cvlm_contour_simplify_mark", "cvlm_contour_simplify_emit", "cvlm_debug_contour_simplify_host")
    for name in names:
        assert name in hip.EXPORTS and hasattr(lib, name) and hip.ABI[name][0] is ctypes.c_int32
    assert hip.ABI["cvlm_contour_simplify_workspace_bytes"][0] is ctypes.c_int64
    assert {n for n in names if n in hip._STREAMED} == {"cvlm_contour_simplify_mark", "cvlm_contour_simplify_emit"}


def launcher_rows():
    """The three launchers in the form of tests/test_binding_checks_cpu.py's table: (name, host form, symbol, arguments, groups, free)."""
    i32, i64, u8, i16 = torch.int32, torch.int64, torch.uint8, torch.int16
    z = lambda dtype, *shape: torch.zeros(*shape, dtype=dtype)
    rings = dict(xy=z(i16, 8, 2), ring_start=z(u8, 8), vertex_offsets=torch.tensor([0, 4, 8]))
    marks = dict(T=z(i32, 2), keep=z(u8, 8), n_kept=z(i32, 2), n_rings_out=z(i32, 2, 2), status=z(i32, 1))
    outs = dict(out_offsets=torch.tensor([0, 4, 8]), xy_out=z(i16, 8, 2), ring_start_out=z(u8, 8))
    return [("contour_simplify_mark", False, "cvlm_contour_simplify_mark", dict(rings, **marks, round_vertices=8, workspace=z(u8, 256)), (),
             ("xy", "vertex_offsets", "workspace")),
            ("contour_simplify_emit", False, "cvlm_contour_simplify_emit", dict(rings, keep=z(u8, 8), **outs, status=z(i32, 1)), (),
             ("xy", "vertex_offsets", "xy_out")),
            ("contour_simplify_sequential", True, "cvlm_debug_contour_simplify_host", dict(rings, **marks, **outs), (tuple(outs),),
             ("xy", "vertex_offsets", "xy_out"))]


@pytest.mark.parametrize("row", launcher_rows(), ids=lambda r: r[0])
def test_a_spoiled_tensor_is_refused_before_the_call(row, monkeypatch):
    """What tests/test_binding_checks_cpu.py asks of every launcher with a host form, of these three (the sequential form carries no
    `_host` suffix: that test's table is closed)."""
    import test_binding_checks_cpu as BC
    from camouflaged_vlm_amd import hip
    calls = []
    monkeypatch.setattr(hip, "_call", lambda name, *a: calls.append(name))
    name, host, symbol, args, together, free = row
    fn = getattr(hip, name)
    if host:
        fn(**args)
        assert calls == [symbol]
    else:
        with pytest.raises(RuntimeError):
            fn(**args)
        assert calls == []
    calls.clear()
    accepted = []
    for what, bad in BC.mutations(args, together, free):
        try:
            fn(**bad)
            accepted.append(what)
        except AssertionError:
            pass
        except Exception as err:                            # noqa: BLE001 -- any other error is reported with the mutation that raised it
            accepted.append(f"{what} -> {type(err).__name__}")
    assert accepted == [] and calls == []


# ---- simplify_request and MaskPolygons ----------------------------------------------------------------------------------------------------------
SIZES = [(480, 640), (100, 75), (1, 1)]

BAD_REQUESTS = {
    "0.3 px": dict(tolerance=0.3),
    "-1 px": dict(tolerance=-1),
    "-0.25 px": dict(tolerance=-0.25),
    "a bool": dict(tolerance=True),
    "a numpy bool": dict(tolerance=np.bool_(False)),
    "16384 px": dict(tolerance=16384),
    "16383.76 px": dict(tolerance=16383.76),
    "nan": dict(tolerance=float("nan")),
    "inf": dict(tolerance=float("inf")),
    "a string": dict(tolerance="1"),
    "None": dict(tolerance=None),
    "a list of the wrong length": dict(tolerance=[1.0, 2.0]),
    "a list with 0.3": dict(tolerance=[1.0, 0.3, 2.0]),
    "a list with a bool": dict(tolerance=[1.0, True, 2.0]),
    "a list with 16384": dict(tolerance=[1.0, 1.0, 16384.0]),
    "a tensor": dict(tolerance=torch.ones(3)),
    "no sizes": dict(sizes=[]),
    "sizes a string": dict(sizes="480x640"),
    "a size a bool": dict(sizes=[(True, 4)]),
    "width 16385": dict(sizes=[(4, 16385)]),
    "too many planes": dict(sizes=[(1, 1)] * 65536),
}


@pytest.fixture
def launches(monkeypatch):
    """Every launcher the simplify call could reach, replaced by a recorder."""
    from camouflaged_vlm_amd import hip
    seen = []
    for name in ("contour_simplify_mark", "contour_simplify_emit", "contour_simplify_sequential", "contour_simplify_workspace_bytes"):
        monkeypatch.setattr(hip, name, lambda *a, _n=name, **k: seen.append(_n))
    return seen


@pytest.mark.parametrize("name", list(BAD_REQUESTS))
def test_bad_requests_raise_and_launch_nothing(name, launches):
    from camouflaged_vlm_amd import engine
    kw = dict(BAD_REQUESTS[name])
    sizes = kw.pop("sizes", SIZES)
    with pytest.raises(ValueError, match="simplify_contours"):
        engine.simplify_request(sizes, **kw)
    with pytest.raises(ValueError, match="someone"):
        engine.simplify_request(sizes, who="someone", **kw)
    assert launches == []


def host_polygons(planes, connectivity, Ts):
    """(MaskContours, MaskPolygons) on host tensors from the two host entries: what the device calls return, without a device."""
    import test_contour_cpu as CC
    from camouflaged_vlm_amd import engine
    mc = CC.host_contours(planes, connectivity)
    rings = SO.rings_of_planes(planes, connectivity)
    res = SO.run(rings, Ts, host=True)
    total = int(res["out_offsets"][-1])
    n_rings = torch.from_numpy(res["n_rings"])
    return mc, engine.MaskPolygons(xy=torch.from_numpy(np.concatenate(res["xy"]).reshape(total, 2)),
                                   ring_start=torch.from_numpy(np.concatenate(res["ring_start"])),
                                   vertex_offsets=torch.from_numpy(res["out_offsets"]), n_vertices=torch.from_numpy(res["n_kept"].astype(np.int32)),
                                   n_rings=n_rings, n_dropped=(mc.n_rings.sum(1) - n_rings.sum(1)).to(torch.int32), sizes=[p.shape for p in planes],
                                   tolerance=np.asarray(Ts, dtype=np.float64) / 4.0, status=torch.zeros(1, dtype=torch.int32))


def test_the_call_refuses_what_is_no_contours_before_any_launch(launches):
    from camouflaged_vlm_amd import engine
    util = engine.MaskUtilities.__new__(engine.MaskUtilities)
    import test_contour_cpu as CC
    mc = CC.host_contours([np.ones((3, 4), dtype=bool)], 8)
    for bad in (None, torch.zeros(4, 2, dtype=torch.int16), mc):      # a MaskContours on the host is none for the device call
        with pytest.raises(ValueError, match="simplify_contours"):
            engine.MaskUtilities.simplify_contours(util, bad)
    assert launches == []


def test_valid_requests(launches):
    from camouflaged_vlm_amd import engine
    import test_contour_cpu as CC
    mc = CC.host_contours([np.ones((3, 4), dtype=bool)] * 3, 8)
    for src in (SIZES, mc):
        assert engine.simplify_request(src).tolist() == [4, 4, 4] and engine.simplify_request(src).dtype == np.int32
        assert engine.simplify_request(src, tolerance=0).tolist() == [0, 0, 0]
        assert engine.simplify_request(src, tolerance=np.float32(0.75)).tolist() == [3, 3, 3]
        assert engine.simplify_request(src, tolerance=[0.25, np.int64(2), 16383.75]).tolist() == [1, 8, 65535]
        assert engine.simplify_request(src, tolerance=np.asarray([0.5, 1.0, 1.5])).tolist() == [2, 4, 6]
    assert engine.SIMPLIFY_MAX_T == 65535 and launches == []


@pytest.mark.parametrize("connectivity", [4, 8])
def test_to_coco_feeds_polygons_request_and_tells_holes_by_the_mark(connectivity):
    from camouflaged_vlm_amd import engine
    rng = np.random.default_rng(3402)
    planes = [rng.random(s) < 0.6 for s in CO.RAGGED]
    for m in planes:
        m[:3, :3] = True                                              # polygons_request takes no plane without a polygon
    planes[5][20:60, 30:90] = True
    planes[5][30:50, 40:80] = False                                   # a hole that survives
    Ts = [2, 4, 0, 4, 2, 6, 2]
    mc, mp = host_polygons(planes, connectivity, Ts)
    mp.check()
    coco = mp.to_coco()
    assert [d["size"] for d in coco] == [list(s) for s in CO.RAGGED] and mp.tolerance.tolist() == [t / 4 for t in Ts]
    xy, poly_offsets, plane_polys, sizes = engine.polygons_request(coco)                 # accepts this output
    assert sizes == [tuple(s) for s in CO.RAGGED] and plane_polys.tolist() == np.concatenate([[0], np.cumsum(mp.n_rings.sum(1).numpy())]).tolist()
    assert all(len(q) >= 6 for d in coco for q in d["polygons"])
    rings = mp.rings()
    assert rings.dtype == torch.int64 and rings[0] == 0 and rings[-1] == mp.xy.shape[0] and rings.numel() == int(mp.n_rings.sum()) + 1
    outer, areas = mp.to_coco(holes=False), mp.signed_areas()
    assert int(mp.n_rings[5, 1]) >= 1 and int(mp.n_dropped.sum()) > 0
    for p in range(len(planes)):
        assert len(coco[p]["polygons"]) == int(mp.n_rings[p].sum()) == areas[p].size
        assert len(outer[p]["polygons"]) == int(mp.n_rings[p, 0])
        marks = mp.ring_start[int(mp.vertex_offsets[p]):int(mp.vertex_offsets[p + 1])]
        marks = marks[marks != 0].tolist()
        assert outer[p]["polygons"] == [q for q, mark in zip(coco[p]["polygons"], marks) if mark == 1]       # exactly the rings marked 2 go
        assert int((mc.n_rings[p].sum() - mp.n_rings[p].sum())) == int(mp.n_dropped[p])
    identity = host_polygons(planes, connectivity, [0] * len(planes))[1]
    assert torch.equal(identity.xy, mc.xy) and torch.equal(identity.ring_start.ne(0), mc.ring_start.ne(0))
    assert torch.equal(identity.n_rings, mc.n_rings) and int(identity.n_dropped.sum()) == 0
    refused = engine.MaskPolygons(**{**mp.__dict__, "status": torch.ones(1, dtype=torch.int32)})
    with pytest.raises(RuntimeError, match="simplify_contours"):
        refused.check()
    with pytest.raises(RuntimeError, match="simplify_contours"):
        refused.to_coco()
