"""Simplified contour rings on the device: cvlm_contour_simplify_mark / cvlm_contour_simplify_emit against the
definition (tests/simplify_oracle.py) and against the host entry, mark for mark and vertex for vertex -- every comparison is exact --
on the rings of every width that crosses a word seam at heights 1, 2 and 33, both connectivities, tolerances 0, 0.5, 1 and 3 pixels,
the planes of one width in one call; the 300 x 300 chain (one ring of 1200 vertices that revisits every inner point, or 300 rings of
4), the comb whose ring is longer than one pass of the workgroup, 65 x 129 random planes and a plane of hundreds of rings most of
which are dropped; tolerances mixed in one call, ragged planes in one call and in three rounds, used outputs and a used workspace,
guard bands, a base 4 bytes off 16, every refusal; and Cascade.simplify_contours and the drop-in on the tiny cascade."""
import numpy as np
import pytest
import torch

import contour_oracle as CO
import simplify_oracle as SO
import test_simplify_cpu as CPU
from test_contour_gpu import sized_of
from test_labels_gpu import tracer  # noqa: F401  (fixture)
from test_match_gpu import CLASSES, cas, dropin, gold, record_reads, tiny  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("w", CO.WIDTHS)
def test_device_equals_the_oracle_and_the_host_entry(w, connectivity):
    """Every content at the three heights of one width: ONE call per tolerance."""
    rings = SO.width_rings(w, connectivity)
    for T in SO.TOLERANCES:
        Ts = [T] * len(rings)
        res = SO.run(rings, Ts, dev=DEV)
        assert res["status"] == (0, 0)
        SO.check(res, rings, Ts)
        SO.same(res, SO.run(rings, Ts, host=True))


@pytest.mark.parametrize("connectivity", [4, 8])
def test_chain_comb_random_and_many_rings(connectivity):
    """The round loop really iterated (a recursion 8 deep at the least), a ring longer than one pass of the workgroup, a ring that
    revisits points, ring bases from the scan, hundreds of dropped rings."""
    rings = [r for _, r in SO.big_rings(connectivity)]
    depth = 0
    for T in SO.TOLERANCES:
        Ts = [T] * len(rings)
        res = SO.run(rings, Ts, dev=DEV)
        assert res["status"] == (0, 0)
        SO.check(res, rings, Ts)
        SO.same(res, SO.run(rings, Ts, host=True))
        depth = max(depth, max(SO.simplify_plane(r, T)["depth"] for r in rings))
        if T == 0:
            assert res["n_kept"].tolist() == [sum(len(x) for x in r) for r in rings]
        if T == 4:
            assert res["n_kept"][0] == 0 and tuple(res["n_rings"][0]) == (0, 0)               # every pixel of the chain is dropped at 1 px
            assert sum(len(x) for x in rings[3]) > 2000 and res["n_kept"][3] <= 8
    assert depth >= 8
    assert max(len(x) for x in rings[1]) > 1024


@pytest.mark.parametrize("connectivity", [4, 8])
def test_ragged_planes_mixed_tolerances_rounds_used_outputs_and_an_unaligned_base(connectivity):
    rings = SO.ragged_rings(connectivity)
    Ts = [0, 2, 65535, 4, 1, 12, 3]                                   # one tolerance per plane, mixed in one call
    res = SO.run(rings, Ts, dev=DEV)
    assert res["status"] == (0, 0)
    SO.check(res, rings, Ts)
    host = SO.run(rings, Ts, host=True)
    SO.same(res, host)
    SO.same(SO.run(rings, Ts, dev=DEV, rounds=3), host)               # three mark calls through workspaces of their own size
    other = [12, 0, 0, 2, 65535, 1, 4]
    used = SO.run(rings, other, dev=DEV, outs=res["outs"])           # other tolerances into used outputs and a used workspace
    assert used["status"] == (0, 0)
    SO.check(used, rings, other)
    SO.same(SO.run(rings, Ts, dev=DEV, shift=4), host)                # xy 4 bytes off a 16-byte boundary
    nothing = SO.run([[] for _ in rings], Ts, dev=DEV)                # planes without a ring: no vertex, nothing to store
    assert nothing["status"] == (0, 0) and nothing["n_kept"].sum() == 0


@pytest.mark.parametrize("name", [c[0] for c in CPU.refusals()[2]])
def test_refuses_whole_planes(name):
    rings, good, cases = CPU.refusals()
    _, kw, Ts, refused, short = next(c for c in cases if c[0] == name)
    res = SO.run(rings, Ts, dev=DEV, **kw)
    assert max(res["status"]) == 1 and res["status"][0] == (0 if short else 1)
    SO.check(res, rings, Ts, refused=refused, short=short)            # the neighbours are whole
    host = SO.run(rings, Ts, host=True, **kw)
    SO.same(dict(res, status=max(res["status"])), dict(host, status=max(host["status"])))
    whole = SO.run(rings, good, dev=DEV, outs=res["outs"])           # the status is zeroed by the next call
    assert whole["status"] == (0, 0)
    SO.check(whole, rings, good)


def test_every_badarg_leaves_the_device_alone():
    CPU.test_every_badarg_of_the_simplify_entries()
    torch.cuda.synchronize()


# ---- through the engine ---------------------------------------------------------------------------------------------------------------------------
def as_result(mp) -> dict:
    """A MaskPolygons in the form of SO.run's result, for SO.check (the marks aside)."""
    vo = mp.vertex_offsets.cpu().tolist()
    return dict(xy=[mp.xy[a:b].cpu().numpy() for a, b in zip(vo[:-1], vo[1:])],
                ring_start=[mp.ring_start[a:b].cpu().numpy() for a, b in zip(vo[:-1], vo[1:])],
                n_kept=mp.n_vertices.cpu().numpy(), n_rings=mp.n_rings.cpu().numpy())


def check_polygons(mp, rings, Ts) -> None:
    got = as_result(mp)
    for p, (r, T) in enumerate(zip(rings, Ts)):
        want = SO.simplify_plane(r, int(T))
        assert np.array_equal(got["xy"][p], want["xy"]) and np.array_equal(got["ring_start"][p], want["ring_start"]), p
        assert got["n_kept"][p] == want["xy"].shape[0] and tuple(got["n_rings"][p]) == want["n_rings"], p
        assert int(mp.n_dropped[p]) == want["dropped"], p


@pytest.mark.parametrize("connectivity", [4, 8])
def test_simplify_contours_through_the_cascade_under_two_caps(cas, dropin, connectivity, monkeypatch):
    """64 x 64 planes after mask_contours_sized: the call's polygons are the definition's; one read (the total of the kept counts) when
    the input fits one round; a cap that cuts the planes into rounds gives identical results; T = 0 returns the input's vertices."""
    from camouflaged_vlm_amd import hip, maskpost
    from camouflaged_vlm_amd.engine import MaskPolygons
    rng = np.random.default_rng(3403)
    planes = [rng.random((64, 64)) < d for d in (0.02, 0.3, 0.5, 0.7, 0.98)]
    ring = np.zeros((64, 64), dtype=bool)
    ring[8:56, 8:56] = True
    ring[16:48, 16:48] = False
    ring[24:40, 24:40] = True
    planes.append(ring)
    sized = sized_of(cas, planes)
    mc = cas.mask_contours_sized(sized, connectivity=connectivity)
    rings = SO.rings_of_planes(planes, connectivity)
    tol = [0.5, 1, 0.25, 2.0, 1.0, 3]
    Ts = [2, 4, 1, 8, 4, 12]
    torch.cuda.synchronize()
    reads = record_reads(monkeypatch)
    whole = cas.simplify_contours(mc, tolerance=tol)
    monkeypatch.undo()
    assert reads == ["item"], reads                                   # the one read of the counts
    assert isinstance(whole, MaskPolygons) and whole.sizes == [(64, 64)] * 6 and whole.tolerance.tolist() == [float(t) for t in tol]
    whole.check()
    check_polygons(whole, rings, Ts)
    assert tuple(whole.n_rings[5].tolist()) == (2, 1)                 # the squares stand at 3 px
    nv = mc.n_vertices.cpu().numpy()
    need = lambda P, rv, _=0: hip.contour_simplify_workspace_bytes(P, rv)
    for cap in (max(need(2, int(nv[p] + nv[p + 1])) for p in range(5)), 1):
        monkeypatch.setattr(maskpost, "RLE_WS_CAP", cap)
        n_rounds = len(maskpost.contour_rounds(nv, 0, cap, need))
        assert 2 <= n_rounds < 6 if cap > 1 else n_rounds == 6
        part = cas.simplify_contours(mc, tolerance=tol)
        part.check()
        for name in ("xy", "ring_start", "vertex_offsets", "n_vertices", "n_rings", "n_dropped"):
            assert torch.equal(getattr(part, name), getattr(whole, name)), name
    monkeypatch.undo()
    same = cas.simplify_contours(mc, tolerance=0)                     # the identity
    same.check()
    assert torch.equal(same.xy, mc.xy) and torch.equal(same.vertex_offsets, mc.vertex_offsets) and int(same.n_dropped.sum()) == 0
    assert torch.equal(same.ring_start.ne(0), mc.ring_start.ne(0)) and torch.equal(same.n_rings, mc.n_rings)
    marks = same.ring_start[same.ring_start.ne(0)]
    assert int(marks.eq(1).sum()) == int(mc.n_rings[:, 0].sum()) and int(marks.eq(2).sum()) == int(mc.n_rings[:, 1].sum())
    other = dropin.simplify_contours(mc, tolerance=tol)
    assert torch.equal(other.xy, whole.xy) and torch.equal(other.ring_start, whole.ring_start) and torch.equal(other.n_rings, whole.n_rings)
    coco = whole.to_coco()
    assert [len(d["polygons"]) for d in coco] == whole.n_rings.sum(1).tolist()
    decoded = cas.polygons_decode([d for d in coco if d["polygons"]], stats=False)               # the rasteriser takes them
    decoded.check()


def test_a_refused_input_is_passed_through(cas):
    """A MaskContours whose status is set and whose refused plane holds zeros: that plane comes out empty, the others whole, the
    output's status set."""
    from camouflaged_vlm_amd.engine import MaskContours
    planes = CO.ragged_planes(seed=34)[1:5]
    mc = cas.mask_contours_sized(sized_of(cas, planes))
    a, b = mc.vertex_offsets[1:3].tolist()
    xy, start = mc.xy.clone(), mc.ring_start.clone()
    xy[a:b] = 0
    start[a:b] = 0
    n_rings = mc.n_rings.clone()
    n_rings[1] = 0
    spoiled = MaskContours(**{**mc.__dict__, "xy": xy, "ring_start": start, "n_rings": n_rings, "status": torch.ones_like(mc.status)})
    out = cas.simplify_contours(spoiled, tolerance=1.0)
    assert int(out.status.item()) != 0 and int(out.n_vertices[1]) == 0 and out.n_rings[1].tolist() == [0, 0] and int(out.n_dropped[1]) == 0
    with pytest.raises(RuntimeError, match="simplify_contours"):
        out.check()
    good = cas.simplify_contours(mc, tolerance=1.0)
    good.check()
    vo, go = out.vertex_offsets.tolist(), good.vertex_offsets.tolist()
    for p in (0, 2, 3):
        assert torch.equal(out.xy[vo[p]:vo[p + 1]], good.xy[go[p]:go[p + 1]]), p


def test_end_to_end_on_the_tiny_cascade(tiny, cas, tracer, monkeypatch):
    """infer_classes(sizes=) -> mask_contours_sized -> simplify_contours: the polygons are the definition's on the call's own sized bits;
    the launches of infer_classes are the same with and without the two calls behind it."""
    _, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    sizes = [(53, 80), (120, 161)]
    names = lambda log: [e if isinstance(e, str) else e[0] for e in log]
    cas.infer_classes(inp, ci, cm, classes=torch.tensor(CLASSES), masks="bits", sizes=sizes)       # what a first call sets up is set up
    with tracer.Recorder() as log:
        cas.infer_classes(inp, ci, cm, classes=torch.tensor(CLASSES), masks="bits", sizes=sizes)
        torch.cuda.synchronize()
    alone = names(log)
    with tracer.Recorder() as log:
        h = cas.infer_classes(inp, ci, cm, classes=torch.tensor(CLASSES), masks="bits", sizes=sizes)
        mc = cas.mask_contours_sized(h.sized)
        mp = cas.simplify_contours(mc, tolerance=1.5)
        torch.cuda.synchronize()
    both = names(log)
    assert not any("simplify" in n for n in alone)
    assert both[:len(alone)] == alone
    assert both[len(alone):] == ["mask_contour_count", "mask_contour_emit", "contour_simplify_mark", "contour_simplify_emit"]
    mp.check()
    assert mp.sizes == h.sized.sizes and len(mp.sizes) == 6 and 0 < int(mp.n_vertices.sum()) == mp.xy.shape[0] < mc.xy.shape[0]
    rings = SO.rings_of_planes([h.sized.to_numpy(p) for p in range(6)], 8)
    check_polygons(mp, rings, [6] * 6)
    with tracer.Recorder() as log:
        for bad in (dict(tolerance=0.3), dict(tolerance=True), dict(tolerance=[1.0] * 5), dict(tolerance=16384), dict(contours=h.sized)):
            kw = dict(dict(contours=mc), **bad)
            with pytest.raises(ValueError, match="simplify_contours"):
                cas.simplify_contours(kw.pop("contours"), **kw)
    assert log == []
