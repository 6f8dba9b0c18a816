"""Distance maps and surface distances on the device: cvlm_mask_distance_sized against the definition
(tests/distance_oracle.py) and against the host entry, entry for entry, on widths 1 .. 129 x heights 1 .. 130, every pattern and reach
of the issue's list, the three planes that stress the passes, ragged planes in one call, used outputs, guard bands, dirty pad bits, an
unaligned base and every refusal; cvlm_mask_surface_totals against the plain loops at T = 1, 3, 8, its refusals, its empty sides and the
bit pattern and error bound of sum_d; Cascade.mask_distance_sized / mask_surface_distances and the drop-in on random planes, under caps
that force one round and several, at reach="tolerance", on §17's edge bits, and end to end on the tiny cascade.  Every comparison of
integers is exact."""
import math

import numpy as np
import pytest
import torch

import distance_oracle as DO
import test_distance_cpu as CPU
from test_contour_gpu import sized_of
from test_labels_gpu import tracer  # noqa: F401  (fixture)
from test_match_gpu import CLASSES, cas, dropin, gold, record_reads, tiny  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def entries():
    from camouflaged_vlm_amd import hip
    return hip.mask_distance_sized, hip.mask_surface_totals


# ---- the distance kernels -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", DO.HEIGHTS)
def test_device_equals_the_oracle_and_the_host_entry(h):
    """Every width, pattern and reach of one height in ONE call."""
    planes, reaches, which, want = CPU.gpu_list()
    pick = [i for i, p in enumerate(planes) if p.shape[0] == h]
    assert len(pick) == len(DO.WIDTHS) * 14 * 5
    planes, reaches, want = [planes[i] for i in pick], [reaches[i] for i in pick], [want[which[i]] for i in pick]
    res = DO.run_distance(entries()[0], planes, reaches, dev=DEV)
    assert res["status"] == 0
    DO.check_distance(res, planes, reaches, want=want)
    host = DO.run_distance(CPU.host_entries()[0], planes, reaches)
    assert all(np.array_equal(a, b) for a, b in zip(res["maps"], host["maps"]))


def test_the_planes_that_stress_the_passes():
    """The whole column searched from one corner pixel; D2 up to 16383^2 + 1 through the uint16 row distance (against the scipy form);
    rows without a set pixel in the middle of a search -- each unlimited and at reach 7, all in one call."""
    pytest.importorskip("scipy.ndimage")
    planes = [p for _, p in DO.stress_planes() for _ in range(2)]
    reaches = [0, 7] * 3
    want = [DO.edt(p) for p in planes]
    res = DO.run_distance(entries()[0], planes, reaches, dev=DEV)
    assert res["status"] == 0
    DO.check_distance(res, planes, reaches, want=want)
    assert res["maps"][0].max() == 178802 and res["maps"][2].max() == 16383 ** 2 + 1 and res["maps"][2][0, 16383] == 16383 ** 2
    assert (res["maps"][3][:, 8:] == DO.FAR).all() and res["maps"][3][1, 6] == 37 and res["maps"][3][1, 7] == DO.FAR


def test_ragged_planes_used_outputs_dirty_pads_and_an_unaligned_base():
    fn = entries()[0]
    planes, reaches = CPU.ragged_planes(), [0, 3, 0, 1, 0, 0, 5]
    res = DO.run_distance(fn, planes, reaches, dev=DEV)
    assert res["status"] == 0
    DO.check_distance(res, planes, reaches)
    other = [~p for p in planes]
    used = DO.run_distance(fn, other, reaches[::-1], dev=DEV, outs=res["outs"])        # other planes into used outputs and a used workspace
    assert used["status"] == 0
    DO.check_distance(used, other, reaches[::-1])
    dirty = DO.run_distance(fn, planes, reaches, dev=DEV, shift=4, dirty_pads=True)     # bits 4 bytes off a 16-byte boundary, pad bits set
    assert dirty["status"] == 0
    DO.check_distance(dirty, planes, reaches)


@pytest.mark.parametrize("name", [c[0] for c in CPU.refusals()])
def test_refuses_whole_planes(name):
    _, kw, reaches, refused, untouched = next(c for c in CPU.refusals() if c[0] == name)
    rng = np.random.default_rng(31)
    planes = [rng.random(s) < 0.1 for s in CPU.REFUSAL_SIZES]
    res = DO.run_distance(entries()[0], planes, reaches, dev=DEV, **kw)
    assert res["status"] == 1
    DO.check_distance(res, planes, reaches, refused=refused, untouched=untouched)       # the neighbours are whole
    whole = DO.run_distance(entries()[0], planes, [0, 0, 0], dev=DEV, outs=res["outs"])  # the status is zeroed by every call
    assert whole["status"] == 0
    DO.check_distance(whole, planes, [0, 0, 0])


def test_every_badarg_leaves_the_device_alone():
    CPU.test_every_badarg_of_the_distance_entry()
    CPU.test_every_badarg_of_the_totals_entry()
    torch.cuda.synchronize()


# ---- the totals -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 3, 8])
def test_totals_equal_the_plain_loops_and_the_host_entry(T):
    """Random pairs of three sizes at radii 0, 1, 7 and 23170 (and four more at T = 8), with empty A, empty B and both empty among
    them, against unlimited maps and maps cut at reach 7."""
    a, b, pairs, radii = CPU.totals_cases()
    for reach in (0, 7):
        maps = [DO.d2_of(m, reach) for m in b]
        res = DO.run_totals(entries()[1], a, maps, pairs, radii[T], dev=DEV)
        assert res["status"] == 0
        DO.check_totals(res, a, maps, pairs, radii[T])
        host = DO.run_totals(CPU.host_entries()[1], a, maps, pairs, radii[T])
        for k in ("n", "far", "within", "max_d2", "sum_d2"):
            assert np.array_equal(res[k], host[k]), k
    empties = [i for i, (p, q) in enumerate(pairs) if not a[p].any() or not b[q].any()]
    assert len(empties) >= 6 and (res["max_d2"][[i for i in empties if not a[pairs[i][0]].any()]] == -1).all()


@pytest.mark.parametrize("name", [c[0] for c in CPU.totals_refusals()])
def test_totals_refuse_whole_pairs(name):
    _, kw, pairs, radii, refused = next(c for c in CPU.totals_refusals() if c[0] == name)
    a, b, _, _ = CPU.totals_cases()
    maps = [DO.d2_of(m) for m in b]
    res = DO.run_totals(entries()[1], a, maps, pairs, radii, dev=DEV, **kw)
    assert res["status"] == 1
    DO.check_totals(res, a, maps, pairs, radii, refused=refused)                        # the sound pairs are whole
    good = [i for i in range(len(pairs)) if i not in refused]
    again = DO.run_totals(entries()[1], a, maps, [pairs[i] for i in good], [radii[i] for i in good], dev=DEV)
    assert again["status"] == 0                                                         # the status is zeroed by every call


def test_sum_d_is_deterministic_and_within_its_bound():
    """300 x 300, about 45 000 pixels of A over several workgroups: the same bit pattern from two calls into fresh outputs and from a
    call into used ones; within n * 2^-52 * fsum of the oracle's fsum (distance_oracle.sum_d_bound: n <= 10^5)."""
    rng = np.random.default_rng(33)
    a, b = [rng.random((300, 300)) < 0.5], [rng.random((300, 300)) < 0.0005]
    maps = [DO.edt(b[0])]
    first = DO.run_totals(entries()[1], a, maps, [(0, 0)], [[0, 7, 40]], dev=DEV)
    second = DO.run_totals(entries()[1], a, maps, [(0, 0)], [[0, 7, 40]], dev=DEV)
    third = DO.run_totals(entries()[1], a, maps, [(0, 0)], [[0, 7, 40]], dev=DEV, outs=first["outs"])
    assert first["sum_d"].tobytes() == second["sum_d"].tobytes() == third["sum_d"].tobytes()
    want = DO.totals(a[0], maps[0], [0, 7, 40])
    assert 40000 < want["n"] <= 10 ** 5 and want["sum_d"] > 0
    print("sum_d", float(first["sum_d"][0]), "fsum", want["sum_d"], "bound", DO.sum_d_bound(want))
    DO.check_totals(first, a, maps, [(0, 0)], [[0, 7, 40]])


# ---- through the engine ---------------------------------------------------------------------------------------------------------------------------
def engine_planes(seed: int = 34):
    """Predictions and annotations of three sizes: blobs with a displaced copy, an empty prediction, an empty annotation, both empty."""
    rng = np.random.default_rng(seed)
    sizes = [(70, 33), (70, 33), (97, 131), (97, 131), (33, 31), (33, 31), (33, 31)]
    yy = lambda s: np.mgrid[0:s[0], 0:s[1]]
    blob = lambda s, cy, cx, r: (yy(s)[0] - cy) ** 2 + (yy(s)[1] - cx) ** 2 <= r * r
    a = [blob(sizes[0], 30, 16, 12), blob(sizes[1], 40, 10, 9) | (rng.random(sizes[1]) < 0.01), blob(sizes[2], 50, 60, 40),
         rng.random(sizes[3]) < 0.5, np.zeros(sizes[4], dtype=bool), blob(sizes[5], 16, 15, 8), np.zeros(sizes[6], dtype=bool)]
    b = [blob(sizes[0], 33, 16, 12), blob(sizes[1], 40, 20, 9), blob(sizes[2], 47, 66, 35), blob(sizes[3], 50, 60, 30),
         blob(sizes[4], 16, 15, 8), np.zeros(sizes[5], dtype=bool), np.zeros(sizes[6], dtype=bool)]
    return a, b


def oracle_totals(a, b, pairs, radii, reach_of=lambda p, q: 0, surface=True):
    sa = [DO.surface(m) for m in a] if surface else a
    sb = [DO.surface(m) for m in b] if surface else b
    ab = [DO.totals(sa[p], DO.d2_of(sb[q], reach_of(p, q)), r) for (p, q), r in zip(pairs, radii)]
    ba = [DO.totals(sb[q], DO.d2_of(sa[p], reach_of(p, q)), r) for (p, q), r in zip(pairs, radii)]
    return ab, ba


def check_engine(host, ab, ba, only=None):
    for side, want in (("ab", ab), ("ba", ba)):
        for i, t in enumerate(want):
            for k in ("n", "far", "within", "max_d2", "sum_d2") if only is None else only:
                assert np.asarray(host[side][k][i]).tolist() == t[k], (side, i, k, host[side][k][i], t[k])
            if only is None:
                assert abs(float(host[side]["sum_d"][i]) - t["sum_d"]) <= DO.sum_d_bound(t), (side, i)


def test_surface_distances_through_cascade_and_dropin_in_one_round_and_in_several(cas, dropin, monkeypatch):
    from camouflaged_vlm_amd import engine, maskpost, surfeval
    a, b = engine_planes()
    sa, sb = sized_of(cas, a), sized_of(cas, b)
    pairs = [(p, p) for p in range(7)] + [(0, 1), (1, 0), (5, 4), (2, 3)]
    torch.cuda.synchronize()
    reads = record_reads(monkeypatch)
    st = cas.mask_surface_distances(sa, sb, pairs=pairs, tolerance=[0.008, 2, 0])
    monkeypatch.undo()
    assert reads == [], reads                                                           # no synchronisation
    assert isinstance(st, engine.SurfaceTotals)
    st.check()
    host = st.to_host()
    radii = [[DO.surface_tolerance(*a[p].shape), 2, 0] for p, _ in pairs]
    assert host["radii"].tolist() == radii and host["pairs"].tolist() == [list(p) for p in pairs] and host["status"] == 0
    ab, ba = oracle_totals(a, b, pairs, radii)
    check_engine(host, ab, ba)
    got = surfeval.surface_metrics(host)
    for i in range(len(pairs)):
        want = DO.metrics(ab[i], ba[i])
        assert got["hausdorff"][i] == want["hausdorff"] and got["nsd"][i].tolist() == want["nsd"] and got["f"][i].tolist() == want["f"], i
        assert got["precision"][i].tolist() == want["precision"] and got["recall"][i].tolist() == want["recall"], i
        assert got["assd"][i] == want["assd"] or abs(got["assd"][i] - want["assd"]) <= 2.0 ** -40 * want["assd"], i
    assert got["hausdorff"][6] == 0.0 and got["hausdorff"][4] == got["hausdorff"][5] == math.inf and got["f"][6].tolist() == [1.0, 1.0, 1.0]
    # caps: one that holds three small maps a side, one below any map: several rounds, the same tables to the last bit
    for cap, n_rounds in ((6 * 70 * 33 * 2 + 6 * 33 * 31, None), (1, len(pairs))):
        monkeypatch.setattr(maskpost, "RLE_WS_CAP", cap)
        rounds = engine.surface_rounds(np.asarray(pairs), sa.sizes, sb.sizes, cap)
        assert 1 < len(rounds) < len(pairs) if n_rounds is None else len(rounds) == n_rounds
        part = cas.mask_surface_distances(sa, sb, pairs=pairs, tolerance=[0.008, 2, 0])
        part.check()
        for side in ("ab", "ba"):
            for k in maskpost.SURFACE_TABLES:
                assert torch.equal(getattr(part, side)[k], getattr(st, side)[k]), (cap, side, k)
    monkeypatch.undo()
    other = dropin.mask_surface_distances(sa, sb, pairs=pairs, tolerance=[0.008, 2, 0])
    assert all(torch.equal(other.ab[k], st.ab[k]) and torch.equal(other.ba[k], st.ba[k]) for k in maskpost.SURFACE_TABLES)


def test_reach_tolerance_keeps_the_counts(cas):
    """reach="tolerance": `within` and `n` equal the unlimited call's; what lies beyond the largest radius is far."""
    a, b = engine_planes(35)
    sa, sb = sized_of(cas, a), sized_of(cas, b)
    pairs = [(p, p) for p in range(7)]
    whole = cas.mask_surface_distances(sa, sb, pairs=pairs, tolerance=[1, 0.02]).to_host()
    near = cas.mask_surface_distances(sa, sb, pairs=pairs, tolerance=[1, 0.02], reach="tolerance").to_host()
    assert near["status"] == 0
    for side in ("ab", "ba"):
        assert np.array_equal(near[side]["within"], whole[side]["within"]) and np.array_equal(near[side]["n"], whole[side]["n"])
        assert (near[side]["far"] == near[side]["n"] - near[side]["within"].max(axis=1)).all() and near[side]["far"].sum() > 0
    radii = near["radii"].tolist()
    ab, ba = oracle_totals(a, b, pairs, radii, reach_of=lambda p, q: max(1, max(radii[p])))
    check_engine(near, ab, ba)


def test_a_square_against_itself_shifted_by_three(cas):
    from camouflaged_vlm_amd import surfeval
    sq, moved = np.zeros((100, 100), dtype=bool), np.zeros((100, 100), dtype=bool)
    sq[20:80, 20:80] = True
    moved[20:80, 23:83] = True
    m = surfeval.surface_metrics(cas.mask_surface_distances(sized_of(cas, [sq]), sized_of(cas, [moved]), tolerance=[2, 3]).to_host())
    assert m["hausdorff"][0] == 3.0 and m["nsd"][0, 0] < 1.0 and m["nsd"][0, 1] == 1.0 and m["f"][0, 1] == 1.0 and 0.0 < m["assd"][0] < 3.0


def test_distance_maps_through_cascade_and_dropin(cas, dropin, monkeypatch):
    from camouflaged_vlm_amd import engine
    planes = CPU.ragged_planes(36)
    sized = sized_of(cas, planes)
    torch.cuda.synchronize()
    reads = record_reads(monkeypatch)
    md = cas.mask_distance_sized(sized)
    cut = cas.mask_distance_sized(sized, reach=[0, 3, 0, 1, 0, 0, 5])
    monkeypatch.undo()
    assert reads == [], reads
    assert isinstance(md, engine.MaskDistances) and md.sizes == [tuple(p.shape) for p in planes] and md.d2.dtype == torch.int32
    md.check()
    cut.check()
    for p, plane in enumerate(planes):
        want = DO.d2_of(plane)
        assert np.array_equal(md.plane(p).cpu().numpy(), want), p
        assert np.array_equal(cut.plane(p).cpu().numpy(), DO.with_reach(want, int(cut.reach[p]))), p
        dist = md.distance(p).cpu().numpy()
        assert dist.dtype == np.float32 and dist.shape == plane.shape
        assert np.array_equal(dist, np.where(want == DO.FAR, np.inf, np.sqrt(want.astype(np.float32))).astype(np.float32)), p
    assert np.isinf(md.distance(6).cpu().numpy()).all() and md.pix_offsets.cpu().tolist() == np.cumsum([0] + [p.size for p in planes]).tolist()
    other = dropin.mask_distance_sized(sized, reach=[0, 3, 0, 1, 0, 0, 5])
    assert torch.equal(other.d2, cut.d2)


def test_edge_bits_score_as_surfaces_of_their_own(cas):
    """surface=None on §17's packed edge maps wrapped as sized planes: the edge pixels themselves against each other."""
    from camouflaged_vlm_amd import engine
    g = torch.Generator().manual_seed(37)
    smooth = torch.nn.functional.avg_pool2d(torch.rand(3, 1, 72, 72, generator=g), 9, stride=1)          # (3, 1, 64, 64)
    prob = (smooth - smooth.amin()) / (smooth.amax() - smooth.amin())
    prob = prob.to(DEV)

    def wrap(eb):
        n = eb.bits.shape[0]
        off = torch.arange(n + 1, dtype=torch.int64, device=DEV) * eb.bits.shape[1]
        return engine.SizedMasks(bits=eb.bits.reshape(-1), offsets=off, area=eb.area, box=None,
                                 status=torch.zeros(1, dtype=torch.int32, device=DEV), sizes=[(64, 64)] * n, level=0)

    pred, truth = wrap(cas.pack_edges(prob, threshold=0.6)), wrap(cas.pack_edges(prob, threshold=0.7))
    st = cas.mask_surface_distances(pred, truth, tolerance=[1, 3], surface=None)
    st.check()
    a, b = [pred.to_numpy(p) for p in range(3)], [truth.to_numpy(p) for p in range(3)]
    assert any(m.any() for m in a) and any(m.any() for m in b)
    pairs = [(p, p) for p in range(3)]
    ab, ba = oracle_totals(a, b, pairs, [[1, 3]] * 3, surface=False)
    host = st.to_host()
    check_engine(host, ab, ba)
    assert host["ab"]["n"].tolist() == [int(m.sum()) for m in a]                         # the planes as given, not their boundaries


def test_end_to_end_on_the_tiny_cascade(tiny, cas, tracer, monkeypatch):
    """The surfaces of the call's own masks against annotations made from the call's own encoding: Hausdorff 0, NSD 1, F 1; against one
    annotation eroded by one pixel: the oracle's values; the launches of infer_classes are the same with and without the call."""
    import boundary_oracle as BO
    import rle_oracle as RO
    from camouflaged_vlm_amd import surfeval
    _, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    sizes = [(53, 80), (120, 161)]
    names = lambda log: [e if isinstance(e, str) else e[0] for e in log]
    run = lambda: cas.infer_classes(inp, ci, cm, classes=torch.tensor(CLASSES), masks="bits", sizes=sizes, rle="sized")
    h = run()                                                         # what a first call sets up is set up
    gts = cas.rle_decode(h.rle.to_coco())
    with tracer.Recorder() as log:
        run()
        torch.cuda.synchronize()
    alone = names(log)
    with tracer.Recorder() as log:
        h = run()
        st = cas.mask_surface_distances(h.sized, gts)
        torch.cuda.synchronize()
    both = names(log)
    assert not any("distance" in n or "surface" in n for n in alone)
    assert both[:len(alone)] == alone
    assert both[len(alone):] == ["mask_boundary_sized"] * 2 + ["mask_distance_sized", "mask_surface_totals"] * 2
    st.check()
    m = surfeval.surface_metrics(st.to_host())
    assert (m["hausdorff"] == 0.0).all() and (m["assd"] == 0.0).all() and (m["nsd"] == 1.0).all() and (m["f"] == 1.0).all()
    planes = [h.sized.to_numpy(p) for p in range(6)]
    p = max(range(6), key=lambda q: int(planes[q].sum()))
    assert planes[p].sum() > 9
    worn = list(planes)
    worn[p] = BO.erode(planes[p], 1)
    gts = cas.rle_decode([{"size": list(x.shape), "counts": RO.plane_counts(x).tolist()} for x in worn])
    host = cas.mask_surface_distances(h.sized, gts, tolerance=[0.008, 1, 0]).to_host()
    radii = host["radii"].tolist()
    assert radii == [[DO.surface_tolerance(*x.shape), 1, 0] for x in planes] and host["status"] == 0
    ab, ba = oracle_totals(planes, worn, [(q, q) for q in range(6)], radii)
    check_engine(host, ab, ba)
    got, want = surfeval.surface_metrics(host), DO.metrics(ab[p], ba[p])
    assert got["hausdorff"][p] == want["hausdorff"] and got["nsd"][p].tolist() == want["nsd"] and got["f"][p].tolist() == want["f"]
    if worn[p].any():
        assert got["hausdorff"][p] >= 1.0 and got["nsd"][p, 2] < 1.0     # thin parts vanish under the erosion: the distance has no upper bound
    with tracer.Recorder() as log:
        for bad in (dict(tolerance=True), dict(surface="seg2bmap"), dict(reach="far"), dict(pairs=[(0, 3)]), dict(tolerance=[1] * 9)):
            with pytest.raises(ValueError, match="mask_surface_distances"):
                cas.mask_surface_distances(h.sized, gts, **bad)
        with pytest.raises(ValueError, match="mask_distance_sized"):
            cas.mask_distance_sized(h.sized, reach=-1)
    assert log == []
