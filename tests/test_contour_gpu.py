"""Contours of sized planes on the device: cvlm_mask_contour_count / cvlm_mask_contour_emit against the definition
(tests/contour_oracle.py) and against the host entry, vertex for vertex, on every width that crosses a word seam -- lattice column w
falls into a word of its own at w = 32 and 64 --, heights 1, 2 and 33, both connectivities, diagonal pairs and checkerboards, a chain
whose one ring of 1200 vertices passes every inner point twice, a comb whose ring exceeds one pass of the rank pass's workgroup and
whose vertical walks span the plane, a plane of hundreds of rings; ragged planes in one call and in three rounds, used outputs,
guard bands, dirty pad bits, an unaligned base and every refusal; the round trip through cvlm_mask_poly_decode on the device, the ring
counts against cvlm_mask_components and cvlm_mask_holes, and Cascade.mask_contours_sized and the drop-in on the tiny cascade."""
import numpy as np
import pytest
import torch

import contour_oracle as CO
import test_contour_cpu as CPU
from test_labels_gpu import tracer  # noqa: F401  (fixture)
from test_match_gpu import CLASSES, cas, dropin, gold, record_reads, tiny  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("h", CO.HEIGHTS)
def test_device_equals_the_oracle_and_the_host_entry(h, connectivity):
    """Every content at every width of one height; the planes of one width are ONE call."""
    for w in CO.WIDTHS:
        planes = [m for _, m in CO.contents(h, w, seed=1000 * h + w)]
        res = CO.run(planes, connectivity, dev=DEV)
        assert res["status"] == (0, 0)
        CO.check(res, planes, connectivity)
        CO.same(res, CO.run(planes, connectivity, host=True))


@pytest.mark.parametrize("connectivity", [4, 8])
def test_chain_comb_and_many_rings(connectivity):
    """Ranking and placement: rings longer than the workgroup, a ring that visits points twice, ring bases from the scan."""
    planes = [m for _, m in CO.big_cases()]
    res = CO.run(planes, connectivity, dev=DEV)
    assert res["status"] == (0, 0)
    CO.check(res, planes, connectivity)
    CO.same(res, CO.run(planes, connectivity, host=True))
    assert res["n_vertices"][0] == 1200 and tuple(res["n_rings"][0]) == ((1, 0) if connectivity == 8 else (300, 0))
    assert res["n_vertices"][1] > 1024 and tuple(res["n_rings"][1]) == (1, 0)
    assert res["n_rings"][2].sum() > 100


@pytest.mark.parametrize("connectivity", [4, 8])
def test_ragged_planes_rounds_used_outputs_dirty_pads_and_an_unaligned_base(connectivity):
    planes = CO.ragged_planes()
    res = CO.run(planes, connectivity, dev=DEV)
    assert res["status"] == (0, 0)
    CO.check(res, planes, connectivity)
    host = CO.run(planes, connectivity, host=True)
    CO.same(res, host)
    CO.same(CO.run(planes, connectivity, dev=DEV, rounds=3), host)                      # three emit calls through workspaces of their own size
    other = [~p for p in planes]
    fresh = CO.run(other, connectivity, dev=DEV)
    CO.check(fresh, other, connectivity)
    first, second = (res, other) if res["vertex_offsets"][-1] >= fresh["vertex_offsets"][-1] else (fresh, planes)
    used = CO.run(second, connectivity, dev=DEV, outs=first["outs"])                    # other planes into used outputs and a used workspace
    assert used["status"] == (0, 0)
    CO.check(used, second, connectivity)
    CO.same(CO.run(planes, connectivity, dev=DEV, shift=4, dirty_pads=True), host)      # bits 4 bytes off a 16-byte boundary, pad bits set


@pytest.mark.parametrize("name", [c[0] for c in CPU.refusals()[1]])
def test_refuses_whole_planes(name):
    sizes, cases = CPU.refusals()
    _, kw, refused, short, status = next(c for c in cases if c[0] == name)
    rng = np.random.default_rng(26)
    planes = [rng.random(s) < 0.7 for s in sizes]
    res = CO.run(planes, 8, dev=DEV, **kw)
    assert res["status"] == status
    CO.check(res, planes, 8, refused=refused, short=short)                              # the neighbours are whole
    CO.same(res, CO.run(planes, 8, host=True, **kw))
    whole = CO.run(planes, 8, dev=DEV)                                                  # the status is zeroed by every call
    assert whole["status"] == (0, 0)
    CO.check(whole, planes, 8)


def test_every_badarg_leaves_the_device_alone():
    CPU.test_every_badarg_of_the_contour_entries()
    torch.cuda.synchronize()


# ---- through the engine ---------------------------------------------------------------------------------------------------------------------------
def sized_of(cas, planes):
    """Bool planes as SizedMasks on the device, through polygons_decode's sibling rle_decode."""
    import rle_oracle as RO
    return cas.rle_decode([{"size": list(m.shape), "counts": RO.plane_counts(m).tolist()} for m in planes])


def xor_round_trip(cas, sized, contours) -> None:
    """polygons_decode of each ring as a plane of its own, the bytes XORed with torch, equal to the input bits."""
    coco = contours.to_coco()
    for p, d in enumerate(coco):
        lo, hi = sized.byte_range(p)
        want = sized.bits[lo:hi]
        polys = d["polygons"]
        assert all(3 <= len(q) // 2 <= 65535 for q in polys)
        acc = torch.zeros_like(want)
        for a in range(0, len(polys), 4096):
            part = cas.polygons_decode([{"size": d["size"], "polygons": [q]} for q in polys[a:a + 4096]], stats=False)
            part.check()
            for row in part.bits.view(-1, hi - lo):
                acc ^= row
        assert torch.equal(acc, want), p


@pytest.mark.parametrize("connectivity", [4, 8])
def test_round_trip_and_ring_counts_through_the_cascade(cas, dropin, connectivity, monkeypatch):
    """Random 64 x 64 planes: XOR of the rings' polygon planes is the mask; n_rings[:, 0] is cvlm_mask_components' count and
    n_rings[:, 1] cvlm_mask_holes' count at the SAME connectivity argument -- both take the foreground's connectivity, §15 connects
    clear pixels at its dual and calls a hole a clear region without a border pixel, which is a background component that the one
    clear frame of the definition does not reach.  One synchronisation: the read of n_vertices."""
    from camouflaged_vlm_amd.engine import MaskContours
    rng = np.random.default_rng(2603)
    planes = [rng.random((64, 64)) < d for d in (0.02, 0.3, 0.5, 0.7, 0.98)]
    ring = np.zeros((64, 64), dtype=bool)
    ring[8:56, 8:56] = True
    ring[16:48, 16:48] = False
    ring[24:40, 24:40] = True
    planes.append(ring)
    sized = sized_of(cas, planes)
    torch.cuda.synchronize()
    reads = record_reads(monkeypatch)
    mc = cas.mask_contours_sized(sized, connectivity=connectivity)
    monkeypatch.undo()
    assert reads.count("cpu") == 1 and "item" not in reads and "tolist" not in reads, reads
    assert isinstance(mc, MaskContours) and mc.connectivity == connectivity and mc.sizes == [(64, 64)] * 6
    mc.check()
    want = CO.run(planes, connectivity, host=True)
    assert torch.equal(mc.n_vertices.cpu(), torch.from_numpy(want["n_vertices"].astype(np.int32)))
    assert np.array_equal(mc.xy.cpu().numpy(), np.concatenate(want["xy"])) and np.array_equal(mc.n_rings.cpu().numpy(), want["n_rings"])
    assert mc.vertex_offsets.cpu().tolist() == want["vertex_offsets"].tolist()
    assert tuple(mc.n_rings[5].tolist()) == (2, 1)
    xor_round_trip(cas, sized, mc)
    rows = sized.bits.view(6, -1)
    comp = cas.mask_components(rows, 64, 64, components=0, connectivity=connectivity)
    holes = cas.mask_holes(rows, 64, 64, holes=0, connectivity=connectivity)
    assert torch.equal(mc.n_rings[:, 0], comp.n_comp.to(torch.int32)) and torch.equal(mc.n_rings[:, 1], holes.n_holes.to(torch.int32))
    areas = mc.signed_areas()
    assert [int(a.sum()) for a in areas] == [int(m.sum()) for m in planes]
    other = dropin.mask_contours_sized(sized, connectivity=connectivity)
    assert torch.equal(other.xy, mc.xy) and torch.equal(other.ring_start, mc.ring_start) and torch.equal(other.n_rings, mc.n_rings)


def test_rounds_under_the_workspace_cap_give_the_same_contours(cas, monkeypatch):
    """The engine's own rounds: a cap that holds two planes at a time, then one below a single plane's need."""
    from camouflaged_vlm_amd import hip, maskpost
    planes = CO.ragged_planes(seed=27) + [CO.chain(60)]
    sized = sized_of(cas, planes)
    whole = cas.mask_contours_sized(sized)
    nv = whole.n_vertices.cpu().numpy()
    max_words = max(h * ((w + 31) // 32) for h, w in sized.sizes)
    for cap in (max(hip.mask_contour_workspace_bytes(2, int(nv[p] + nv[p + 1]), max_words) for p in range(len(planes) - 1)), 1):
        monkeypatch.setattr(maskpost, "RLE_WS_CAP", cap)
        rounds = maskpost.contour_rounds(nv, max_words, cap, hip.mask_contour_workspace_bytes)
        assert 2 <= len(rounds) < len(planes) if cap > 1 else len(rounds) == len(planes)
        part = cas.mask_contours_sized(sized)
        part.check()
        assert torch.equal(part.xy, whole.xy) and torch.equal(part.ring_start, whole.ring_start) and torch.equal(part.n_rings, whole.n_rings)
    monkeypatch.undo()
    want = CO.run(planes, 8, host=True)
    assert np.array_equal(whole.xy.cpu().numpy(), np.concatenate(want["xy"]))


def test_end_to_end_on_the_tiny_cascade(tiny, cas, tracer, monkeypatch):
    """infer_classes(sizes=) -> mask_contours_sized -> to_coco -> polygons_decode gives the call's own sized bits back under the XOR
    rule; the launches of infer_classes are the same with and without the contour call behind it."""
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
        torch.cuda.synchronize()
    both = names(log)
    assert not any("contour" in n for n in alone)
    assert both[:len(alone)] == alone and both[len(alone):] == ["mask_contour_count", "mask_contour_emit"]
    mc.check()
    assert mc.sizes == h.sized.sizes and len(mc.sizes) == 6 and int(mc.n_vertices.sum()) == mc.xy.shape[0] > 0
    planes = [h.sized.to_numpy(p) for p in range(6)]
    CO.check(dict(n_vertices=mc.n_vertices.cpu().numpy(), n_rings=mc.n_rings.cpu().numpy(),
                  xy=[mc.xy[a:b].cpu().numpy() for a, b in zip(mc.vertex_offsets[:-1].tolist(), mc.vertex_offsets[1:].tolist())],
                  ring_start=[mc.ring_start[a:b].cpu().numpy() for a, b in zip(mc.vertex_offsets[:-1].tolist(), mc.vertex_offsets[1:].tolist())]),
             planes, 8)
    xor_round_trip(cas, h.sized, mc)
    with tracer.Recorder() as log:
        for bad in (dict(connectivity=6), dict(connectivity=True), dict(sized=h.sized.bits)):
            kw = dict(dict(sized=h.sized), **bad)
            with pytest.raises(ValueError, match="mask_contours_sized"):
                cas.mask_contours_sized(kw.pop("sized"), **kw)
    assert log == []
