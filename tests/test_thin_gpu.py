"""Thinning of sized planes on the device: cvlm_mask_thin_sized against the definition (tests/thin_oracle.py) and against
the host entry, under mode 0 (the resident kernel) and mode 1 (the stepping kernels), on widths 1 .. 129 x heights 1 .. 130 and every
pattern of the issue's list with max_iter 1, 2 and unlimited mixed, the stepping path at steps = 1, 3 and 64, the full 200 x 300 plane,
one plane on either side of the resident budget, ragged planes in one call, used outputs, guard bands, dirty pad bits, an unaligned
base and every refusal; Cascade.mask_thin_sized's rounds, §17's edge bits, Cascade.mask_cldice and the drop-in, end to end on the tiny
cascade.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import test_thin_cpu as CPU
import thin_oracle as TO
from test_contour_gpu import sized_of
from test_labels_gpu import tracer  # noqa: F401  (fixture)
from test_match_gpu import CLASSES, cas, dropin, gold, record_reads, tiny  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = (0, 1)


def entry():
    from camouflaged_vlm_amd import hip
    return hip.mask_thin_sized


_CACHE = {}


def budget_planes():
    """1024 columns, random at 0.5: the tallest plane that is resident and the first that is not, with the oracle's answers."""
    if "budget" not in _CACHE:
        rng = np.random.default_rng(51)
        h = TO.LDS_BUDGET // (4 * 34) - 2
        planes = [rng.random((h, 1024)) < 0.5, rng.random((h + 1, 1024)) < 0.5]
        _CACHE["budget"] = (planes, [TO.thin(p) for p in planes])
    return _CACHE["budget"]


# ---- the entry ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_device_equals_the_oracle_and_the_host_entry(mode):
    """Every width, height, pattern and max_iter in ONE call per mode; the list's slowest plane takes 64 iterations."""
    planes, limits, want = CPU.gpu_list()
    assert max(n for _, n in want) < 80
    res = TO.run(entry(), planes, limits, dev=DEV, mode=mode, steps=80)
    assert res["status"] == 0
    TO.check(res, planes, limits, want=want)
    host = TO.run(CPU.host_entry(), planes, limits)
    assert all(np.array_equal(a, b) for a, b in zip(res["raw"], host["raw"]))
    for k in ("area", "box", "iters", "done"):
        assert np.array_equal(res[k], host[k]), k
    bare = TO.run(entry(), planes[:70], limits[:70], dev=DEV, mode=mode, steps=80, stats=False)      # without areas and boxes
    TO.check(bare, planes[:70], limits[:70], want=want[:70], stats=False)


def test_the_stepping_path_runs_out_of_steps_and_resumes():
    """A 33 x 65 plane at 0.9 that needs more than 3 iterations, beside one that needs 1 and one limited to 2: done is 0 while steps
    run out and 1 once they do not; the state after k steps is the oracle's after k iterations."""
    rng = np.random.default_rng(52)
    planes = [rng.random((33, 65)) < 0.9, np.ones((3, 3), dtype=bool), rng.random((33, 65)) < 0.9]
    limits = [0, 0, 2]
    need = TO.thin(planes[0])[1]
    assert 3 < need < 64
    for steps, done in ((1, [0, 0, 0]), (3, [0, 1, 1]), (64, [1, 1, 1])):
        res = TO.run(entry(), planes, limits, dev=DEV, mode=1, steps=steps)
        assert res["status"] == 0
        cut = [min(steps, m) if m else steps for m in limits]
        TO.check(res, planes, cut, done=done)
    assert res["iters"].tolist() == [need, 1, 2]
    part = TO.run(entry(), planes, limits, dev=DEV, mode=1, steps=3)
    rest = TO.run(entry(), part["planes"], [0, 0, 0], dev=DEV, mode=1, steps=64)          # the output fed back as the input
    assert all(np.array_equal(a, b) for a, b in zip(rest["planes"][:2], res["planes"][:2]))
    assert (part["iters"] + rest["iters"]).tolist()[:2] == [need, 1]


@pytest.mark.parametrize("mode", MODES)
def test_the_full_200_by_300_plane(mode):
    planes = [np.ones((200, 300), dtype=bool)]
    res = TO.run(entry(), planes, [0], dev=DEV, mode=mode, steps=128)
    assert res["status"] == 0 and res["area"].tolist() == [101] and res["iters"].tolist() == [100] and res["done"].tolist() == [1]
    TO.check(res, planes, [0])


@pytest.mark.parametrize("mode", MODES)
def test_either_side_of_the_resident_budget(mode):
    """Under mode 0 the first plane is thinned by the resident kernel at its largest and the second by the stepping kernels."""
    from camouflaged_vlm_amd import hip
    planes, want = budget_planes()
    assert hip.mask_thin_resident(*planes[0].shape) and not hip.mask_thin_resident(*planes[1].shape)
    assert max(n for _, n in want) < 32
    res = TO.run(entry(), planes, [0, 0], dev=DEV, mode=mode, steps=32)
    assert res["status"] == 0
    TO.check(res, planes, [0, 0], want=want)
    if mode == 0:
        host = TO.run(CPU.host_entry(), planes, [0, 0])
        assert all(np.array_equal(a, b) for a, b in zip(res["raw"], host["raw"]))


@pytest.mark.parametrize("mode", MODES)
def test_ragged_planes_used_outputs_dirty_pads_an_unaligned_base_and_three_calls(mode):
    fn = entry()
    planes, limits = CPU.ragged_planes(), [0, 1, 0, 2, 0, 0, 1]
    res = TO.run(fn, planes, limits, dev=DEV, mode=mode)
    assert res["status"] == 0
    TO.check(res, planes, limits)
    for _ in range(2):                                                                    # the same bits from three calls
        again = TO.run(fn, planes, limits, dev=DEV, mode=mode)
        assert all(np.array_equal(a, b) for a, b in zip(again["raw"], res["raw"])) and np.array_equal(again["iters"], res["iters"])
    other = [~p for p in planes]
    used = TO.run(fn, other, limits[::-1], dev=DEV, mode=mode, outs=res["outs"])          # other planes into used outputs and a used workspace
    assert used["status"] == 0
    TO.check(used, other, limits[::-1])
    dirty = TO.run(fn, planes, limits, dev=DEV, mode=mode, shift=4, dirty_pads=True)      # bits 4 bytes off a 16-byte boundary, pad bits set
    assert dirty["status"] == 0
    TO.check(dirty, planes, limits)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [c[0] for c in CPU.refusals()])
def test_refuses_whole_planes(name, mode):
    _, kw, limits, refused, untouched = next(c for c in CPU.refusals() if c[0] == name)
    rng = np.random.default_rng(45)
    planes = [rng.random(s) < 0.8 for s in CPU.REFUSAL_SIZES]
    res = TO.run(entry(), planes, limits, dev=DEV, mode=mode, **kw)
    assert res["status"] == 1
    TO.check(res, planes, limits, refused=refused, untouched=untouched)                   # the neighbours are whole
    whole = TO.run(entry(), planes, [0, 0, 0], dev=DEV, mode=mode, outs=res["outs"])      # the status is zeroed by every call
    assert whole["status"] == 0
    TO.check(whole, planes, [0, 0, 0])


def test_a_plane_that_is_not_resident_is_refused_without_steps():
    """steps = 0 is a call of resident planes; the host cannot see the sizes, so the kernel refuses what would need the other path."""
    tall = np.ones((TO.LDS_BUDGET // 12, 7), dtype=bool)                                  # one word column: 3 words per row with its border
    assert TO.lds_bytes(*tall.shape) > TO.LDS_BUDGET
    res = TO.run(entry(), [np.ones((4, 6), dtype=bool), tall, np.ones((3, 3), dtype=bool)], [0, 0, 0], dev=DEV, mode=0, steps=0)
    assert res["status"] == 1 and res["area"].tolist() == [3, 0, 1] and res["done"].tolist() == [1, 0, 1] and (res["raw"][1] == 0).all()


def test_every_badarg_leaves_the_device_alone():
    CPU.test_every_badarg_of_the_thin_entry()
    torch.cuda.synchronize()


# ---- through the engine ---------------------------------------------------------------------------------------------------------------------------
def test_resident_planes_through_cascade_and_dropin_without_a_synchronisation(cas, dropin, monkeypatch):
    from camouflaged_vlm_amd import engine
    planes = CPU.ragged_planes(53) + [np.ones((64, 64), dtype=bool)]
    sized = sized_of(cas, planes)
    torch.cuda.synchronize()
    reads = record_reads(monkeypatch)
    mt = cas.mask_thin_sized(sized)
    cut = cas.mask_thin_sized(sized, max_iter=[1, 2, 1, 3, 1, 1, 2, 5])
    monkeypatch.undo()
    assert reads == [], reads                                                             # no synchronisation
    assert isinstance(mt, engine.MaskThin) and isinstance(mt.masks, engine.SizedMasks)
    assert mt.masks.sizes == [tuple(p.shape) for p in planes] and mt.masks.offsets is sized.offsets and mt.masks.level == sized.level
    mt.check()
    cut.check()
    for res, limits in ((mt, [0] * 8), (cut, [1, 2, 1, 3, 1, 1, 2, 5])):
        for p, plane in enumerate(planes):
            want, n = TO.thin(plane, limits[p])
            assert np.array_equal(res.masks.to_numpy(p), want), p
            assert int(res.iters[p]) == n and int(res.done[p]) == 1 and int(res.masks.area[p]) == int(want.sum()), p
            assert res.masks.box[p].tolist() == TO.box_of(want), p
    assert int(mt.iters[7]) == 32 and int(cut.iters[7]) == 5
    other = dropin.mask_thin_sized(sized, max_iter=[1, 2, 1, 3, 1, 1, 2, 5])
    assert torch.equal(other.masks.bits, cut.masks.bits) and torch.equal(other.iters, cut.iters)


@pytest.mark.parametrize("steps", [1, 3, 64])
def test_rounds_of_stepped_planes_equal_the_one_call_to_the_last_bit(cas, monkeypatch, steps):
    """path="steps" at steps = 1, 3 and 64 on planes of which one needs more than 3 iterations: one read per round, and the same bits,
    areas, boxes and iteration counts as the resident kernel gives in one call."""
    rng = np.random.default_rng(54)
    planes = [rng.random((33, 65)) < 0.9, np.ones((4, 6), dtype=bool), np.zeros((5, 40), dtype=bool), rng.random((70, 33)) < 0.7]
    limits = [None, [2, 1, 1, 3]]
    sized = sized_of(cas, planes)
    for max_iter in limits:
        one = cas.mask_thin_sized(sized, max_iter=max_iter)
        torch.cuda.synchronize()
        reads = record_reads(monkeypatch)
        got = cas.mask_thin_sized(sized, max_iter=max_iter, path="steps", steps=steps)
        monkeypatch.undo()
        got.check()
        most = int(one.iters.max())
        assert 3 < most < 64 or max_iter is not None
        rounds = reads.count("cpu")
        assert rounds == (most // steps + 1 if max_iter is None else -(-most // steps)), (reads, most)
        assert torch.equal(got.masks.bits, one.masks.bits) and torch.equal(got.iters, one.iters) and torch.equal(got.masks.area, one.masks.area)
        assert torch.equal(got.masks.box, one.masks.box) and got.done.tolist() == [1] * 4
        for p, plane in enumerate(planes):
            want, n = TO.thin(plane, 0 if max_iter is None else max_iter[p])
            assert np.array_equal(got.masks.to_numpy(p), want) and int(got.iters[p]) == n, p


def test_resident_and_stepped_planes_in_one_call(cas):
    """path="auto" on the planes on either side of the budget and a small one: the large one goes through rounds of 2 iterations."""
    from camouflaged_vlm_amd import engine
    import boundary_oracle as BO
    big, want = budget_planes()
    planes = [np.ones((4, 6), dtype=bool), big[1], big[0]]
    _, off, _, _ = BO.tables([p.shape for p in planes], guard=0)
    sized = engine.SizedMasks(bits=torch.from_numpy(np.concatenate([BO.pack(p).reshape(-1) for p in planes])).to(DEV),
                              offsets=torch.from_numpy(off).to(DEV), area=None, box=None, status=torch.zeros(1, dtype=torch.int32, device=DEV),
                              sizes=[p.shape for p in planes], level=0)
    got = cas.mask_thin_sized(sized, steps=2)
    got.check()
    assert got.done.tolist() == [1, 1, 1] and got.iters.tolist() == [2, want[1][1], want[0][1]] and want[1][1] > 2
    assert np.array_equal(got.masks.to_numpy(1), want[1][0]) and np.array_equal(got.masks.to_numpy(2), want[0][0])
    assert got.masks.area.tolist() == [3, int(want[1][0].sum()), int(want[0][0].sum())]
    assert got.masks.box[1].tolist() == TO.box_of(want[1][0])


def test_edge_bits_thin_as_sized_planes(cas):
    """§17's packed edge maps, several pixels thick, wrapped as sized planes and thinned: the oracle's one-pixel edges."""
    from camouflaged_vlm_amd import engine
    g = torch.Generator().manual_seed(55)
    smooth = torch.nn.functional.avg_pool2d(torch.rand(3, 1, 72, 72, generator=g), 9, stride=1)          # (3, 1, 64, 64)
    prob = ((smooth - smooth.amin()) / (smooth.amax() - smooth.amin())).to(DEV)
    eb = cas.pack_edges(prob, threshold=0.6)
    n = eb.bits.shape[0]
    off = torch.arange(n + 1, dtype=torch.int64, device=DEV) * eb.bits.shape[1]
    thick = engine.SizedMasks(bits=eb.bits.reshape(-1), offsets=off, area=eb.area, box=None,
                              status=torch.zeros(1, dtype=torch.int32, device=DEV), sizes=[(64, 64)] * n, level=0)
    got = cas.mask_thin_sized(thick)
    got.check()
    for p in range(n):
        x = thick.to_numpy(p)
        want, k = TO.thin(x)
        assert x.sum() > 64 and want.sum() < x.sum()
        assert np.array_equal(got.masks.to_numpy(p), want) and int(got.iters[p]) == k and int(got.masks.area[p]) == int(want.sum()), p


def test_cldice_through_cascade_and_dropin(cas, dropin, monkeypatch):
    from camouflaged_vlm_amd import engine, surfeval
    limb, cut = TO.limb_planes()
    empty = np.zeros_like(limb)
    small = np.ones((9, 40), dtype=bool)
    a, b = [limb, limb, empty, empty, small], [limb, cut, empty, limb, small]
    sa, sb = sized_of(cas, a), sized_of(cas, b)
    pairs = [(p, p) for p in range(5)] + [(1, 0), (0, 1), (0, 3), (0, 4)]                # the last of two different sizes
    torch.cuda.synchronize()
    reads = record_reads(monkeypatch)
    t = cas.mask_cldice(sa, sb, pairs=pairs)
    monkeypatch.undo()
    assert reads == [], reads                                                             # every plane is resident: no synchronisation
    assert isinstance(t, engine.ClDiceTotals)
    host = t.to_host()
    assert host["pairs"].tolist() == [list(p) for p in pairs] and host["status"] == 1    # the refused pair
    with pytest.raises(RuntimeError, match="mask_cldice"):
        t.check()
    got = surfeval.cldice(host)
    for i, (p, q) in enumerate(pairs[:-1]):
        want = TO.cldice_counts(a[p], b[q])
        assert {k: int(host[k][i]) for k in want} == want, i
        assert got["cldice"][i] == TO.cldice(want), i
    assert got["cldice"][:5].tolist() == [1.0, got["cldice"][1], 1.0, 0.0, 1.0] and 0.0 < got["cldice"][1] < 1.0
    assert np.isnan(got["cldice"][-1]) and host["skel_a_in_b"][-1] == -1
    by_image = cas.mask_cldice(sa, sb, a_image=[0, 1, 2, 3, 4], b_image=[0, 1, 2, 3, 4])
    by_image.check()
    assert by_image.pairs.tolist() == [[p, p] for p in range(5)] and torch.equal(by_image.skel_a_in_b, t.skel_a_in_b[:5])
    other = dropin.mask_cldice(sa, sb, pairs=pairs)
    assert all(torch.equal(getattr(other, k), getattr(t, k)) for k in ("skel_a", "skel_a_in_b", "skel_b", "skel_b_in_a"))


def test_end_to_end_on_the_tiny_cascade(tiny, cas, tracer, monkeypatch):
    """The call's own masks against annotations decoded from the call's own encoding: clDice 1; against one annotation with a limb cut
    off: the oracle's value; the launches of infer_classes are the same with and without the call."""
    from camouflaged_vlm_amd import surfeval
    import rle_oracle as RO
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
        t = cas.mask_cldice(h.sized, gts)
        torch.cuda.synchronize()
    both = names(log)
    assert not any("thin" in n for n in alone)
    assert both[:len(alone)] == alone
    assert both[len(alone):] == ["mask_thin_sized"] * 2 + ["mask_inter_sized"] * 2
    t.check()
    assert (surfeval.cldice(t.to_host())["cldice"] == 1.0).all()
    planes = [h.sized.to_numpy(p) for p in range(6)]
    p = max(range(6), key=lambda q: int(planes[q].sum()))
    ys, xs = np.nonzero(planes[p])
    assert planes[p].sum() > 9
    worn = list(planes)
    worn[p] = planes[p].copy()
    worn[p][:, (int(xs.min()) + int(xs.max()) + 1) // 2:] = False     # the right half of the largest mask is cut off
    gts = cas.rle_decode([{"size": list(x.shape), "counts": RO.plane_counts(x).tolist()} for x in worn])
    host = cas.mask_cldice(h.sized, gts).to_host()
    got = surfeval.cldice(host)
    for q in range(6):
        want = TO.cldice_counts(planes[q], worn[q])
        assert {k: int(host[k][q]) for k in want} == want and got["cldice"][q] == TO.cldice(want), q
    assert got["cldice"][p] < 1.0 and all(got["cldice"][q] == 1.0 for q in range(6) if q != p)
    with tracer.Recorder() as log:
        for bad in (dict(max_iter=0), dict(path="fast"), dict(steps=0), dict(max_iter=[1])):
            with pytest.raises(ValueError, match="mask_thin_sized"):
                cas.mask_thin_sized(h.sized, **bad)
        with pytest.raises(ValueError, match="mask_cldice"):
            cas.mask_cldice(h.sized, gts, pairs=[(0, 6)])
        with pytest.raises(ValueError, match="mask_cldice"):
            cas.mask_cldice(h.sized, gts, pairs=[(0, 0)], a_image=[0] * 6, b_image=[0] * 6)
    assert log == []
