"""Mask NMS on the device: cvlm_mask_nms_inter and cvlm_mask_nms == their host twins == the oracle
(tests/nms_oracle.py) on the one ragged scene -- D from 1 to 1024, interleaved groups, dirty pad bits -- with every output pre-filled
with garbage, a second identical call giving identical bytes, guard bands around inter; refusals as on the host; the tiny engine
through pack_masks_sized -> mask_regions_sized -> compact -> classify_regions -> mask_nms_sized -> select -> mask_rle_sized /
coco_match; Q = 0 launches nothing.  Integers, greedy and linear decays are exact; the gaussian decay is within one float32 ulp."""
import os

import numpy as np
import pytest
import torch

import nms_oracle as NO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COMBOS = [("iou", "greedy", False), ("min", "greedy", True), ("iou", "linear", True), ("min", "linear", False), ("iou", "gaussian", False),
          ("min", "gaussian", True)]


@pytest.fixture(scope="module")
def hip():
    from camouflaged_vlm_amd import hip
    hip.load()
    return hip


@pytest.fixture(scope="module")
def sc():
    return NO.scene()


def test_inter_device_equals_host_twin_equals_oracle(hip, sc):
    got = NO.run_inter(hip, sc, dev=DEV)
    assert got["status"] == 0 and got["bands"]
    assert np.array_equal(got["inter"], sc["inter"])
    host = NO.run_inter(hip, sc)
    assert np.array_equal(got["inter"], host["inter"]) and host["status"] == 0
    again = NO.run_inter(hip, sc, dev=DEV)
    assert again["inter"].tobytes() == got["inter"].tobytes() and again["status"] == 0 and again["bands"]
    rejected = int((sc["inter"] == 0).sum())
    print(f"cvlm_mask_nms_inter: {sc['inter'].size} pairs, {rejected} of them 0")


@pytest.mark.parametrize("measure,method,class_aware", COMBOS)
def test_nms_device_equals_host_twin_equals_oracle(hip, sc, measure, method, class_aware):
    kw = dict(measure=measure, method=method, class_aware=class_aware, thr=0.5 if measure == "iou" else 0.7, sigma=2.0)
    want = NO.nms_oracle(sc, sc["inter"], **kw)
    got = NO.run_nms(hip, sc, sc["inter"], dev=DEV, **kw)
    host = NO.run_nms(hip, sc, sc["inter"], **kw)
    assert got["status"] == 0 and host["status"] == 0
    NO.same(got, want, method)
    NO.same(got, host, method)                                        # the gaussian: device against host twin to the same bound
    again = NO.run_nms(hip, sc, sc["inter"], dev=DEV, **kw)
    for k in NO.EXACT + ("decay",):
        assert again[k].tobytes() == got[k].tobytes(), k
    if method == "gaussian":
        err = np.abs(got["decay"].astype(np.float64) - want["decay"].astype(np.float64)) / np.maximum(want["decay"], 1e-30)
        print(f"gaussian decay against the oracle: {float(err.max()) * 2 ** 23:.3f} ulp at the worst, "
              f"{int((got['decay'] != host['decay']).sum())} values differ from the host twin")


def test_the_threshold_tie_and_the_chain_on_the_device(hip, sc):
    row = lambda k: NO.row_of(sc, k)
    at_half = NO.run_nms(hip, sc, sc["inter"], dev=DEV, thr=0.5)
    below = NO.run_nms(hip, sc, sc["inter"], dev=DEV, thr=NO.BELOW_HALF)
    assert at_half["keep"][row(7)] == 1 and below["keep"][row(7)] == 0 and below["by"][row(7)] == row(6)
    a, b, c = row(10), row(11), row(12)
    assert at_half["keep"][[a, b, c]].tolist() == [1, 0, 1] and at_half["by"][b] == a and at_half["by"][c] == -1


def test_refusals_on_the_device_are_the_host_twins(hip):
    small = NO.scene(big=False)
    box = small["box"].copy()
    box[NO.row_of(small, 1)] = [5, 0, 4, 0]                           # image 1: a box with x0 > x1, its pair is refused
    goff = small["group_offsets"].copy()
    goff[3], goff[4] = goff[4], goff[3]                               # images 2 .. 4 run backwards or past their pair blocks
    for over in (dict(box=box), dict(group_offsets=goff), dict(box=box, group_offsets=goff)):
        d, h = NO.run_inter(hip, small, dev=DEV, **over), NO.run_inter(hip, small, **over)
        assert d["status"] == h["status"] == (1 if "box" in over else 0) | (2 if "group_offsets" in over else 0)
        assert np.array_equal(d["inter"], h["inter"]) and d["bands"] and bool((d["inter"] == -1).any())
        nd = NO.run_nms(hip, small, h["inter"], dev=DEV, **{k: v for k, v in over.items() if k != "box"})
        nh = NO.run_nms(hip, small, h["inter"], **{k: v for k, v in over.items() if k != "box"})
        assert nd["status"] == nh["status"] == (2 if "group_offsets" in over else 0)
        NO.same(nd, nh, "greedy")


# ---- the tiny engine -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(golden_dir):
    with np.load(os.path.join(golden_dir, "tiny_classes.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def chain(gold):
    """The engine, K = 2 hypotheses per image as P = 4 planes of mask logits, their sized planes at two ragged sizes with the same two
    blobs ORed into every plane -- one object found under both prompts --, the split, the compacted instances and their classes."""
    from camouflaged_vlm_amd import spec, synth
    from camouflaged_vlm_amd.engine import Cascade, Precision
    g, c = spec.TINY_SAM, spec.TINY_CLIP
    dev = torch.device(DEV)
    sd_np = synth.make_full_state_dict(g, c)
    inp, ci, cm = (torch.from_numpy(t).to(dev) for t in synth.make_inputs(g, c, batch=2))
    cas = Cascade({k: torch.from_numpy(v) for k, v in sd_np.items()}, g, c, dev, Precision.named("exact"))
    cas.clip.set_text_bank(cas.clip.text_features(gold["eot_test"].tolist(), "test"), torch.from_numpy(gold["bank_test"]), "test")
    h = cas.infer_classes(inp, ci, cm, topk=2)
    logits = h.masks.reshape(-1, 1, g.inp_size, g.inp_size).clone()
    image_of = [0, 0, 1, 1]
    sizes = [(37, 45), (37, 45), (50, 33), (50, 33)]
    sized = cas.pack_masks_sized(logits, sizes)
    for p, (hh, ww) in enumerate(sizes):
        blobs = np.zeros((hh, ww), bool)
        blobs[1:4, 1:5] = blobs[hh - 5:hh - 1, ww - 7:ww - 2] = True
        lo, hi = sized.byte_range(p)
        sized.bits[lo:hi] |= torch.from_numpy(NO.pack_rows(blobs)).to(dev)
    regs = cas.mask_regions_sized(sized, regions=4)
    regions, plane_of, _ = regs.compact()
    cls = cas.classify_regions(regions, plane_of, logits, ci, image_of=image_of)
    return dict(cas=cas, regions=regions, image=[image_of[int(p)] for p in plane_of], cls=cls, scores=cls.logits.softmax(-1).amax(-1))


def engine_oracle(regions, image, scores, category, **kw) -> dict:
    """The oracle on what the device holds: the instances' bytes, areas, boxes, scores and categories read back."""
    dims, off = NO.tables(regions.sizes)
    keys, member, goff, poff = NO.groups_of(image)
    sc = dict(bits=regions.bits.cpu().numpy(), offsets=off, dims=dims, area=regions.area.cpu().numpy(), box=regions.box.cpu().numpy(),
              member=member, group_offsets=goff, pair_offsets=poff, scores=scores.cpu().numpy().astype(np.float32),
              category=None if category is None else category.cpu().numpy().astype(np.int32))
    sc["inter"] = NO.inter_oracle(sc)
    return dict(NO.nms_oracle(sc, sc["inter"], class_aware=category is not None, **kw), inter=sc["inter"])


def test_the_chain_from_hypotheses_to_coco(chain):
    from camouflaged_vlm_amd import maskpost
    cas, regions, image, scores, pred = chain["cas"], chain["regions"], chain["image"], chain["scores"], chain["cls"].pred
    Q = len(regions.sizes)
    out = cas.mask_nms_sized(regions, scores=scores, image=image, category=pred)
    want = engine_oracle(regions, image, scores, pred)
    got = {k: getattr(out, k).cpu().numpy() for k in NO.EXACT + ("decay", "inter")}
    NO.same(got, want, "greedy")
    assert np.array_equal(got["inter"], want["inter"]) and out.status.cpu().tolist() == [0, 0]
    kept, idx = out.select(regions)
    print(f"{Q} instances of K = 2 hypotheses, {idx.size} survive: predicted classes {pred.cpu().tolist()}, n_keep {got['n_keep'].tolist()}")
    assert 0 < idx.size < Q and idx.tolist() == np.flatnonzero(want["keep"]).tolist()
    for n, q in enumerate(idx):
        assert np.array_equal(kept.to_numpy(n), regions.to_numpy(int(q)))
    assert torch.equal(kept.area, regions.area[torch.from_numpy(idx).to(regions.area.device)])
    # the survivors go on as any SizedMasks: COCO results, and matched against themselves every one is a true positive
    ids, cats, sc = [image[int(q)] for q in idx], pred.cpu().numpy()[idx].tolist(), out.rescored(scores)[torch.from_numpy(idx).to(scores.device)]
    res = maskpost.instances_to_coco(cas.mask_rle_sized(kept), ids, cats, sc, boxes=kept.box)
    assert len(res) == idx.size and all(sum(d["segmentation"]["counts"][1::2]) == int(a) for d, a in zip(res, kept.area.cpu()))
    m = cas.coco_match(kept, kept, scores=sc, det_image=ids, gt_image=ids, det_category=cats, gt_category=cats)
    m.check()
    assert bool((m.dt_match[0, 0] >= 0).all())
    # class-agnostic, Matrix NMS and host-side columns give the oracle's too
    for kw, category in ((dict(), None), (dict(method="linear"), pred), (dict(method="gaussian", measure="min", sigma=0.5), None)):
        o = cas.mask_nms_sized(regions, scores=scores.cpu().tolist(), image=image, category=None if category is None else category.cpu().tolist(), **kw)
        w = engine_oracle(regions, image, scores, category, **kw)
        NO.same({k: getattr(o, k).cpu().numpy() for k in NO.EXACT + ("decay",)}, w, kw.get("method", "greedy"))


def test_no_instance_launches_nothing_and_bad_arguments_raise_first(chain, monkeypatch):
    from camouflaged_vlm_amd import hip, maskpost
    cas, regions, image, scores = chain["cas"], chain["regions"], chain["image"], chain["scores"]
    calls = []
    monkeypatch.setattr(hip, "_call", lambda name, *a: calls.append(name))
    none = maskpost.SizedMasks(bits=regions.bits[:0], offsets=regions.offsets[:1], area=regions.area[:0], box=regions.box[:0],
                               status=regions.status, sizes=[])
    e = cas.mask_nms_sized(none, scores=scores[:0], image=[])
    assert e.keep.shape == e.by.shape == e.decay.shape == e.order.shape == e.n_keep.shape == e.inter.shape == (0,) and calls == []
    assert e.keep.dtype == torch.uint8 and e.decay.dtype == torch.float32 and e.status.tolist() == [0, 0]
    kept, idx = e.select(none)
    assert idx.size == 0 and kept.sizes == []
    Q = len(regions.sizes)
    for kw in (dict(scores=scores[:-1], image=image), dict(scores=scores.double(), image=image), dict(scores=scores, image=image[:-1]),
               dict(scores=scores, image=image, category=scores), dict(scores=scores, image=image, category=[0] * (Q - 1)),
               dict(scores=scores, image=image, iou=1.5), dict(scores=scores, image=image, method="soft"),
               dict(scores=["a"] * Q, image=image)):
        with pytest.raises(ValueError):
            cas.mask_nms_sized(regions, **kw)
    with pytest.raises(ValueError):
        cas.mask_nms_sized(regions.bits, scores=scores, image=image)
    no_box = maskpost.SizedMasks(bits=regions.bits, offsets=regions.offsets, area=regions.area, box=None, status=regions.status, sizes=regions.sizes)
    with pytest.raises(ValueError):
        cas.mask_nms_sized(no_box, scores=scores, image=image)
    assert calls == []
