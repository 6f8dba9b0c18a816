"""COCO matching on the device: cvlm_coco_match against the published loops (tests/match_oracle.py) and against the host
entry, byte for byte, on every (D, G) shape that crosses a 32-bit word of the taken-bitset, a 64-lane wave or the 128 threads of a
group, with IoU ties, exact threshold hits, special scores, crowds, refused pairs, T = 1 / 16 and A = 1 / 8; 37 ragged groups in one
call; guard bands and a second call into used outputs; every group refusal; Cascade.coco_match and the drop-in on planes from
rle_decode without a synchronisation; and the tiny cascade end to end: annotations made from the call's own encoding give AP = 1, a
lowered score gives the oracle's AP to the last bit.

Figures of the MI355X run this file was written with are in DESIGN.md §22."""
import os
import sys

import numpy as np
import pytest
import torch

import match_oracle as MO
import rle_oracle as RO
from test_classes_gpu import build_tiny
from test_match_cpu import SMALL_RNGS, ragged_groups, refusal_cases, shape_cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TABLES = ("dt_order", "dt_match", "dt_ignore", "gt_match", "gt_ignore")


def entries():
    from camouflaged_vlm_amd import hip
    return hip.coco_match, hip.coco_match_host


@pytest.mark.parametrize("name", [c[0] for c in shape_cases()])
def test_device_equals_the_oracle_and_the_host_entry(name):
    _, groups, kw = next(c for c in shape_cases() if c[0] == name)
    dev_fn, host_fn = entries()
    tabs = MO.tables(groups)
    res = MO.run_entry(dev_fn, tabs, dev=DEV, guard=16, **kw)
    assert res["status"] == 0
    MO.check_groups(res, groups, **kw)
    host = MO.run_entry(host_fn, tabs, **kw)
    again = MO.run_entry(dev_fn, tabs, dev=DEV, outs=res["outs"], **kw)               # a second call into used outputs
    for key in TABLES:
        assert np.array_equal(res[key], host[key]) and np.array_equal(res[key], again[key]), key
    assert again["status"] == 0


def test_ragged_groups_in_one_call():
    groups = ragged_groups()
    assert len(groups) == 37
    dev_fn, host_fn = entries()
    tabs = MO.tables(groups)
    res = MO.run_entry(dev_fn, tabs, dev=DEV, guard=16, area_rngs=SMALL_RNGS, max_det=20)
    assert res["status"] == 0
    MO.check_groups(res, groups, area_rngs=SMALL_RNGS, max_det=20)
    host = MO.run_entry(host_fn, tabs, area_rngs=SMALL_RNGS, max_det=20)
    for key in TABLES:
        assert np.array_equal(res[key], host[key]), key


@pytest.mark.parametrize("name", [c[0] for c in refusal_cases()])
def test_refuses_whole_groups(name):
    _, groups, tabs, refused = next(c for c in refusal_cases() if c[0] == name)
    dev_fn, host_fn = entries()
    res = MO.run_entry(dev_fn, tabs, dev=DEV, guard=16, area_rngs=SMALL_RNGS)
    assert res["status"] == 1
    MO.check_groups(res, groups, area_rngs=SMALL_RNGS, refused=refused)
    host = MO.run_entry(host_fn, tabs, area_rngs=SMALL_RNGS)
    for key in TABLES:
        assert np.array_equal(res[key], host[key]), key
    whole = MO.run_entry(dev_fn, MO.tables(groups), dev=DEV, outs=res["outs"], area_rngs=SMALL_RNGS)     # the status is zeroed again
    assert whole["status"] == (1 if "1024" in name else 0)


# ---- tiny geometry, exact ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(golden_dir):
    with np.load(os.path.join(golden_dir, "tiny_classes.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def tiny():
    from camouflaged_vlm_amd import spec, synth
    g, c = spec.TINY_SAM, spec.TINY_CLIP
    sd_np = synth.make_full_state_dict(g, c)
    inp, ci, cm = synth.make_inputs(g, c, batch=2)
    dev = torch.device(DEV)
    return g, c, sd_np, tuple(torch.from_numpy(t).to(dev) for t in (inp, ci, cm)), dev


@pytest.fixture(scope="module")
def cas(tiny, gold):
    return build_tiny(tiny, gold)


@pytest.fixture(scope="module")
def dropin(tiny, gold, golden_dir):
    import camouflaged_vlm_amd as cv
    if cv.DROPIN_DIR not in sys.path:
        sys.path.insert(0, cv.DROPIN_DIR)
    import models
    from cocotrainers.mapleAlphaCLIP import CustomCLIP
    g, c, sd_np, _, _ = tiny
    with np.load(os.path.join(golden_dir, "tiny_cascade.npz")) as z:
        eot_train = z["eot_train"].tolist()
    clip = CustomCLIP(geometry=c, eot_train=eot_train, eot_test=gold["eot_test"].tolist())
    enc_cfg = dict(name="sam", img_size=g.inp_size, mlp_ratio=4, patch_size=16, qkv_bias=True, use_rel_pos=True,
                   window_size=14, out_chans=256, scale_factor=32, input_type="fft", freq_nums=0.25, prompt_type="highpass",
                   prompt_embed_dim=256, tuning_stage=1234, handcrafted_tune=True, embedding_tune=True, adaptor="adaptor",
                   embed_dim=g.embed_dim, depth=g.depth, num_heads=g.num_heads, global_attn_indexes=list(g.global_attn_indexes))
    model = models.make({"name": "sam_maskdecoder_edge", "args": {"inp_size": g.inp_size, "loss": "iou", "encoder_mode": enc_cfg}}).cuda()
    model.train_text_features = model.train_text_features[:c.n_cls_train]
    model.test_text_features = model.test_text_features[:c.n_cls_test]
    model.load_mapleAlphaCLIP(clip)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    return model.eval()


def record_reads(monkeypatch):
    reads = []
    for name in ("item", "cpu", "tolist", "numpy"):
        real = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _real=real, _n=name, **k: (reads.append(_n), _real(self, *a, **k))[1])
    return reads


def oracle_groups(req, det_planes, gt_planes, scores, iscrowd=None, gt_area=None):
    """The groups of a MatchRequest as the oracle takes them, from the planes as bool arrays: the intersections by & and sum."""
    groups = []
    for e in range(len(req.keys)):
        ds = req.det_perm[req.det_offsets[e]:req.det_offsets[e + 1]]
        gs = req.gt_perm[req.gt_offsets[e]:req.gt_offsets[e + 1]]
        inter = np.array([[int((det_planes[d] & gt_planes[g]).sum()) for g in gs] for d in ds], dtype=np.int64).reshape(len(ds), len(gs))
        groups.append(dict(inter=inter, det_area=np.array([int(det_planes[d].sum()) for d in ds], dtype=np.int64),
                           scores=np.asarray(scores, dtype=np.float32)[ds], gt_area=np.array([int(gt_planes[g].sum()) for g in gs], dtype=np.int64),
                           range_area=None if gt_area is None else np.asarray(gt_area, dtype=np.float64)[gs],
                           iscrowd=np.zeros(len(gs), dtype=np.uint8) if iscrowd is None else np.asarray(iscrowd, dtype=np.uint8)[gs]))
    return groups


def oracle_stats(req, groups, max_dets=(1, 10, 100)):
    cats = sorted({k[0] for k in req.keys}) if req.keys[0][0] is not None else [None]
    evals = [[[] for _ in MO.AREA_RNGS] for _ in cats]
    for key, grp in zip(req.keys, groups):
        for a, r in enumerate(MO.evaluate_group(grp, max_det=req.max_det)):
            evals[cats.index(key[0])][a].append(r)
    return MO.summarize(MO.accumulate(evals, len(cats), 4, max_dets=max_dets))


def test_coco_match_through_cascade_and_dropin(cas, dropin, monkeypatch):
    """Random planes of three images of two sizes through rle_decode: with and without categories, scores on the device (no
    synchronisation) and on the host, a crowd, the file's own areas, an image with annotations only and one with detections only."""
    from camouflaged_vlm_amd import cocoeval
    from camouflaged_vlm_amd.engine import CocoMatches
    rng = np.random.default_rng(22)
    sz = {0: (97, 131), 1: (97, 131), 2: (33, 31), 3: (40, 70), 4: (21, 33)}
    det_image = [0, 0, 1, 1, 2, 0, 1, 1, 4, 0]
    gt_image = [1, 0, 2, 0, 1, 3, 0]
    det_cat = [5, 5, 5, 2, 2, 2, 5, 5, 2, 5]
    gt_cat = [5, 5, 2, 2, 5, 5, 5]
    base = {i: rng.random(sz[i]) < 0.5 for i in sz}
    noisy = lambda i, p: base[i] ^ (rng.random(sz[i]) < p)            # planes close to their image's base: IoUs on both sides of 0.5
    A = [noisy(i, 0.05 * (n % 4)) for n, i in enumerate(det_image)]
    B = [noisy(i, 0.04 * (n % 3)) for n, i in enumerate(gt_image)]
    coco = lambda ms: [{"size": list(m.shape), "counts": RO.plane_counts(m).tolist()} for m in ms]
    a, b = cas.rle_decode(coco(A)), cas.rle_decode(coco(B))
    scores = rng.permutation(10).astype(np.float32) / 10
    scores[3] = scores[6]
    on_dev = torch.from_numpy(scores).to(DEV)
    crowd, file_area = [0, 0, 0, 1, 0, 0, 0], [float(m.sum()) * 0.9 for m in B]
    torch.cuda.synchronize()
    for kw in (dict(), dict(det_category=det_cat, gt_category=gt_cat), dict(det_category=det_cat, gt_category=gt_cat, iscrowd=crowd, gt_area=file_area, max_det=2)):
        reads = record_reads(monkeypatch)
        m = cas.coco_match(a, b, scores=on_dev, det_image=det_image, gt_image=gt_image, **kw)
        monkeypatch.undo()
        assert reads == [], reads
        assert isinstance(m, CocoMatches)
        m.check()
        h = m.to_host()
        groups = oracle_groups(m.request, A, B, scores, kw.get("iscrowd"), kw.get("gt_area"))
        MO.check_groups(h, groups, max_det=m.request.max_det)
        assert (h["dt_match"] >= 0).any() and (h["dt_match"][0, 0] != h["dt_match"][0, -1]).any()
        assert np.array_equal(h["score"], scores[m.request.det_perm])
        if "max_det" not in kw:
            assert cocoeval.summarize(cocoeval.accumulate(m)) == oracle_stats(m.request, groups)
        for other in (cas.coco_match(a, b, scores=scores.tolist(), det_image=det_image, gt_image=gt_image, **kw),
                      dropin.coco_match(a, b, scores=on_dev, det_image=det_image, gt_image=gt_image, **kw)):
            for key in TABLES:
                assert torch.equal(getattr(other, key), getattr(m, key)), key
    # a side without planes: nothing is intersected
    none = cas.coco_match(None, b, scores=[], det_image=[], gt_image=gt_image)
    assert none.overlaps is None and none.status.item() == 0 and none.dt_match.shape == (4, 10, 0) and (none.gt_match == -1).all()
    assert np.array_equal(none.gt_ignore.cpu().numpy(), np.array([[0 if lo <= m.sum() <= hi else 1 for m in (B[q] for q in none.request.gt_perm)]
                                                                  for lo, hi in MO.AREA_RNGS], dtype=np.uint8))
    only = cas.coco_match(a, None, scores=on_dev, det_image=det_image, gt_image=[])
    assert only.overlaps is None and (only.dt_match == -1).all() and only.status.item() == 0
    # bad requests raise before anything is launched
    from camouflaged_vlm_amd import hip
    seen = []
    for name in ("coco_match", "mask_inter_sized"):
        monkeypatch.setattr(hip, name, lambda *a, _n=name, **k: seen.append(_n))
    for bad in (dict(det_image=det_image[:-1]), dict(det_category=det_cat), dict(iou_thrs=[0.0]), dict(max_det=0), dict(scores=on_dev[:-1]),
                dict(scores=on_dev.double()), dict(scores=[float("nan")] * 10), dict(scores=None), dict(gt_image=[0] * 7),
                dict(dets=a.bits), dict(gts=cas.rle_decode(coco(B), stats=False))):
        args = dict(dets=a, gts=b, scores=on_dev, det_image=det_image, gt_image=gt_image)
        args.update(bad)
        with pytest.raises(ValueError):
            cas.coco_match(args.pop("dets"), args.pop("gts"), **args)
    assert seen == []


SIZES = [(213, 320), (480, 641)]
CLASSES = [[0, 1, 2], [2, 1, 0]]


def test_end_to_end_on_the_tiny_cascade(tiny, cas, monkeypatch):
    """Annotations made from the call's own rle="sized" output match their hypotheses at every threshold and give AP = 1; with one
    annotation left out and its hypothesis -- now a false positive -- ranked above a lowered true positive, AP is the oracle's."""
    from camouflaged_vlm_amd import cocoeval
    _, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    h = cas.infer_classes(inp, ci, cm, classes=torch.tensor(CLASSES), masks="bits", sizes=SIZES, rle="sized")
    planes = [h.sized.to_numpy(p) for p in range(6)]
    image, cat = [0, 0, 0, 1, 1, 1], [c for row in CLASSES for c in row]
    full = [p for p in range(6) if planes[p].any()]
    assert len(full) >= 3
    dicts = h.rle.to_coco()
    gts = cas.rle_decode([dicts[p] for p in full])
    scores = h.sized.area.to(torch.float32)                           # on the device; an empty hypothesis ranks last
    m = cas.coco_match(h.sized, gts, scores=scores, det_image=image, gt_image=[image[p] for p in full], det_category=cat,
                       gt_category=[cat[p] for p in full])
    m.check()
    host = m.to_host()
    for e, key in enumerate(host["keys"]):
        d0, d1, g0, g1 = host["det_offsets"][e], host["det_offsets"][e + 1], host["gt_offsets"][e], host["gt_offsets"][e + 1]
        assert d1 - d0 == 1 and (g1 - g0 == 1) == bool(planes[m.request.det_perm[d0]].any())
        assert (host["dt_match"][0, :, d0] == (g0 if g1 > g0 else -1)).all()         # at every threshold
    stats = cocoeval.summarize(cocoeval.accumulate(m))
    assert stats[0] == stats[1] == stats[2] == 1.0 and stats[8] == 1.0
    # class-agnostic, the annotation of hypothesis full[1] left out, the score of full[0] lowered below everything
    kept = [p for p in full if p != full[1]]
    gts = cas.rle_decode([dicts[p] for p in kept])
    s = np.linspace(0.9, 0.4, 6).astype(np.float32)
    for lowered in (False, True):
        if lowered:
            s[full[0]] = 0.05
        m = cas.coco_match(h.sized, gts, scores=torch.from_numpy(s).to(DEV), det_image=image, gt_image=[image[p] for p in kept])
        m.check()
        groups = oracle_groups(m.request, planes, [planes[p] for p in kept], s)
        MO.check_groups(m.to_host(), groups)
        got, want = cocoeval.summarize(cocoeval.accumulate(m)), oracle_stats(m.request, groups)
        assert got == want, (got, want)                               # to the last bit
        assert 0.0 < got[0] <= 1.0
