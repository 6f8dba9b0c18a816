"""Panoptic quality on the device: the cvlm_pan_* kernels against the oracle (tests/pq_oracle.py: the definition in numpy)
and against the host entries, exactly -- integers to the count, IoU and their sums as f64 bit patterns: the hand-written known answers,
the remap on both input types, the pair histogram on every width around the unit of 64 pixels x heights 1, 2, 33, seven ragged images
in one call, slot tables on both sides of the LDS bound, uniform and checkered maps, accumulating calls, used outputs, guard bands, an
unaligned base, out-of-range indices and refused images, the totals over two batches at B = 1, 9 and C = 3, 133, 4097;
Cascade.panoptic_remap / panoptic_quality and LabelMaps.pq_inputs behind infer_classes on the tiny geometry, and the drop-in."""
import json
import os

import numpy as np
import pytest
import torch

import pq_oracle as PO
from test_labels_gpu import CLASSES, SIZES, cas, gold, tiny, tracer  # noqa: F401  (fixtures)
from test_pq_cpu import check_remap

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def test_known_answers():
    PO.case_known(DEV)


def test_remap():
    check_remap(DEV)


def test_widths_and_heights():
    PO.case_widths_and_heights(DEV)


@pytest.mark.parametrize("which", range(5))
def test_slot_shapes_on_both_sides_of_the_lds_bound(which):
    G, S = PO.slot_shapes()[which]
    PO.case_slot_shape(DEV, G, S)


def test_uniform_and_checkered_maps():
    PO.case_uniform_and_checkered(DEV)


def test_accumulating_calls_used_outputs_and_an_unaligned_base():
    PO.case_accumulating_calls(DEV)


def test_out_of_range_index_is_counted_nowhere():
    PO.case_out_of_range_index(DEV)


def test_refused_image_is_skipped_whole():
    PO.case_refused_image(DEV)


@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("C_", [3, 133, 4097])
def test_accumulate_over_two_batches(B, C_):
    PO.case_accumulate(DEV, B, C_)


def test_device_equals_the_host_entries_on_shifted_maps():
    """Most pairs match with IoU < 1: the f64 divisions and sums of the device against the host entries' and the oracle's, bit by bit."""
    pred, gt, pred_cat, gt_cat, gt_crowd = PO.shifted(PO.RAGGED[1:], 20, 61, 3)
    G, S = gt_cat.shape[1], pred_cat.shape[1]
    got = PO.Run(PO.RAGGED[1:], G, S, 61, DEV).score(pred, pred_cat, gt, gt_cat, gt_crowd)
    host = PO.Run(PO.RAGGED[1:], G, S, 61, "cpu").score(pred, pred_cat, gt, gt_cat, gt_crowd)
    PO.compare(got, host)
    PO.compare(got, PO.pq_compute(pred, pred_cat, gt, gt_cat, gt_crowd, 61))
    assert (got["pred_match"] > 0).sum() > 10 and (got["pred_iou"][got["pred_match"] > 0] < 1.0).any()


# ---- tiny geometry ------------------------------------------------------------------------------------------------------------------------------
def as_images(flat: torch.Tensor, sizes) -> list:
    a, out, at = flat.cpu().numpy(), [], 0
    for h, w in sizes:
        out.append(a[at:at + h * w].reshape(h, w))
        at += h * w
    return out


def test_infer_classes_scored_end_to_end(tiny, cas, tracer, golden_dir, monkeypatch):
    from camouflaged_vlm_amd import segeval
    from camouflaged_vlm_amd.engine import PanopticTotals
    _, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    classes = torch.tensor(CLASSES)
    h = cas.infer_classes(inp, ci, cm, classes=classes, masks="bits", sizes=SIZES, label_maps=True)
    m = h.label_maps
    pred, pred_cat = m.pq_inputs(h.classes)
    seg = m.segment.cpu().numpy().astype(np.int64)
    assert np.array_equal(pred.cpu().numpy(), np.where(seg < 0, 0, seg + 1)) and pred_cat.tolist() == [[-1] + c for c in h.classes.tolist()]
    assert int(m.n_segments.sum()) > 0
    # ground truth made from the call's own panoptic map: its segments under raw ids 1000 + 7 * slot, listed in reverse order
    K = m.K
    kept = m.kept.cpu().numpy()
    listed = [[k for k in reversed(range(K)) if kept[b, k]] for b in range(2)]
    raw = torch.where(pred > 0, 1000 + 7 * pred, pred)
    segments = [[(1000 + 7 * (k + 1), CLASSES[b][k], 0) for k in listed[b]] for b in range(2)]
    gt = cas.panoptic_remap(raw, SIZES, segments)
    gt.check()
    slot = np.zeros((2, K + 1), np.int64)
    for b in range(2):
        for i, k in enumerate(listed[b]):
            slot[b, k + 1] = i + 1
    want_gt = np.concatenate([slot[b][p.reshape(-1)] for b, p in enumerate(as_images(pred, SIZES))])
    assert gt.unknown.tolist() == [0, 0] and np.array_equal(gt.gt.cpu().numpy(), want_gt)
    rgb = torch.stack([raw % 256, raw // 256 % 256, raw // 65536], dim=1).to(torch.uint8)
    assert torch.equal(cas.panoptic_remap(rgb, SIZES, segments, rgb=True).gt, gt.gt)
    t = cas.panoptic_quality(pred, pred_cat, gt.gt, gt.gt_cat, gt.gt_crowd, SIZES, num_classes=4)
    assert isinstance(t, PanopticTotals)
    t.check()
    host = t.to_host()
    present = host["counts"].sum(0) > 0
    avg = segeval.pq_average(t.counts, t.iou_sum)
    assert present.any() and all((avg["per_class"][k][present] == 1.0).all() for k in ("pq", "sq", "rq"))
    assert avg["All"] == dict(pq=1.0, sq=1.0, rq=1.0, n=int(present.sum()))
    assert host["counts"][0].sum() == int(m.n_segments.sum()) and not host["counts"][1:].any()
    # one segment relabelled, one turned into crowd: every count and iou_sum is the oracle's on the same maps
    gt_cat, gt_crowd = gt.gt_cat.copy(), gt.gt_crowd.copy()
    (b0, k0), (b1, k1) = np.argwhere(kept)[0], np.argwhere(kept)[-1]
    gt_cat[b0, slot[b0, k0 + 1]] = (gt_cat[b0, slot[b0, k0 + 1]] + 1) % 4
    gt_crowd[b1, slot[b1, k1 + 1]] = 1
    moved = [np.roll(g, (3, 5), (0, 1)) for g in as_images(gt.gt, SIZES)]
    t2 = cas.panoptic_quality(pred, pred_cat, moved, gt_cat, gt_crowd, SIZES, num_classes=4)
    want = PO.pq_compute(as_images(pred, SIZES), pred_cat.cpu().numpy(), moved, gt_cat, gt_crowd, 4)
    PO.compare(t2.to_host(), want)
    assert want["counts"][1].sum() + want["counts"][2].sum() > 0
    # totals= sums the two calls on the device
    t3 = cas.panoptic_quality(pred, pred_cat, gt.gt, gt.gt_cat, gt.gt_crowd, SIZES, num_classes=4, totals=t2)
    both = PO.pq_compute(as_images(pred, SIZES), pred_cat.cpu().numpy(), as_images(gt.gt, SIZES), gt.gt_cat, gt.gt_crowd, 4, want["totals"])
    PO.compare(t3.to_host(), both, names=("counts", "inter", "pred_match", "gt_match"))
    # the call itself launches what it launched before this family existed; the family's own launches come behind it
    with open(os.path.join(golden_dir, "mask_post_launches.json")) as f:
        recorded = json.load(f)
    with tracer.Recorder() as log:
        cas.infer_classes(inp, ci, cm, classes=classes, masks="bits")
        torch.cuda.synchronize()
    names = [e if isinstance(e, str) else e[0] for e in log]
    assert names == [recorded["names"][e if isinstance(e, int) else e[0]] for e in recorded["calls"]["infer_classes bits"]]
    with tracer.Recorder() as log:
        h2 = cas.infer_classes(inp, ci, cm, classes=classes, masks="bits", sizes=SIZES, label_maps=True)
        n_call = len(log)
        p2, c2 = h2.label_maps.pq_inputs(h2.classes)
        cas.panoptic_quality(p2, c2, gt.gt, gt.gt_cat, gt.gt_crowd, SIZES, num_classes=4)
        torch.cuda.synchronize()
    names = [e if isinstance(e, str) else e[0] for e in log]
    assert not any(n.startswith("pan_") for n in names[:n_call])
    assert names[n_call:] == ["label_lookup", "pan_pair_hist", "pan_match", "pan_accumulate"]


def test_bad_requests_raise_and_launch_nothing(cas, tracer):
    pred = torch.zeros(SIZES[0][0] * SIZES[0][1], dtype=torch.int32, device=DEV)
    ok = dict(pred=pred, pred_cat=[[-1, 0]], gt=pred, gt_cat=[[-1, 1]], gt_crowd=[[0, 0]], sizes=SIZES[:1], num_classes=2)
    with tracer.Recorder() as log:
        for kw in (dict(num_classes=65537), dict(sizes=SIZES), dict(pred_cat=[[-1, 2]]), dict(gt_cat=[[0, 1]]), dict(gt_crowd=[[0, 0, 0]]),
                   dict(gt=pred[:-1]), dict(pred_cat=torch.zeros(1, 2, device=DEV)), dict(gt_cat=torch.zeros(2, 2, dtype=torch.int32, device=DEV))):
            with pytest.raises(ValueError, match="panoptic_quality"):
                cas.panoptic_quality(**dict(ok, **kw))
        for kw in (dict(segments=[]), dict(segments=[[(3, 1, 0), (3, 1, 0)]]), dict(raw=pred[:-1]), dict(rgb=True)):
            k = dict(dict(raw=pred, sizes=SIZES[:1], segments=[[(3, 1, 0)]]), **kw)
            with pytest.raises(ValueError, match="panoptic_remap"):
                cas.panoptic_remap(k.pop("raw"), k.pop("sizes"), k.pop("segments"), **k)
    assert log == [], log[:5]


def test_dropin_passes_panoptic_calls_through(tiny, gold, golden_dir):
    import sys
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
    model.eval()
    sizes = PO.RAGGED[1:]
    pred, gt_dense, pred_cat, gt_cat, gt_crowd = PO.shifted(sizes, 6, 5, 17)
    segments = [[(10 * (s + 1), int(gt_cat[b, s + 1]), int(gt_crowd[b, s + 1])) for s in range(6)] for b in range(len(sizes))]
    raw = [np.where(g_ > 0, 10 * g_, 0) for g_ in gt_dense]
    gt = model.panoptic_remap(raw, sizes, segments)
    assert np.array_equal(gt.gt.cpu().numpy(), PO.flat(gt_dense)) and np.array_equal(gt.gt_cat, gt_cat) and np.array_equal(gt.gt_crowd, gt_crowd)
    t = model.panoptic_quality(pred, pred_cat, gt.gt, gt.gt_cat, gt.gt_crowd, sizes, num_classes=5)
    PO.compare(t.to_host(), PO.pq_compute(pred, pred_cat, gt_dense, gt_cat, gt_crowd, 5))
