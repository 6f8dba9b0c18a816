"""CPU: panoptic quality -- the oracle (tests/pq_oracle.py: the definition in numpy) on hand-written known answers; the
host entries cvlm_debug_pan_*_host (the kernels' per-thread functions run sequentially on the CPU) against the oracle on every shape
the device tests use, exactly: integers to the count, IoU and their sums as f64 bit patterns; the refusals of the entries (no GPU
needed: they refuse before launching); the host checks engine.pq_request, Cascade.panoptic_remap and Cascade.panoptic_quality with the
launchers replaced by a recorder; segeval.pq_average; LabelMaps.pq_inputs' argument check."""
import ctypes as C

import numpy as np
import pytest
import torch

from camouflaged_vlm_amd import hip, segeval
from camouflaged_vlm_amd.engine import MaskUtilities, PanopticGroundTruth, PanopticTotals, pq_request, pq_segments_request
import pq_oracle as PO

DEV = "cpu"


# ---- known answers ----------------------------------------------------------------------------------------------------------------------------
def test_known_answers():
    PO.case_known(DEV)


def test_pq_average_on_a_hand_table():
    """Classes 0, 1: things; 2, 3, 4: stuff.  Class 1 has no count; class 3 has tp = 0 and fp > 0."""
    counts = np.asarray([[2, 0, 1, 0, 3], [1, 0, 0, 2, 0], [1, 0, 1, 0, 1]], np.int64)
    iou_sum = np.asarray([1.5, 0.0, 0.75, 0.0, 2.4])
    thing = np.asarray([True, True, False, False, False])
    got = segeval.pq_average(counts, iou_sum, thing)
    pq = [1.5 / 3.0, 0.0, 0.75 / 1.5, 0.0, 2.4 / 3.5]
    sq = [0.75, 0.0, 0.75, 0.0, 2.4 / 3]
    rq = [2 / 3.0, 0.0, 1 / 1.5, 0.0, 3 / 3.5]
    assert got["per_class"]["pq"].tolist() == pq and got["per_class"]["sq"].tolist() == sq and got["per_class"]["rq"].tolist() == rq
    assert got["All"]["n"] == 4 and got["Things"]["n"] == 1 and got["Stuff"]["n"] == 3
    assert got["Things"] == dict(pq=pq[0], sq=sq[0], rq=rq[0], n=1)
    want = PO.pq_average(counts, iou_sum, thing)
    for group in ("All", "Things", "Stuff"):
        for k in ("pq", "sq", "rq"):
            assert got[group][k] == pytest.approx(want[group][k], rel=1e-15), (group, k)
    # an empty group is NaN; without isthing only "All"
    none = segeval.pq_average(counts, iou_sum, np.zeros(5, bool))
    assert none["Things"]["n"] == 0 and all(np.isnan(none["Things"][k]) for k in ("pq", "sq", "rq")) and none["Stuff"]["n"] == 4
    assert set(segeval.pq_average(counts, iou_sum)) == {"All", "per_class"}
    assert segeval.pq_average(torch.from_numpy(counts), torch.from_numpy(iou_sum))["All"] == got["All"]
    for bad in (dict(counts=counts[:2]), dict(counts=counts.astype(np.float64)), dict(iou_sum=iou_sum[:4]), dict(isthing=np.zeros(4, bool)),
                dict(isthing=np.zeros(5, np.int32))):
        with pytest.raises(ValueError, match="segeval"):
            segeval.pq_average(**dict(dict(counts=counts, iou_sum=iou_sum), **bad))


# ---- remap --------------------------------------------------------------------------------------------------------------------------------------
def remap_cases():
    """-> (ids per image, sizes, segments): an RGB triple's id, id 0, an id the table lacks, tables of 1 and of 1000 keys with their first
    and last key."""
    rng = np.random.default_rng(5)
    big = sorted(rng.choice(np.arange(1, 2 ** 24), 1000, replace=False).tolist())
    order = rng.permutation(1000)                                     # annotation order is not id order
    seg_big = [(big[i], int(i % 7), int(i % 11 == 0)) for i in order]
    a = np.asarray([[197121, 0, 5, 197121, 77, 0, 5]], np.int64)     # 5 and 77 are not listed
    b = rng.choice(np.asarray(big + [0, 3]), (33, 65)).astype(np.int64)
    b[0, 0], b[0, 1] = big[0], big[-1]
    c = np.full((2, 64), 9, np.int64)
    return [a, b, c], [(1, 7), (33, 65), (2, 64)], [[(197121, 2, 0)], seg_big, []]


def to_rgb(ids: np.ndarray) -> np.ndarray:
    return np.stack([ids % 256, ids // 256 % 256, ids // 65536], axis=-1).astype(np.uint8)


def check_remap(dev: str) -> None:
    ids, sizes, segments = remap_cases()
    assert PO.rgb2id(np.asarray([1, 2, 3], np.uint8)) == 197121
    want = [PO.remap(m, s) for m, s in zip(ids, segments)]
    flat = np.concatenate([m.reshape(-1) for m in ids])
    out, unknown, status = PO.run_remap(flat.astype(np.int32), sizes, segments, dev)
    assert status == 0 and unknown.tolist() == [w[1] for w in want] == [3, int((ids[1] == 3).sum()), 128]
    assert np.array_equal(out, np.concatenate([w[0].reshape(-1) for w in want]))
    assert out[0] == 1 and out[1] == 0 and out[2] == 0
    first, last = segments[1].index(next(s for s in segments[1] if s[0] == min(x[0] for x in segments[1]))), None
    assert out[7] == first + 1 and out[8] == [s[0] for s in segments[1]].index(max(s[0] for s in segments[1])) + 1
    rgb_out, rgb_unknown, rgb_status = PO.run_remap(to_rgb(flat), sizes, segments, dev, rgb=True)
    assert rgb_status == 0 and np.array_equal(rgb_out, out) and np.array_equal(rgb_unknown, unknown)
    # a bad size and a bad table slice: the image keeps the fill, status 1
    dims, off, _ = PO.label_tables(sizes)
    d = dims.copy(); d[1] = (33, 0)
    out2, unknown2, status2 = PO.run_remap(flat.astype(np.int32), sizes, segments, dev, dims=d)
    assert status2 == 1 and (out2[7:7 + 33 * 65] == PO.FILL_I32).all() and np.array_equal(out2[:7], out[:7]) and unknown2.tolist()[1] == 0
    tab = np.asarray([0, 1, 1002, 1001], np.int64)
    out3, _, status3 = PO.run_remap(flat.astype(np.int32), sizes, segments, dev, tab_off=tab)
    assert status3 == 1 and (out3[7:] == PO.FILL_I32).all() and np.array_equal(out3[:7], out[:7])


def test_remap_host_entry():
    check_remap(DEV)


def test_segments_request():
    keys, vals, off, cat, crowd = pq_segments_request([[(9, 1, 0), (3, 2, 1)], [], [(5, 0, 0)]], 3)
    assert keys.tolist() == [3, 9, 5] and vals.tolist() == [2, 1, 1] and off.tolist() == [0, 2, 2, 3]
    assert cat.tolist() == [[-1, 1, 2], [-1, -1, -1], [-1, 0, -1]] and crowd.tolist() == [[0, 0, 1], [0, 0, 0], [0, 0, 0]]
    for bad in ([[(9, 1, 0), (9, 2, 0)]], [[(0, 1, 0)]], [[(2 ** 24, 1, 0)]], [[(1, -1, 0)]], [[(1, 1, 2)]], [[(1, 1)]], [[(1.5, 1, 0)]], [], "x"):
        with pytest.raises(ValueError, match="panoptic_remap"):
            pq_segments_request(bad, 1)


# ---- the pair histogram, the matching and the totals on the host entries -------------------------------------------------------------------
def test_widths_and_heights():
    PO.case_widths_and_heights(DEV)


@pytest.mark.parametrize("which", range(5))
def test_slot_shapes_on_both_sides_of_the_lds_bound(which):
    G, S = PO.slot_shapes()[which]
    assert which < 3 or G * S == hip.pan_lds_cells() + (which == 4)
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


def test_matching_finds_true_positives_on_shifted_maps():
    """The generator of the benchmark's ground truth: the prediction relabelled and shifted, so that most pairs match with IoU < 1."""
    pred, gt, pred_cat, gt_cat, gt_crowd = PO.shifted(PO.RAGGED[1:], 20, 61, 3)
    run = PO.Run(PO.RAGGED[1:], gt_cat.shape[1], pred_cat.shape[1], 61, DEV)
    got = run.score(pred, pred_cat, gt, gt_cat, gt_crowd)
    PO.compare(got, PO.pq_compute(pred, pred_cat, gt, gt_cat, gt_crowd, 61))
    iou = got["pred_iou"][got["pred_match"] > 0]
    assert len(iou) > 10 and (iou < 1.0).any() and got["counts"][1].sum() > 0 and got["counts"][2].sum() > 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_pan_entries_refuse_bad_arguments_without_gpu():
    lib = hip.load()
    p = 1 << 20
    step = 1 << 16
    names = ("raw", "dims", "off", "keys", "vals", "tab", "out", "unknown", "status", "pred", "gt", "inter", "pred_cat", "gt_cat", "crowd",
             "pred_match", "pred_iou", "gt_match", "pred_area", "gt_area", "counts", "iou_sum")
    ok = dict({n: p + i * step for i, n in enumerate(names)}, rgb=0, B=2, G=3, S=4, C=5, n_pix=100, max_pixels=64, n_keys=6, zero=1)
    args = {"cvlm_pan_remap": ("raw", "rgb", "B", "dims", "off", "n_pix", "max_pixels", "keys", "vals", "tab", "n_keys", "out", "unknown", "status"),
            "cvlm_pan_pair_hist": ("pred", "gt", "B", "G", "S", "dims", "off", "n_pix", "max_pixels", "zero", "inter", "status"),
            "cvlm_pan_match": ("inter", "B", "G", "S", "pred_cat", "gt_cat", "crowd", "C", "pred_match", "pred_iou", "gt_match", "pred_area", "gt_area"),
            "cvlm_pan_accumulate": ("B", "G", "S", "pred_cat", "gt_cat", "pred_match", "pred_iou", "gt_match", "C", "zero", "counts", "iou_sum")}
    eight = {"off", "tab", "pred_iou", "counts", "iou_sum"}           # 8-byte aligned; the others 4, gt_crowd and an RGB raw 1
    ranges = [dict(B=0), dict(B=65536)]
    slots = [dict(G=0), dict(S=0), dict(G=4097, S=4096), dict(G=2 ** 24, S=2)]
    classes = [dict(C=0), dict(C=65537)]
    pixels = [dict(n_pix=0), dict(max_pixels=0), dict(max_pixels=2 ** 28 + 1)]
    bad = {"cvlm_pan_remap": ranges + pixels + [dict(rgb=2), dict(rgb=-1), dict(n_keys=0)],
           "cvlm_pan_pair_hist": ranges + pixels + slots, "cvlm_pan_match": ranges + slots + classes,
           "cvlm_pan_accumulate": ranges + slots + classes}
    # every output against an input and against another output: the first byte, the last byte
    overlaps = {"cvlm_pan_remap": [dict(out=ok["raw"] + 396), dict(out=ok["keys"] + 20), dict(unknown=ok["out"] + 396), dict(status=ok["unknown"] + 4),
                                   dict(out=ok["tab"] + 20), dict(unknown=ok["dims"] + 12), dict(status=ok["vals"])],
                "cvlm_pan_pair_hist": [dict(inter=ok["pred"] + 396), dict(inter=ok["gt"] - 92), dict(status=ok["inter"] + 92), dict(status=ok["off"] + 20)],
                "cvlm_pan_match": [dict(pred_match=ok["inter"] + 92), dict(pred_iou=ok["pred_cat"] + 24), dict(gt_match=ok["crowd"] + 4),
                                   dict(gt_area=ok["gt_match"] + 20), dict(pred_area=ok["pred_iou"] + 56), dict(gt_area=ok["gt_cat"] - 20)],
                "cvlm_pan_accumulate": [dict(counts=ok["pred_iou"] + 56), dict(iou_sum=ok["counts"] + 112), dict(counts=ok["gt_match"] + 16),
                                        dict(iou_sum=ok["pred_cat"] - 32)]}

    def call(name, k, host):
        fn = getattr(lib, ("cvlm_debug_" + name[5:] + "_host") if host else name)
        a = [k[n] for n in args[name]]
        return fn(*a) if host else fn(*a, None)

    for name, params in args.items():
        cases = list(bad[name]) + overlaps[name]
        for n in params:
            if n not in names:
                continue
            cases.append({n: None})
            if n == "crowd":
                continue
            cases.append({n: ok[n] + (4 if n in eight else 2)})
        for kw in cases:
            for host in (False, True):
                assert call(name, dict(ok, **kw), host) == -1, (name, kw, host)
    # an RGB raw needs no alignment, an int32 raw does: the odd base is refused only without rgb (the host entry then runs: real memory)
    raw = torch.zeros(16, dtype=torch.uint8)
    z = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt)
    dims, off, keys, vals, tab = torch.tensor([[1, 4]], dtype=torch.int32), torch.tensor([0, 4]), z(1) + 7, z(1) + 1, torch.tensor([0, 1])
    out, unknown, status = z(4), z(1), z(1)
    a = lambda base, rgb: (base, rgb, 1, dims.data_ptr(), off.data_ptr(), 4, 4, keys.data_ptr(), vals.data_ptr(), tab.data_ptr(), 1,
                           out.data_ptr(), unknown.data_ptr(), status.data_ptr())
    raw[1:13] = torch.tensor([7, 0, 0, 0, 0, 0, 8, 0, 0, 7, 0, 0], dtype=torch.uint8)
    assert lib.cvlm_debug_pan_remap_host(*a(raw.data_ptr() + 1, 1)) == 0 and out.tolist() == [1, 0, 0, 1] and unknown.tolist() == [1]
    assert lib.cvlm_debug_pan_remap_host(*a(raw.data_ptr() + 1, 0)) == -1
    assert lib.cvlm_debug_pan_lds_cells() == hip.pan_lds_cells() > 0


# ---- the Python side: every ValueError before any launch --------------------------------------------------------------------------------------
class Recorder:
    """Stands where the launchers stand and records what reaches them."""

    def __init__(self, monkeypatch):
        self.calls = []
        for name in ("pan_remap", "pan_pair_hist", "pan_match", "pan_accumulate", "label_lookup"):
            monkeypatch.setattr(hip, name, lambda *a, _n=name, **k: self.calls.append(_n))


class Host(MaskUtilities):
    device = torch.device("cpu")


def test_pq_request_raises_before_any_launch(monkeypatch):
    rec = Recorder(monkeypatch)
    pc, gc, gw = [[-1, 0, 1], [-1, 2, -1]], [[-1, 0], [-1, 1]], [[0, 0], [0, 1]]
    ok = dict(pred_cat=pc, gt_cat=gc, gt_crowd=gw, sizes=[(4, 5), (6, 7)], num_classes=3, n_pred=62, n_gt=62, who="caller")
    sizes, a, b, c, G, S = pq_request(**ok)
    assert sizes == [(4, 5), (6, 7)] and (G, S) == (2, 3) and a.dtype == np.int32 and b.dtype == np.int32 and c.dtype == np.uint8
    assert pq_request(**dict(ok, gt_crowd=np.asarray(gw, bool)))[3].tolist() == gw
    wide = np.full((2, 4097), -1, np.int32)
    bad = [dict(num_classes=0), dict(num_classes=65537), dict(num_classes=3.0), dict(num_classes=True), dict(sizes=None), dict(sizes=[(4, 5)]),
           dict(sizes=[(4, 5), (0, 7)]), dict(sizes=[]), dict(n_pred=61), dict(n_gt=63), dict(n_pred=60, n_gt=60),
           dict(pred_cat=[[-1, 0, 3], [-1, 2, -1]]), dict(pred_cat=[[-1, 0, -2], [-1, 2, -1]]), dict(gt_cat=[[-1, 3], [-1, 1]]),
           dict(pred_cat=[[0, 0, 1], [-1, 2, -1]]), dict(gt_cat=[[-1, 0], [1, 1]]), dict(pred_cat=[[-1, 0, 1]]), dict(pred_cat=[-1, 0, 1]),
           dict(pred_cat=np.asarray(pc, np.float32)), dict(pred_cat=np.asarray(pc) > 0), dict(pred_cat="abc"), dict(pred_cat=np.zeros((2, 0), np.int32)),
           dict(gt_cat=[[-1, 0, 1], [-1, 1, 2]]), dict(gt_crowd=[[0, 0, 0], [0, 1, 0]]), dict(gt_crowd=[[0, 2], [0, 1]]),
           dict(gt_crowd=[[0.0, 0.0], [0.0, 1.0]]), dict(pred_cat=wide, gt_cat=wide[:, :4096], gt_crowd=np.zeros((2, 4096), np.uint8))]
    for kw in bad:
        with pytest.raises(ValueError, match="caller"):
            pq_request(**dict(ok, **kw))
    assert rec.calls == []


def test_panoptic_calls_raise_before_any_launch(monkeypatch):
    rec = Recorder(monkeypatch)
    eng = Host()
    sizes = [(4, 5), (6, 7)]
    raw = np.zeros(62, np.int32)
    segs = [[(5, 1, 0)], [(7, 2, 1), (9, 0, 0)]]
    bad = [dict(rgb=1), dict(sizes=None), dict(sizes=sizes[:1]), dict(segments=segs[:1]), dict(segments=[[(5, 1, 0), (5, 2, 0)], []]),
           dict(segments=[[(0, 1, 0)], []]), dict(raw=np.zeros(61, np.int32)), dict(raw=np.zeros(62, np.float32)), dict(raw=[0] * 62),
           dict(raw=np.zeros((62, 3), np.int32), rgb=True), dict(raw=np.zeros((62, 4), np.uint8), rgb=True), dict(raw=np.zeros(0, np.int32)),
           dict(raw=np.full(62, 2 ** 31, np.int64))]
    for kw in bad:
        k = dict(dict(raw=raw, sizes=sizes, segments=segs, rgb=False), **kw)
        with pytest.raises(ValueError, match="panoptic_remap"):
            eng.panoptic_remap(k.pop("raw"), k.pop("sizes"), k.pop("segments"), **k)
    assert rec.calls == []
    gt = eng.panoptic_remap([np.zeros((4, 5), np.int64), np.zeros((6, 7), np.int64)], sizes, segs)
    assert isinstance(gt, PanopticGroundTruth) and rec.calls == ["pan_remap"] and gt.gt.shape == (62,) and gt.unknown.shape == (2,)
    assert gt.gt_cat.tolist() == [[-1, 1, -1], [-1, 2, 0]] and gt.gt_crowd.tolist() == [[0, 0, 0], [0, 1, 0]]
    assert eng.panoptic_remap(np.zeros((62, 3), np.uint8), sizes, segs, rgb=True).gt.shape == (62,)
    rec.calls.clear()
    pred, pred_cat = np.zeros(62, np.int32), [[-1, 0], [-1, 1]]
    ok = dict(pred=pred, pred_cat=pred_cat, gt=gt.gt, gt_cat=gt.gt_cat, gt_crowd=gt.gt_crowd, sizes=sizes, num_classes=3)
    other = eng.panoptic_quality(**dict(ok, num_classes=4))
    assert isinstance(other, PanopticTotals) and rec.calls == ["pan_pair_hist", "pan_match", "pan_accumulate"]
    assert other.counts.shape == (3, 4) and other.inter.shape == (2, 3, 2) and other.pred_iou.dtype == torch.float64
    rec.calls.clear()
    bad = [dict(num_classes=0), dict(pred=np.zeros(61, np.int32)), dict(pred=np.zeros(62, np.float32)), dict(gt=np.zeros(63, np.int32)),
           dict(sizes=[(4, 5), (6, 8)]), dict(pred_cat=[[-1, 3], [-1, 1]]), dict(pred_cat=[[0, 0], [-1, 1]]), dict(gt_cat=gt.gt_cat[:, :2]),
           dict(gt_crowd=gt.gt_crowd[:1]), dict(totals=other), dict(totals=other.counts), dict(pred=None)]
    for kw in bad:
        with pytest.raises(ValueError, match="panoptic_quality"):
            eng.panoptic_quality(**dict(ok, **kw))
    assert rec.calls == []
    again = eng.panoptic_quality(**dict(ok, num_classes=4, totals=other))
    assert again.counts is other.counts and again.iou_sum is other.iou_sum and again.status is other.status and again.inter is not other.inter


def test_containers():
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt)
    t = PanopticTotals(counts=z(3, 2, dt=torch.int64), iou_sum=z(2, dt=torch.float64), status=z(1), inter=z(1, 2, 2), pred_match=z(1, 2),
                       pred_iou=z(1, 2, dt=torch.float64), gt_match=z(1, 2), pred_area=z(1, 2), gt_area=z(1, 2), num_classes=2)
    t.check()
    host = t.to_host()
    assert host["counts"].shape == (3, 2) and host["status"] == 0 and host["pred_iou"].dtype == np.float64
    for code, word in ((1, "refused"), (2, "outside"), (3, "refused")):
        t.status[0] = code
        with pytest.raises(RuntimeError, match=word):
            t.check()
    g = PanopticGroundTruth(gt=z(4), unknown=z(1), gt_cat=np.zeros((1, 1), np.int32), gt_crowd=np.zeros((1, 1), np.uint8), status=z(1), sizes=[(2, 2)])
    g.check()
    g.status[0] = 1
    with pytest.raises(RuntimeError, match="panoptic_remap"):
        g.check()


def test_pq_inputs_checks_its_labels(monkeypatch):
    from camouflaged_vlm_amd.engine import LabelMaps, label_tables
    rec = Recorder(monkeypatch)
    dims, off, _ = label_tables([(4, 5), (6, 7)])
    z16 = torch.zeros(62, dtype=torch.int16)
    m = LabelMaps(score=torch.zeros(62), winner=z16, segment=z16.clone(), areas=torch.zeros(3, 6, dtype=torch.int32),
                  segment_id=torch.zeros(6, dtype=torch.int32), n_segments=torch.zeros(2, dtype=torch.int32), status=torch.zeros(1, dtype=torch.int32),
                  dims=torch.from_numpy(dims), pix_offsets=torch.from_numpy(off), sizes=[(4, 5), (6, 7)], K=3)
    for labels in ([[0, 1], [1, 2]], [[0.0, 1, 2], [1, 2, 3]], [0, 1, 2]):
        with pytest.raises(ValueError, match="pq_inputs"):
            m.pq_inputs(labels)
    assert rec.calls == []
    pred, pred_cat = m.pq_inputs([[5, 6, 7], [7, 6, 5]])
    assert rec.calls == ["label_lookup"] and pred.shape == (62,) and pred.dtype == torch.int32
    assert pred_cat.tolist() == [[-1, 5, 6, 7], [-1, 7, 6, 5]] and pred_cat.dtype == torch.int32
