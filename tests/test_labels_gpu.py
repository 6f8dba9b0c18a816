"""Label maps on the device: the cvlm_label_* kernels against the oracle (tests/labels_oracle.py: the published loops) and
against the host entries -- blocky +-30 planes with dyadic weights exactly, no pixel left out: every width around the unit of 64
pixels x heights 1, 2, 33, enlarged and reduced from three source sizes, seven ragged images in one call at K = 1, 2, 5, 64, 65, the
same planes cut into calls of 4 at K = 3, every kind of weight, +-inf and NaN planes, used outputs, guard bands, a logits base off 16
bytes; `winner` on smooth logits under the measured margin of the oracle module; everything behind the argmax exactly against the
published loop on the device's own winner map and the device's own sized bits; the lookup; the histogram on both of its paths; the
refusals; Cascade.label_maps / label_iou and label_maps=True of infer_classes / decode on the tiny geometry.

Figures of the MI355X run this file was written with are in DESIGN.md §23."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import labels_oracle as LO
import sized_oracle as SO
from test_classes_gpu import build_tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SOURCES = [(64, 64), (96, 128), (32, 64)]


def both(logits, sizes, weights=None, level=128, thr=0.8, cuts=None, exact=True):
    """The device's outputs, held against the oracle under the rule and -- on exact inputs -- against the host entries' outputs."""
    got = LO.run(logits, sizes, weights, level, thr, dev=DEV, cuts=cuts)
    LO.compare(got, logits, sizes, weights, level, thr, exact=exact, dev=DEV)
    if exact:
        host = LO.run(logits, sizes, weights, level, thr)
        for name in ("winner", "segment"):
            assert all(np.array_equal(a, b) for a, b in zip(got[name], host[name])), name
        for name in ("orig_area", "won_area", "kept_area", "segment_id", "n_segments"):
            assert np.array_equal(got[name], host[name]), name
    return got


# ---- the kernels: exact ------------------------------------------------------------------------------------------------------------------
def test_every_width_and_height_is_exact():
    i = 0
    for w in SO.GEOMETRY_WIDTHS:
        for h in SO.GEOMETRY_HEIGHTS:
            Hs, Ws = SOURCES[i % 3]
            both(LO.blocky(1, 3, Hs, Ws, 100 * h + w), [(h, w)], LO.dyadic(1, 3))
            i += 1


@pytest.mark.parametrize("src,dsts", [((64, 64), [(97, 131), (33, 31)]), ((96, 128), [(150, 201), (50, 70)]), ((32, 64), [(70, 133), (16, 20)])])
def test_enlarged_and_reduced_are_exact(src, dsts):
    logits = LO.blocky(2, 4, *src, seed=src[0])
    both(logits, dsts, LO.dyadic(2, 4))
    both(logits, dsts, LO.dyadic(2, 4), level=1, thr=0.5)
    both(logits, dsts, None, level=255, thr=1.0)


def test_known_answers():
    """tests/test_labels_cpu.py's worked example (areas 80 / 32, won 48 / 80), equal planes, a NaN plane, an image of NaN planes."""
    col = lambda x0, x1: np.where((np.arange(16) >= x0) & (np.arange(16) < x1), np.float32(30), np.float32(-30))[None].repeat(8, 0)
    logits = np.stack([col(0, 10), col(6, 10)])[None].astype(np.float32)
    for thr, ids in ((0.5, [1, 2]), (0.8, [0, 1])):
        got = both(logits, [(8, 16)], [[0.5, 1.0]], thr=thr)
        assert got["orig_area"].tolist() == [[80, 32]] and got["won_area"].tolist() == [[48, 80]] and got["kept_area"].tolist() == [[48, 32]]
        assert got["segment_id"].tolist() == [ids]
    one = SO.blocky(24, 40, 5)
    for cuts in (None, [1], [1, 2]):
        got = both(np.stack([one, one, one])[None], [(33, 65)], [[0.5, 0.5, 0.5]], cuts=cuts)
        assert (got["winner"][0] == 0).all()
    nan = np.full((24, 40), np.nan, np.float32)
    got = both(np.stack([nan, one, nan])[None], [(33, 65)], [[4.0, 0.25, 4.0]])
    assert (got["winner"][0] == 1).all() and got["segment_id"].tolist() == [[0, 1, 0]]
    got = both(np.stack([np.stack([nan, nan]), LO.blocky(1, 2, 24, 40, 7)[0]]), [(5, 65), (33, 31)])
    assert (got["winner"][0] == -1).all() and (got["segment"][0] == -1).all() and got["n_segments"].tolist()[0] == 0


@pytest.mark.parametrize("K", [1, 2, 5, 64, 65])
def test_ragged_images_in_one_call(K):
    both(LO.blocky(7, K, 24, 40, 11 * K), LO.RAGGED, LO.dyadic(7, K), thr=0.5)


def test_any_cut_into_calls_gives_the_same_outputs():
    logits = LO.blocky(7, 3, 24, 40, 77)
    wts = LO.dyadic(7, 3)
    whole = both(logits, LO.RAGGED, wts, thr=0.5)
    for cuts in (list(range(4, 21, 4)), list(range(1, 21))):
        other = both(logits, LO.RAGGED, wts, thr=0.5, cuts=cuts)
        for name, a in whole.items():
            b = other[name]
            same = all(np.array_equal(x, y) for x, y in zip(a, b)) if isinstance(a, list) else np.array_equal(a, b)
            assert same, name                                        # the scores too: a pixel's state does not depend on the cut


def test_more_planes_than_one_tile_of_counters():
    """K above the 1024 planes a workgroup counts in LDS at a time: the state passes from one tile to the next inside a call."""
    rng = np.random.default_rng(3)
    K = 1030
    on = rng.random((1, K, 4, 8)) < 0.3
    logits = np.where(on, np.float32(30), np.float32(-30)).astype(np.float32)
    wts = (1.0 + (np.arange(K) % 7) / 8.0).astype(np.float32)[None]
    both(logits, [(5, 70)], wts, thr=0.5)


@pytest.mark.parametrize("kind", ["null", "equal", "zero", "negative", "nan", "nan_all", "inf_planes"])
def test_weights_and_values(kind):
    logits = LO.blocky(2, 4, 24, 40, 21)
    wts = {"null": None, "equal": np.full((2, 4), 0.75), "zero": np.zeros((2, 4)), "negative": -LO.dyadic(2, 4),
           "nan": np.asarray([[1.0, np.nan, 0.5, np.nan], [np.nan, 2.0, 2.0, 0.25]]), "nan_all": np.full((2, 4), np.nan),
           "inf_planes": LO.dyadic(2, 4)}[kind]
    if kind == "inf_planes":
        logits = np.where(logits > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
    got = both(logits, [(33, 65), (70, 33)], wts, thr=0.5)
    if kind == "nan_all":
        assert all((w == -1).all() for w in got["winner"]) and got["n_segments"].tolist() == [0, 0]


def test_used_outputs_and_an_unaligned_base():
    logits = LO.blocky(7, 2, 24, 40, 5)
    st = LO.State(LO.RAGGED, 2, DEV)
    first = LO.run(logits, LO.RAGGED, LO.dyadic(7, 2), dev=DEV, state=st)
    LO.compare(first, logits, LO.RAGGED, LO.dyadic(7, 2), exact=True, dev=DEV)
    other = LO.run(LO.blocky(7, 2, 24, 40, 6), LO.RAGGED, None, dev=DEV, state=st)
    again = LO.run(logits, LO.RAGGED, LO.dyadic(7, 2), dev=DEV, state=st)
    assert not np.array_equal(first["won_area"], other["won_area"])
    for name in ("winner", "segment", "score"):
        assert all(np.array_equal(a, b) for a, b in zip(first[name], again[name])), name
    for name in ("orig_area", "won_area", "kept_area", "segment_id", "n_segments"):
        assert np.array_equal(first[name], again[name]), name
    flat = torch.zeros(14 * 24 * 40 + 5, dtype=torch.float32, device=DEV)
    base = (-flat.data_ptr() // 4) % 4
    off = flat[base + 1:base + 1 + 14 * 24 * 40].view(14, 24, 40)
    assert off.data_ptr() % 16 == 4
    off.copy_(torch.from_numpy(logits.reshape(14, 24, 40)))
    st.init()
    st.accumulate(off, 0, LO.dyadic(7, 2))
    st.finish()
    shifted = st.read()
    assert all(np.array_equal(a, b) for a, b in zip(first["winner"], shifted["winner"])) and np.array_equal(first["segment_id"], shifted["segment_id"])


# ---- the one inexact comparison ------------------------------------------------------------------------------------------------------------
def test_smooth_logits_under_the_measured_margin():
    for logits, (h, w), wts in LO.smooth_cases():
        both(logits, [(h, w)], wts, thr=0.5, exact=False)
        got = LO.run(logits, [(h, w)], wts, overlap_threshold=0.5, dev=DEV)
        host = LO.run(logits, [(h, w)], wts, overlap_threshold=0.5)
        near = LO.near_ties(logits[0], h, w, wts[0])
        print(f"{(h, w)}: device and host entry differ at {int((got['winner'][0] != host['winner'][0]).sum())} pixels, {int(near.sum())} near a tie")
        assert np.array_equal(got["winner"][0][~near], host["winner"][0][~near])


# ---- lookup ----------------------------------------------------------------------------------------------------------------------------------
def test_lookup_equals_the_definition_on_the_device_s_own_maps():
    logits = LO.blocky(7, 5, 24, 40, 13)
    nan = np.full((24, 40), np.nan, np.float32)
    logits[4] = nan                                                  # an image without a winner: void everywhere
    st = LO.State(LO.RAGGED, 5, DEV)
    got = LO.run(logits, LO.RAGGED, LO.dyadic(7, 5), overlap_threshold=0.5, dev=DEV, state=st)
    table = np.random.default_rng(1).integers(-5, 1000, (7, 5)).astype(np.int32)
    for which, tab, void in (("winner", table, 255), ("segment", table, -9), ("segment", got["segment_id"], 0)):
        out = st.lookup(which, tab, void)
        for b, (h, w) in enumerate(LO.RAGGED):
            m = got[which][b].astype(np.int64)
            want = np.where(m < 0, void, np.asarray(tab)[b][np.maximum(m, 0)])
            assert np.array_equal(out[st.host_off[b]:st.host_off[b + 1]].reshape(h, w), want), (which, b)
    assert st.read()["status"] == 0
    pan = st.lookup("segment", got["segment_id"], 0)
    assert pan.max() == got["n_segments"].max() and (pan[st.host_off[4]:st.host_off[5]] == 0).all()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_a_refused_image_stays_at_the_fill_and_its_neighbours_whole():
    logits = LO.blocky(7, 2, 24, 40, 9)
    wts = LO.dyadic(7, 2)
    good = LO.run(logits, LO.RAGGED, wts, overlap_threshold=0.5, dev=DEV)
    dims, off, _ = LO.tables(LO.RAGGED)
    cases = []
    bad = off.copy(); bad[3:] += 1
    cases.append(dict(offsets=bad, skipped=(2,), n_pix=int(off[-1]) + 1))
    bad = off.copy(); bad[2] -= 1
    cases.append(dict(offsets=bad, skipped=(1, 2)))
    for hw in ((0, 65), (5, 0), (-5, 65), (5, 16385), (2 ** 31 - 1, 2 ** 31 - 1)):
        d = dims.copy(); d[2] = hw
        cases.append(dict(dims=d, skipped=(2,)))
    cases.append(dict(n_pix=int(off[-1]) - 1, skipped=(6,)))
    bad = off.copy(); bad[0] = -1
    cases.append(dict(offsets=bad, skipped=(0,)))
    for case in cases:
        st = LO.State(LO.RAGGED, 2, DEV, n_pix=case.get("n_pix"))
        d = st.dims if "dims" not in case else torch.from_numpy(case["dims"]).to(DEV)
        o = st.off if "offsets" not in case else torch.from_numpy(case["offsets"]).to(DEV)
        st.init()
        st.accumulate(torch.from_numpy(logits.reshape(14, 24, 40)).to(DEV), 0, wts, dims=d, off=o)
        st.finish(0.5, dims=d, off=o)
        used = np.asarray(case.get("offsets", off))
        st.host_off = used
        got = st.read()
        assert got["status"] == 1, case
        for b in range(7):
            if b in case["skipped"]:
                lo, hi = max(int(used[b]), 0), min(int(used[b + 1]), st.n)
                assert (st.winner[lo:hi] == -1).all() and (st.segment[lo:hi] == -1).all() and (st.score[lo:hi] == 0).all(), (case, b)
                assert not got["orig_area"][b].any() and not got["won_area"][b].any() and not got["segment_id"][b].any()
                assert got["n_segments"][b] == 0
            else:
                assert np.array_equal(got["winner"][b], good["winner"][b]) and np.array_equal(got["segment"][b], good["segment"][b]), (case, b)
                assert np.array_equal(got["segment_id"][b], good["segment_id"][b]) and np.array_equal(got["orig_area"][b], good["orig_area"][b])
        if "dims" in case:                                           # the lookup refuses the same image and writes nothing of it
            from camouflaged_vlm_amd import hip
            out = torch.full((st.n,), LO.FILL_I32, dtype=torch.int32, device=DEV)
            hip.label_lookup(st.winner, 7, 2, d, st.off, st.max_pixels, torch.arange(14, dtype=torch.int32, device=DEV), 255, out, st.status)
            assert (out[int(off[2]):int(off[3])] == LO.FILL_I32).all() and (out[:int(off[2])] != LO.FILL_I32).all()


# ---- the histogram -----------------------------------------------------------------------------------------------------------------------------
def device_hist(pred, gt, C, ignore_index=255, reduce_zero_label=False, totals=None):
    from camouflaged_vlm_amd import hip
    fresh = totals is None
    if fresh:
        totals = torch.full((3, C), -5, dtype=torch.int64, device=DEV)
    hip.label_iou_hist(torch.from_numpy(np.ascontiguousarray(pred, dtype=np.int32)).to(DEV), torch.from_numpy(np.ascontiguousarray(gt)).to(DEV),
                       C, ignore_index, reduce_zero_label, fresh, totals)
    return totals


@pytest.mark.parametrize("C", [3, 150, 4096, 4097])                   # 4096: the last C of the LDS path; 4097: wave-aggregated global atomics
@pytest.mark.parametrize("gt_dtype", [np.uint8, np.int32])
def test_histogram_equals_the_definition(C, gt_dtype):
    rng = np.random.default_rng(C)
    for n in (1, 63, 4133, 300001):                                   # one pixel; no multiple of 64; more than one workgroup
        top = min(C, 255) if gt_dtype is np.uint8 else C
        gt = rng.integers(0, top + 1, n).astype(gt_dtype)
        if gt_dtype is np.int32:
            gt[rng.random(n) < 0.05] = -3
        gt[rng.random(n) < 0.1] = 255
        pred = np.where(rng.random(n) < 0.6, gt.astype(np.int64), rng.integers(-1, C + 2, n)).astype(np.int32)
        for reduce in (False, True):
            want = LO.intersect_and_union(pred, gt, C, 255, reduce)
            assert np.array_equal(device_hist(pred, gt, C, 255, reduce).cpu().numpy(), want), (n, reduce)
        if n > 1:                                                    # two calls accumulate to one call over the concatenation
            t = device_hist(pred[:n // 3], gt[:n // 3], C, ignore_index=0)
            t = device_hist(pred[n // 3:], gt[n // 3:], C, ignore_index=0, totals=t)
            assert np.array_equal(t.cpu().numpy(), LO.intersect_and_union(pred, gt, C, 0))


# ---- tiny geometry, exact ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(golden_dir):
    with np.load(os.path.join(golden_dir, "tiny_classes.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def tiny():
    from camouflaged_vlm_amd import spec, synth
    g, c = spec.TINY_SAM, spec.TINY_CLIP
    inp, ci, cm = synth.make_inputs(g, c, batch=2)
    dev = torch.device(DEV)
    return g, c, synth.make_full_state_dict(g, c), tuple(torch.from_numpy(t).to(dev) for t in (inp, ci, cm)), dev


@pytest.fixture(scope="module")
def cas(tiny, gold):
    return build_tiny(tiny, gold)


@pytest.fixture(scope="module")
def tracer():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "trace_mask_launches.py")
    spec = importlib.util.spec_from_file_location("trace_mask_launches", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SIZES = [(213, 320), (480, 641)]
CLASSES = [[0, 1, 2], [2, 1, 0]]                                      # K = 3: a chunk of 4 crosses the image boundary
# distinct per image, the largest 1.0: the top of the range LO.MARGIN, an absolute figure, holds for.  On the tiny model's planes 2 and 15
# pixels of the two images lie within the margin of a tie (the cap is 6 and 30)
WEIGHTS = [[1.0, 0.6, 0.4], [0.5, 0.75, 1.0]]


def as_read(m) -> dict:
    """A LabelMaps in the form of State.read()."""
    h = m.to_host()
    B, K = m.B, m.K
    score = m.score.cpu().numpy()
    return dict(h, score=[score[slice(*m._range(b))].reshape(m.sizes[b]) for b in range(B)])


def check_label_maps(m, masks: torch.Tensor, sizes, weights, thr: float = 0.8, exact: bool = False):
    """The maps of a call against the oracle on the call's own `masks` (n, K, S, S), under the rule of the smooth comparison (exact:
    blocky planes, every pixel held)."""
    from camouflaged_vlm_amd.engine import LabelMaps
    assert isinstance(m, LabelMaps) and m.sizes == [tuple(s) for s in sizes] and m.K == masks.shape[1] and m.level == 128
    m.check()
    got = as_read(m)
    LO.compare(got, masks.cpu().numpy(), sizes, weights, 128, thr, exact=exact, dev=DEV)
    for b, (h, w) in enumerate(sizes):
        assert m.winner_of(b).shape == (h, w) and np.array_equal(m.winner_of(b).cpu().numpy(), got["winner"][b])
        assert np.array_equal(m.segment_of(b).cpu().numpy(), got["segment"][b])
    return got


def test_cascade_label_maps_and_label_iou(cas):
    logits = torch.from_numpy(LO.blocky(7, 3, 24, 40, 31)).to(DEV)
    wts = LO.dyadic(7, 3)
    m = cas.label_maps(logits.view(21, 24, 40), LO.RAGGED, K=3, weights=wts, overlap_threshold=0.5)
    got = check_label_maps(m, logits, LO.RAGGED, wts, 0.5, exact=True)
    again = cas.label_maps(logits.view(21, 1, 24, 40), LO.RAGGED, K=3, weights=torch.from_numpy(wts).to(DEV), overlap_threshold=0.5)
    assert torch.equal(again.winner, m.winner) and torch.equal(again.segment, m.segment) and torch.equal(again.segment_id, m.segment_id)
    labels = np.arange(21).reshape(7, 3) % 5
    sem = m.categories(labels)
    pan_cat = m.categories(torch.from_numpy(labels).to(DEV), which="segment", void=-1)
    pan = m.panoptic()
    for b in range(7):
        w, s = got["winner"][b].astype(np.int64), got["segment"][b].astype(np.int64)
        assert np.array_equal(m.image_of(sem, b).cpu().numpy(), np.where(w < 0, 255, labels[b][np.maximum(w, 0)]))
        assert np.array_equal(m.image_of(pan_cat, b).cpu().numpy(), np.where(s < 0, -1, labels[b][np.maximum(s, 0)]))
        assert np.array_equal(m.image_of(pan, b).cpu().numpy(), np.where(s < 0, 0, got["segment_id"][b][np.maximum(s, 0)]))
    # scored against itself: IoU 1.0 on the classes present; against a relabelled map: the definition's totals
    from camouflaged_vlm_amd import segeval
    totals = cas.label_iou(sem, sem, num_classes=5)
    present = totals[2].cpu().numpy() > 0
    iou = segeval.eval_metrics(totals)[2]
    assert present.any() and (iou[present] == 1.0).all() and np.isnan(iou[~present]).all() and segeval.mean_iou(totals) == 1.0
    gt = sem.cpu().numpy().copy()
    gt[gt == 2] = 3
    gt[::7] = 255
    want = LO.intersect_and_union(sem.cpu().numpy(), gt, 5)
    assert np.array_equal(cas.label_iou(sem, gt.astype(np.uint8), num_classes=5).cpu().numpy(), want)
    twice = cas.label_iou(sem, torch.from_numpy(gt).to(DEV), num_classes=5, totals=cas.label_iou(sem, gt, num_classes=5))
    assert np.array_equal(twice.cpu().numpy(), 2 * want)


def test_infer_classes_and_decode_label_maps(tiny, cas, tracer, golden_dir, monkeypatch):
    from camouflaged_vlm_amd import segeval
    _, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    classes = torch.tensor(CLASSES)
    weights = torch.tensor(WEIGHTS, device=DEV)
    plain = cas.infer_classes(inp, ci, cm, classes=classes, masks="both", sizes=SIZES)
    assert plain.label_maps is None
    h = cas.infer_classes(inp, ci, cm, classes=classes, masks="both", sizes=SIZES, label_maps=True, label_weights=weights)
    torch.cuda.synchronize()
    for f in ("masks", "edges", "logits", "pred", "mask_bits", "area", "box"):           # every other field keeps its bits
        assert torch.equal(getattr(h, f).contiguous().view(torch.uint8), getattr(plain, f).contiguous().view(torch.uint8)), f
    assert torch.equal(h.sized.bits, plain.sized.bits)
    got = check_label_maps(h.label_maps, h.masks, SIZES, WEIGHTS)
    assert np.array_equal(got["orig_area"].reshape(-1), h.sized.area.cpu().numpy())
    assert sum(len(np.unique(w)) for w in got["winner"]) > 2                               # not one winner per image
    # host weights, masks="bits": the same maps without a (B, K, S, S) tensor
    bits = cas.infer_classes(inp, ci, cm, classes=classes, masks="bits", sizes=SIZES, label_maps=True, label_weights=WEIGHTS)
    assert bits.masks is None and torch.equal(bits.label_maps.winner, h.label_maps.winner)
    assert torch.equal(bits.label_maps.segment, h.label_maps.segment) and torch.equal(bits.label_maps.areas, h.label_maps.areas)
    # the semantic map scored against itself and against a map with one region relabelled
    sem = h.label_maps.categories(h.classes)
    totals = cas.label_iou(sem, sem, num_classes=4)
    present = totals[2].cpu().numpy() > 0
    assert present.any() and (segeval.eval_metrics(totals)[2][present] == 1.0).all()
    gt = sem.clone()
    region = h.label_maps.image_of(gt, 1)[100:300, 200:500]
    region[region == 1] = 3
    want = LO.intersect_and_union(sem.cpu().numpy(), gt.cpu().numpy(), 4)
    assert np.array_equal(cas.label_iou(sem, gt, num_classes=4).cpu().numpy(), want) and want[0].sum() < want[2].sum()
    # decode under the default switches: its maps against the oracle on its own planes (against infer_classes: the next test)
    enc = cas.encode(inp, ci, cm)
    d = cas.decode(enc, classes=classes, masks="both", sizes=SIZES, label_maps=True, label_weights=weights)
    check_label_maps(d.label_maps, d.masks, SIZES, WEIGHTS)
    # without the option: the launches recorded on the commit before it; with it: the same launches and the label family's
    with open(os.path.join(golden_dir, "mask_post_launches.json")) as f:
        recorded = json.load(f)
    with tracer.Recorder() as log:
        cas.infer_classes(inp, ci, cm, classes=classes, masks="bits")
        torch.cuda.synchronize()
    names = [e if isinstance(e, str) else e[0] for e in log]
    assert names == [recorded["names"][e if isinstance(e, int) else e[0]] for e in recorded["calls"]["infer_classes bits"]]
    with tracer.Recorder() as log:
        cas.infer_classes(inp, ci, cm, classes=classes, masks="bits", sizes=SIZES)
        torch.cuda.synchronize()
    without = [e if isinstance(e, str) else e[0] for e in log]
    with tracer.Recorder() as log:
        cas.infer_classes(inp, ci, cm, classes=classes, masks="bits", sizes=SIZES, label_maps=True, label_weights=weights)
        torch.cuda.synchronize()
    with_maps = [e if isinstance(e, str) else e[0] for e in log]
    assert not any(n.startswith("label_") for n in without)
    assert [n for n in with_maps if not n.startswith("label_")] == without
    assert [n for n in with_maps if n.startswith("label_")] == ["label_init", "label_accumulate", "label_accumulate", "label_finish"]


def test_decode_gives_the_maps_of_infer_classes_without_ksplits(tiny, cas, monkeypatch):
    """With the GEMM K-splits off the summation order of a GEMM no longer depends on its row count and decode(encode(x)) has the bits
    of infer_classes(x) (tests/test_session_gpu.py: `nosplit`): then the planes are equal, and so is every tensor of the label maps."""
    monkeypatch.setenv("CVLM_GEMM_TAIL", "0")
    monkeypatch.setenv("CVLM_GEMM_SK", "0")
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    _, _, _, (inp, ci, cm), _ = tiny
    classes = torch.tensor(CLASSES)
    kw = dict(classes=classes, masks="both", sizes=SIZES, label_maps=True, label_weights=WEIGHTS)
    h = cas.infer_classes(inp, ci, cm, **kw)
    d = cas.decode(cas.encode(inp, ci, cm), **kw)
    torch.cuda.synchronize()
    h.label_maps.check(), d.label_maps.check()
    assert torch.equal(d.masks, h.masks)
    for f in ("winner", "segment", "score", "areas", "segment_id", "n_segments"):
        assert torch.equal(getattr(d.label_maps, f), getattr(h.label_maps, f)), f
    assert int(h.label_maps.n_segments.sum()) > 0


def test_bad_label_requests_raise_and_launch_nothing(tiny, cas, tracer):
    _, _, _, (inp, ci, cm), _ = tiny
    enc = cas.encode(inp, ci, cm)
    torch.cuda.synchronize()
    ok = dict(masks="bits", sizes=SIZES, label_maps=True)
    bad = [dict(sizes=None), dict(masks="logits"), dict(label_weights=[1.0, 2.0]), dict(label_weights=[[1.0, float("nan")], [1.0, 1.0]]),
           dict(label_weights=torch.ones(2, 2, device=DEV, dtype=torch.float64)), dict(label_weights=torch.ones(3, 2, device=DEV)),
           dict(overlap_threshold=0.0), dict(overlap_threshold=float("nan")), dict(overlap_threshold=1.5), dict(sized_level=0),
           dict(label_maps=False, label_weights=[[1.0, 1.0], [1.0, 1.0]]), dict(label_maps="yes")]
    with tracer.Recorder() as log:
        for kw in bad:
            with pytest.raises(ValueError):
                cas.infer_classes(inp, ci, cm, topk=2, **dict(ok, **kw))
            with pytest.raises(ValueError):
                cas.decode(enc, topk=2, **dict(ok, **kw))
        logits = torch.zeros(4, 8, 8, device=DEV)
        for kw in (dict(K=3), dict(sizes=SIZES[:1]), dict(weights=[1.0]), dict(level=256), dict(overlap_threshold=-1.0),
                   dict(logits=logits.cpu()), dict(weights=torch.ones(2, 2, device=DEV, dtype=torch.float16))):
            k = dict(dict(logits=logits, sizes=SIZES, K=2), **kw)
            with pytest.raises(ValueError):
                cas.label_maps(k.pop("logits"), k.pop("sizes"), **k)
        for kw in (dict(num_classes=0), dict(pred=torch.zeros(3, device=DEV)), dict(gt=torch.zeros(4, dtype=torch.uint8, device=DEV))):
            k = dict(dict(pred=torch.zeros(3, dtype=torch.int32, device=DEV), gt=torch.zeros(3, dtype=torch.uint8, device=DEV), num_classes=3), **kw)
            with pytest.raises(ValueError):
                cas.label_iou(k.pop("pred"), k.pop("gt"), **k)
    assert log == [], log[:5]


def test_dropin_passes_label_maps_through(tiny, gold, golden_dir):
    import sys
    import camouflaged_vlm_amd as cv
    if cv.DROPIN_DIR not in sys.path:
        sys.path.insert(0, cv.DROPIN_DIR)
    import models
    from cocotrainers.mapleAlphaCLIP import CustomCLIP
    g, c, sd_np, (inp, ci, cm), dev = tiny
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
    model.cascade().class_chunk = lambda: 4
    with torch.no_grad():
        h = model.infer_classes(inp, ci, cm, topk=3, masks="both", sizes=SIZES, label_maps=True, label_weights=WEIGHTS, overlap_threshold=0.5)
        check_label_maps(h.label_maps, h.masks, SIZES, WEIGHTS, 0.5)
        enc = model.encode_images(inp, ci, cm)
        d = model.decode_classes(enc, topk=3, masks="both", sizes=SIZES, label_maps=True, label_weights=WEIGHTS)
        check_label_maps(d.label_maps, d.masks, SIZES, WEIGHTS)
        m = model.label_maps(h.masks.view(6, *h.masks.shape[-2:]), SIZES, K=3, weights=WEIGHTS, overlap_threshold=0.5)
        assert torch.equal(m.winner, h.label_maps.winner) and torch.equal(m.segment, h.label_maps.segment)
        sem = m.categories(h.classes)
        assert np.array_equal(model.label_iou(sem, sem, num_classes=4).cpu().numpy(), LO.intersect_and_union(sem.cpu().numpy(), sem.cpu().numpy(), 4))
