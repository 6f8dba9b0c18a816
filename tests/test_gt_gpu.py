"""COCO annotations on the device: cvlm_mask_rle_decode against the definition (tests/gt_oracle.py: rle.decode, itself
held against a pixel loop in tests/test_gt_cpu.py) and against the host entry on every shape and plane, ragged in one call, off a
16-byte boundary, in rounds, with zero counts, and on every refusal; cvlm_mask_inter_sized against unpackbits / & / sum; the round
trips with cvlm_mask_rle_emit_w; Cascade.rle_decode / mask_inter_sized; ground_truth= of Cascade.infer_classes / decode / the drop-in
against the oracle on the call's own planes and against the call without it.  Everything is integers and compared exactly.

Figures of the MI355X run this file was written with are in DESIGN.md §20."""
import os
import sys

import numpy as np
import pytest
import torch

import gt_oracle as GO
import rle_oracle as RO
import sized_oracle as SO
from test_classes_gpu import build_tiny
from test_gt_cpu import all_pairs, inter_refusals, items_of, ragged_items, refusal_cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def entries():
    from camouflaged_vlm_amd import hip
    return hip.mask_rle_decode, hip.mask_rle_decode_host, hip.mask_inter_sized, hip.mask_inter_sized_host


def check_items(items, **over):
    """One device call and one host call for the items: both equal the definition, and each other."""
    dec, dec_host, _, _ = entries()
    got, area, box, status = GO.run_decode(dec, items, dev=DEV, **over)
    host_over = {k: v for k, v in over.items() if k != "ws_planes"}
    want, h_area, h_box, h_status = GO.run_decode(dec_host, items, **host_over)
    assert status == h_status == 0
    for p, (c, h, w) in enumerate(items):
        GO.check_plane(got[p], area[p], box[p], GO.expected(c, h, w), h, w)
        assert np.array_equal(got[p], want[p])
    assert np.array_equal(area, h_area) and np.array_equal(box, h_box)
    return got


# ---- the decoder -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", GO.SHAPES)
def test_decode_equals_the_definition_and_the_host_entry(h, w):
    """65 x 97 in period-2 stripes has 6 305 counts, more than one slab of the count walk; 130 x 517 has 2 101 stream words, more than
    one slab of the prefix pass.  Without statistics the bits are the same."""
    items = items_of(h, w)
    if (h, w) == (65, 97):
        assert max(len(c) for c, _, _ in items) == 6305
    got = check_items(items)
    bare, a, _, status = GO.run_decode(entries()[0], items, dev=DEV, stats=False)
    assert status == 0 and a is None and all(np.array_equal(x, y) for x, y in zip(bare, got))


def test_decode_ragged_off_sixteen_bytes_and_in_rounds():
    """Nine planes of nine sizes in one call; bit offsets that start 4 bytes off a 16-byte boundary; a workspace of exactly two planes,
    which forces five rounds."""
    whole = check_items(ragged_items())
    off16 = check_items(ragged_items(), guard=GO.GUARD + 4)
    rounds = check_items(ragged_items(), ws_planes=2)
    assert all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(whole, off16, rounds))


@pytest.mark.parametrize("kind", GO.ZERO_KINDS)
def test_decode_zero_counts(kind):
    """Every case again with zero counts inserted: one, two, three in a row, a trailing 0 -- and ragged in one call."""
    for h, w in GO.SHAPES:
        check_items([(GO.with_zeros(c, kind, seed=i), h, w) for i, (c, _, _) in enumerate(items_of(h, w))])
    check_items(ragged_items(zeros=kind))
    if kind == "two":
        got = check_items([([0, 0, 33 * 31], 33, 31), ([0, 33 * 31], 33, 31), ([0, 0, 1], 1, 1)])
        assert not got[0].any() and not got[2].any()


@pytest.mark.parametrize("name", list(refusal_cases()))
def test_decode_refuses_whole_planes(name):
    """status 1, the refused plane zero -- or untouched where its table is at fault --, area 0, box -1, its neighbours whole and every
    band untouched (GO.run_decode); the host entry refuses the same planes."""
    items, over, refused, unstored = refusal_cases()[name]
    dec, dec_host, _, _ = entries()
    got, area, box, status = GO.run_decode(dec, items, dev=DEV, **over)
    _, h_area, h_box, h_status = GO.run_decode(dec_host, items, **over)
    assert status == h_status == 1 and np.array_equal(area, h_area) and np.array_equal(box, h_box)
    for p, (c, h, w) in enumerate(items):
        if p in unstored:
            assert got[p] is None and area[p] == 0 and box[p].tolist() == [-1] * 4
        elif p in refused:
            GO.check_plane(got[p], area[p], box[p], None, h, w)
        else:
            GO.check_plane(got[p], area[p], box[p], GO.expected(c, h, w), h, w)


def test_decode_replays_into_used_outputs():
    """Every output is initialised by the call: a second call into the same tensors, and one after a call that refused a plane, gives
    the same bytes."""
    from camouflaged_vlm_amd import hip
    items = ragged_items()
    sizes = [(h, w) for _, h, w in items]
    d, off, _, _ = SO.tables(sizes, 0)
    flat = np.concatenate([c for c, _, _ in items]).astype(np.int32)
    ro = np.concatenate([[0], np.cumsum([len(c) for c, _, _ in items])]).astype(np.int64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    P, mp = len(items), max(h * w for h, w in sizes)
    bits = torch.empty(int(off[-1]), dtype=torch.uint8, device=DEV)
    area, box, status = (torch.empty(s, dtype=torch.int32, device=DEV) for s in ((P,), (P, 4), (1,)))
    ws = torch.empty(hip.mask_rle_decode_workspace_bytes(3, mp), dtype=torch.uint8, device=DEV)
    bad = flat.copy()
    bad[0] += 1
    seen = []
    for counts in (flat, flat, bad, flat):
        hip.mask_rle_decode(t(counts), t(ro), t(d), t(off), mp, bits, area, box, status, ws)
        seen.append((bits.cpu().numpy().copy(), area.cpu().tolist(), box.cpu().tolist(), status.item()))
    assert [s[3] for s in seen] == [0, 0, 1, 0] and seen[2][1][0] == 0
    for s in (seen[1], seen[3]):
        assert np.array_equal(s[0], seen[0][0]) and s[1:] == seen[0][1:]


# ---- the intersections ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", GO.INTER_SHAPES)
def test_inter_equals_the_oracle(h, w):
    """Random densities, a plane with itself, disjoint planes, garbage in the pad bits, A and B in one tensor and in two, pairs out of
    order and repeated; 480 x 641 has several word spans per pair."""
    _, _, inter, inter_host = entries()
    A = GO.inter_planes(h, w)
    B = list(reversed(GO.inter_planes(h, w)))
    pairs = all_pairs(len(A))
    pairs = pairs[::-1] + pairs[:5] + pairs[:5]
    for garbage in (False, True):
        got, status = GO.run_inter(inter, A, B, pairs, dev=DEV, garbage=garbage)
        assert status == 0 and np.array_equal(got, GO.inter_oracle(A, B, pairs)), garbage
        assert np.array_equal(got, GO.run_inter(inter_host, A, B, pairs, garbage=garbage)[0])
        same, status = GO.run_inter(inter, A, None, pairs, dev=DEV, garbage=garbage)
        assert status == 0 and np.array_equal(same, GO.inter_oracle(A, A, pairs))
        assert same[[pairs.index((i, i)) for i in range(len(A))]].tolist() == [int(m.sum()) for m in A]
        assert same[pairs.index((3, 4))] == 0                         # the two halves
    small, status = GO.run_inter(inter, A, B, pairs, dev=DEV, max_words=1)      # a smaller grid, the same sums
    assert status == 0 and np.array_equal(small, GO.inter_oracle(A, B, pairs))


def test_inter_refuses_pairs():
    """An index -1, an index equal to P, two sizes, a bad table: -1 and status 1, the other pairs whole."""
    _, _, inter, inter_host = entries()
    A, B, pairs = inter_refusals()
    want = GO.inter_oracle(A, B, pairs)
    got, status = GO.run_inter(inter, A, B, pairs, dev=DEV)
    assert status == 1 and np.array_equal(got, want) and (want == -1).sum() == 6
    _, off, _, _ = SO.tables([m.shape for m in B])
    bad = off.copy()
    bad[1:] += 4
    three = [(0, 0), (1, 1), (2, 2)]
    for over in ((None, bad, None), (None, None, int(off[-1]) - 4), ([[33, 31], [33, 32], [33, 31]], None, None)):
        got, status = GO.run_inter(inter, A, B, three, dev=DEV, b_tables=over)
        host, h_status = GO.run_inter(inter_host, A, B, three, b_tables=over)
        assert status == h_status == 1 and np.array_equal(got, host) and (got == -1).sum() == 1 and (got >= 0).sum() == 2, over


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


def record_reads(monkeypatch):
    reads = []
    for name in ("item", "cpu", "tolist", "numpy"):
        real = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _real=real, _n=name, **k: (reads.append(_n), _real(self, *a, **k))[1])
    return reads


def test_round_trips(cas, monkeypatch):
    """rle_decode(mask_rle_sized(s)) gives s back -- bits, area, box -- on §19's ragged seven, without a synchronisation;
    mask_rle_sized(rle_decode(r)) gives the canonical counts, zero counts merged away; the compressed strings decode to the planes."""
    from camouflaged_vlm_amd import rle
    from camouflaged_vlm_amd.engine import SizedMasks
    rng = np.random.default_rng(19)
    logits = torch.from_numpy(rng.normal(0, 3, (7, 24, 40)).astype(np.float32)).to(DEV)
    s = cas.pack_masks_sized(logits, SO.RAGGED)
    r = cas.mask_rle_sized(s)
    torch.cuda.synchronize()
    reads = record_reads(monkeypatch)
    d = cas.rle_decode(r)
    monkeypatch.undo()
    assert reads == [], reads
    assert isinstance(d, SizedMasks) and d.level == 0 and d.sizes == SO.RAGGED and d.status.numel() == 1
    d.check()
    assert torch.equal(d.bits, s.bits) and torch.equal(d.area, s.area) and torch.equal(d.box, s.box) and torch.equal(d.offsets, s.offsets)
    bare = cas.rle_decode(r, stats=False)
    assert bare.area is None and bare.box is None and torch.equal(bare.bits, s.bits)
    masks = [s.to_numpy(p) for p in range(7)]
    for compressed in (False, True):
        again = cas.rle_decode(r.to_coco(compressed=compressed))
        again.check()
        assert torch.equal(again.bits, s.bits) and torch.equal(again.area, s.area) and torch.equal(again.box, s.box)
    zeros = [{"size": list(m.shape), "counts": GO.with_zeros(RO.plane_counts(m), GO.ZERO_KINDS[p % 4], seed=p).tolist()} for p, m in enumerate(masks)]
    planes = [rle.decode(z["counts"], *z["size"]) for z in zeros]
    back = cas.mask_rle_sized(cas.rle_decode(zeros))
    want = [RO.plane_counts(m) for m in planes]
    assert back.n_runs.cpu().tolist() == [len(w) for w in want] and np.array_equal(back.counts.cpu().numpy(), np.concatenate(want))
    assert any(len(w) != len(z["counts"]) for w, z in zip(want, zeros))
    # a MaskRle whose counts do not describe its planes: the kernel's checks are the only ones, check() reports them
    r.counts[int(r.offsets[3].item())] += 1
    broken = cas.rle_decode(r)
    with pytest.raises(RuntimeError, match="rle_decode"):
        broken.check()
    assert int(broken.area[3]) == 0 and not bool(broken.plane(3).any()) and torch.equal(broken.plane(4), s.plane(4))
    for bad in (None, [], [{"size": [2, 3], "counts": [5]}], s, s.bits):
        with pytest.raises(ValueError):
            cas.rle_decode(bad)


def test_mask_inter_sized_and_iou(cas):
    """Detections against annotations of three images of two sizes: pairs from image ids, ordered by p then q; explicit pairs with a
    size mismatch (-1); iou() with and without iscrowd against the formula, inter = 0 and the -1 rows included."""
    from camouflaged_vlm_amd.engine import SizedOverlaps
    rng = np.random.default_rng(20)
    sz = [(97, 131), (97, 131), (33, 31)]
    a_image, b_image = [0, 0, 1, 1, 2], [1, 0, 2, 0, 1]
    A = [rng.random(sz[i]) < 0.4 for i in a_image]
    B = [rng.random(sz[i]) < 0.3 for i in b_image]
    B[1][:] = False                                                   # an empty annotation: inter = 0
    coco = lambda ms: [{"size": list(m.shape), "counts": RO.plane_counts(m).tolist()} for m in ms]
    a, b = cas.rle_decode(coco(A)), cas.rle_decode(coco(B))
    o = cas.mask_inter_sized(a, b, a_image=a_image, b_image=b_image)
    assert isinstance(o, SizedOverlaps)
    pairs = [(p, q) for p in range(5) for q in range(5) if a_image[p] == b_image[q]]
    assert o.pairs.cpu().tolist() == [list(p) for p in pairs] and o.status.item() == 0
    want = GO.inter_oracle(A, B, pairs)
    assert np.array_equal(o.inter.cpu().numpy(), want) and (want == 0).any()
    assert o.area_a.cpu().tolist() == [int(A[p].sum()) for p, _ in pairs] and o.area_b.cpu().tolist() == [int(B[q].sum()) for _, q in pairs]
    crowd = [False, True, False, True, True]
    for flags in (None, crowd):
        got = o.iou(flags)
        f = [False] * len(pairs) if flags is None else [flags[q] for _, q in pairs]
        assert got.dtype == np.float64 and np.array_equal(got, GO.iou_formula(want, o.area_a.cpu().tolist(), o.area_b.cpu().tolist(), f))
    mixed = [(4, 2), (0, 2), (2, 1), (2, 1), (4, 3)]                  # (0, 2) and (4, 3): two sizes
    m = cas.mask_inter_sized(a, b, pairs=mixed)
    want = GO.inter_oracle(A, B, mixed)
    assert m.status.item() == 1 and np.array_equal(m.inter.cpu().numpy(), want) and want.tolist().count(-1) == 2
    assert np.array_equal(m.iou(crowd), GO.iou_formula(want, m.area_a.cpu().tolist(), m.area_b.cpu().tolist(), [crowd[q] for _, q in mixed]))
    with pytest.raises(RuntimeError):
        m.check()
    on_device = cas.mask_inter_sized(a, b, pairs=torch.tensor(mixed, device=DEV))
    assert torch.equal(on_device.inter, m.inter)
    own = cas.mask_inter_sized(a, a, pairs=[(p, p) for p in range(5)])
    assert torch.equal(own.inter, a.area) and own.iou().tolist() == [1.0] * 5
    for kw in (dict(), dict(pairs=[(5, 0)]), dict(pairs=[(0, -1)]), dict(a_image=a_image), dict(a_image=[7] * 5, b_image=b_image),
               dict(pairs=mixed, a_image=a_image, b_image=b_image)):
        with pytest.raises(ValueError):
            cas.mask_inter_sized(a, b, **kw)
    with pytest.raises(ValueError):
        cas.mask_inter_sized(a.bits, b, pairs=mixed)
    with pytest.raises(ValueError):
        cas.mask_inter_sized(a, cas.rle_decode(coco(B), stats=False), pairs=mixed)


OTHER = ("classes", "pass1_logits", "masks", "edges", "logits", "pred", "iou", "mask_bits", "area", "box", "inter", "n_comp", "comps", "n_kept",
         "kept_bits", "kept_area", "kept_box", "n_holes", "holes", "n_filled", "filled_bits", "filled_area", "band_bits", "band_area",
         "band_inter", "edge_bits", "edge_area", "edge_band", "edge_inter")
SIZES = [(213, 320), (480, 641)]
CLASSES = [[0, 1, 2], [2, 1, 0]]                                                  # K = 3: a chunk of 4 crosses the image boundary


def annotations(sizes, ids):
    """Two discs and a rectangle, one per entry of ids, each at the size of its image -> (bool planes, COCO dicts)."""
    shapes = []
    for n, b in enumerate(ids):
        h, w = sizes[b]
        if n == 1:
            m = np.zeros((h, w), dtype=bool)
            m[h // 5:h // 2, w // 4:w - 7] = True
        else:
            m = GO.disc(h, w, h * (0.4 + 0.1 * n), w * 0.5, min(h, w) * (0.45 - 0.1 * n))
        shapes.append(m)
    return shapes, [{"size": list(m.shape), "counts": RO.plane_counts(m).tolist()} for m in shapes]


def check_call(cas, call, sizes, ids, K: int, masks: str = "bits"):
    """`call(**kw)` runs one entry point: with ground_truth= the result's `gt_overlaps` is the oracle on the call's own sized bits and
    every other field -- the sized planes and their encoding included -- keeps the bits of the call without it.  -> the result."""
    truth, coco = annotations(sizes, ids)
    gt = cas.rle_decode(coco)
    gt.check()
    plain = call(masks=masks, sizes=sizes, rle="sized")
    assert plain.gt_overlaps is None
    keep = {f: getattr(plain, f).clone() for f in OTHER if getattr(plain, f) is not None}
    keep.update({"sized." + f: getattr(plain.sized, f).clone() for f in ("bits", "area", "box", "offsets")})
    keep.update({"rle." + f: getattr(plain.rle, f).clone() for f in ("counts", "offsets", "n_runs")})
    h = call(masks=masks, sizes=sizes, rle="sized", ground_truth=(gt, ids))
    torch.cuda.synchronize()
    for f in OTHER:
        assert (getattr(h, f) is None) == (f not in keep), f
    for f, t in keep.items():                                                     # bit for bit, floats included
        obj = h
        for part in f.split("."):
            obj = getattr(obj, part)
        assert torch.equal(obj.contiguous().view(torch.uint8), t.contiguous().view(torch.uint8)), f
    o = h.gt_overlaps
    o.check()
    pairs = [(p, q) for p in range(len(sizes) * K) for q in range(len(ids)) if ids[q] == p // K]
    assert o.pairs.cpu().tolist() == [list(p) for p in pairs]
    got = [h.sized.to_numpy(p) for p in range(len(h.sized.sizes))]
    want = GO.inter_oracle(got, truth, pairs)
    assert np.array_equal(o.inter.cpu().numpy(), want) and want.min() >= 0
    assert o.area_a.cpu().tolist() == [int(got[p].sum()) for p, _ in pairs] and o.area_b.cpu().tolist() == [int(truth[q].sum()) for _, q in pairs]
    assert np.array_equal(o.iou(), GO.iou_formula(want, o.area_a.cpu().tolist(), o.area_b.cpu().tolist(), [False] * len(pairs)))
    return h


def test_infer_classes_ground_truth(tiny, cas, monkeypatch):
    _, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    classes = torch.tensor(CLASSES)
    call = lambda **kw: cas.infer_classes(inp, ci, cm, classes=classes, **kw)
    both = check_call(cas, call, SIZES, [0, 0, 1], 3, "both")
    bits = check_call(cas, call, SIZES, [0, 0, 1], 3, "bits")
    assert torch.equal(bits.gt_overlaps.inter, both.gt_overlaps.inter)
    assert int(both.gt_overlaps.inter.max()) > 0
    # ground truth made from the call's own encoding: a hypothesis against itself
    own = cas.rle_decode(both.rle)
    ids = [0, 0, 0, 1, 1, 1]
    h = call(masks="bits", sizes=SIZES, ground_truth=(own, ids))
    o = h.gt_overlaps
    o.check()
    pairs = o.pairs.cpu().tolist()
    assert pairs == [[p, q] for p in range(6) for q in range(6) if ids[q] == p // 3]
    diag = [i for i, (p, q) in enumerate(pairs) if p == q]
    area = h.sized.area.cpu().numpy()
    assert np.array_equal(o.inter.cpu().numpy()[diag], area) and area.max() > 0
    assert np.array_equal(o.iou()[diag], (area > 0).astype(np.float64))


def test_decode_ground_truth(tiny, cas, monkeypatch):
    _, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    enc = cas.encode(inp, ci, cm)
    sizes = [SIZES[1], SIZES[0], SIZES[1]]                                        # one per decoded row
    check_call(cas, lambda **kw: cas.decode(enc, topk=3, images=[1, 0, 1], **kw), sizes, [1, 1, 2], 3, "both")
    check_call(cas, lambda **kw: cas.decode(enc, topk=3, images=[1, 0, 1], **kw), sizes, [2, 0, 0], 3, "bits")


def test_bad_ground_truth_requests_raise_and_launch_nothing(tiny, cas):
    from camouflaged_vlm_amd import hip
    _, _, _, (inp, ci, cm), _ = tiny
    enc = cas.encode(inp, ci, cm)
    _, coco = annotations(SIZES, [0, 0, 1])
    gt = cas.rle_decode(coco)
    bare = cas.rle_decode(coco, stats=False)
    torch.cuda.synchronize()
    calls = []
    names = ("gemm", "layernorm", "topk_select", "patchify", "split_f32", "expand_blocks", "bilinear", "mask_pack", "mask_pack_sized",
             "mask_rle_count", "mask_rle_emit", "mask_rle_count_w", "mask_rle_emit_w", "mask_overlap", "mask_rle_decode", "mask_inter_sized")
    saved = {n: getattr(hip, n) for n in names}
    for n in saved:
        setattr(hip, n, lambda *a, _n=n, **k: calls.append(_n))
    try:
        for kw in (dict(masks="bits", ground_truth=(gt, [0, 0, 1])), dict(masks="logits", sizes=SIZES, ground_truth=(gt, [0, 0, 1])),
                   dict(masks="bits", sizes=SIZES, ground_truth=(gt, [0, 1, 1])), dict(masks="bits", sizes=SIZES, ground_truth=(gt, [0, 0, 2])),
                   dict(masks="bits", sizes=SIZES, ground_truth=(gt, [0, 0, -1])), dict(masks="bits", sizes=SIZES, ground_truth=(gt, [0, 0])),
                   dict(masks="bits", sizes=SIZES, ground_truth=(gt, [0, 0, 1.0])), dict(masks="bits", sizes=SIZES, ground_truth=gt),
                   dict(masks="bits", sizes=SIZES, ground_truth=(coco, [0, 0, 1])), dict(masks="bits", sizes=SIZES, ground_truth=(bare, [0, 0, 1])),
                   dict(masks="bits", sizes=SIZES[::-1], ground_truth=(gt, [0, 0, 1]))):
            with pytest.raises(ValueError):
                cas.infer_classes(inp, ci, cm, topk=2, **kw)
            with pytest.raises(ValueError):
                cas.decode(enc, topk=2, **kw)
        for bad in (None, [], "ab", [{"size": [2, 3], "counts": [5]}], [{"size": [2, 3], "counts": [7, -1]}], [{"size": [0, 3], "counts": [0]}],
                    [{"size": [2, 3], "counts": "\x01"}]):
            with pytest.raises(ValueError):
                cas.rle_decode(bad)
        for kw in (dict(), dict(pairs=[(3, 0)]), dict(a_image=[0, 0, 1], b_image=[2, 2, 2])):
            with pytest.raises(ValueError):
                cas.mask_inter_sized(gt, gt, **kw)
    finally:
        for n, f in saved.items():
            setattr(hip, n, f)
    assert calls == []


def test_ground_truth_memory_is_the_results(tiny, cas, monkeypatch):
    """After one call per mode has sized the grow-only workspaces, ground_truth= peaks above the same call without it by no more than
    the new result tensors, the two uploaded size tables and the two gathers' index temporaries (each one allocator block at this
    size) -- and by nothing at all where the call's peak lies inside the chunk loop, before the intersection runs; the decoder's
    workspace "cls_rle" is no larger than RLE_WS_CAP."""
    from camouflaged_vlm_amd import engine
    _, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    _, coco = annotations(SIZES, [0, 0, 1])
    gt = cas.rle_decode(coco)
    modes = {"sized": dict(masks="bits", sizes=SIZES), "gt": dict(masks="bits", sizes=SIZES, ground_truth=(gt, [0, 0, 1]))}
    for kw in modes.values():
        cas.infer_classes(inp, ci, cm, topk=3, **kw)
    torch.cuda.synchronize()
    assert cas.ws._flat[("u8", "cls_rle")].numel() <= engine.RLE_WS_CAP
    block = lambda ts: sum(-(-t.numel() * t.element_size() // 512) * 512 for t in ts)              # the allocator's 512-byte blocks
    peak, results = {}, {}
    for name, kw in modes.items():
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        h = cas.infer_classes(inp, ci, cm, topk=3, **kw)
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - start
        o = h.gt_overlaps
        results[name] = 0 if o is None else block([o.pairs, o.inter, o.area_a, o.area_b, o.status])
        del h, o
    print(f"peak over the starting level: {peak}; new results {results}")
    assert results["gt"] > 0 and 0 <= peak["gt"] - peak["sized"] <= results["gt"] + 6 * 512


# ---- drop-in ---------------------------------------------------------------------------------------------------------------------------------
def test_dropin_passes_ground_truth_through(tiny, gold, golden_dir):
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
        check_call(model, lambda **kw: model.infer_classes(inp, ci, cm, topk=3, **kw), SIZES, [0, 0, 1], 3, "both")
        enc = model.encode_images(inp, ci, cm)
        h = check_call(model, lambda **kw: model.decode_classes(enc, topk=3, **kw), SIZES, [1, 0, 1], 3, "bits")
        truth, coco = annotations(SIZES, [1, 0, 1])
        o = model.mask_inter_sized(h.sized, model.rle_decode(coco), a_image=[0, 0, 0, 1, 1, 1], b_image=[1, 0, 1])
        assert torch.equal(o.inter, h.gt_overlaps.inter) and torch.equal(o.pairs, h.gt_overlaps.pairs)
