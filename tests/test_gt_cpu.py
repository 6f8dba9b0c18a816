"""COCO annotations on the device without a GPU: the oracle against a pixel loop; cvlm_debug_mask_rle_decode_host and
cvlm_debug_mask_inter_sized_host -- the kernels' per-thread functions (csrc/gt_logic.h) run sequentially -- against the oracle on every
shape, plane, zero count and refusal of the GPU tests; the pure host checks `rle_decode_request`, `pairs_request` and
`ground_truth_request`; `SizedOverlaps.iou` against the formula; every CVLM_E_BADARG of the new entries; the exports."""
import dataclasses

import numpy as np
import pytest
import torch

import gt_oracle as GO
import rle_oracle as RO
import sized_oracle as SO
from camouflaged_vlm_amd import hip, rle
from camouflaged_vlm_amd.engine import (ClassHypotheses, SizedMasks, SizedOverlaps, ground_truth_request, pairs_request,
                                        rle_decode_request, sized_request)


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------------
def test_the_definition_equals_a_pixel_loop():
    n = 0
    for h, w in ((1, 1), (1, 5), (5, 1), (3, 4), (7, 9), (8, 33)):
        for name, m in GO.planes(h, w).items():
            c = RO.plane_counts(m)
            assert np.array_equal(rle.decode(c, h, w), m) and np.array_equal(GO.decode_loop(c, h, w), m), name
            for kind in GO.ZERO_KINDS:
                z = GO.with_zeros(c, kind, seed=n)
                assert int(z.sum()) == h * w and np.array_equal(rle.decode(z, h, w), GO.decode_loop(z, h, w)), (name, kind)
                n += 1
    assert n >= 12
    assert not rle.decode([0, 0, 6], 2, 3).any() and rle.decode([0, 6], 2, 3).all()
    assert np.array_equal(rle.decode([2, 0, 1, 3], 2, 3), GO.decode_loop([2, 0, 1, 3], 2, 3))


# ---- the host entry of the decoder -----------------------------------------------------------------------------------------------------------
def items_of(h, w):
    return [(RO.plane_counts(m), h, w) for m in GO.planes(h, w).values()]


@pytest.mark.parametrize("h,w", GO.SHAPES)
def test_host_decode_equals_the_definition(h, w):
    cases = GO.planes(h, w)
    got, area, box, status = GO.run_decode(hip.mask_rle_decode_host, items_of(h, w))
    assert status == 0
    for p, (name, m) in enumerate(cases.items()):
        GO.check_plane(got[p], area[p], box[p], m, h, w)
    bare, a, _, status = GO.run_decode(hip.mask_rle_decode_host, items_of(h, w), stats=False)
    assert status == 0 and a is None and all(np.array_equal(x, y) for x, y in zip(bare, got))


def ragged_items(zeros=None):
    out = []
    for i, (h, w) in enumerate(GO.SHAPES):
        m = list(GO.planes(h, w).values())[4 + i % 6]                # checker, stripes, random planes in turn
        c = RO.plane_counts(m)
        out.append((c if zeros is None else GO.with_zeros(c, zeros, seed=i), h, w))
    return out


def test_host_decode_ragged_and_off_sixteen_bytes():
    for guard in (GO.GUARD, GO.GUARD + 4):
        items = ragged_items()
        got, area, box, status = GO.run_decode(hip.mask_rle_decode_host, items, guard=guard)
        assert status == 0
        for p, (c, h, w) in enumerate(items):
            GO.check_plane(got[p], area[p], box[p], GO.expected(c, h, w), h, w)


@pytest.mark.parametrize("kind", GO.ZERO_KINDS)
def test_host_decode_zero_counts(kind):
    for h, w in GO.SHAPES:
        items = [(GO.with_zeros(c, kind, seed=i), h, w) for i, (c, _, _) in enumerate(items_of(h, w))]
        got, area, box, status = GO.run_decode(hip.mask_rle_decode_host, items)
        assert status == 0
        for p, (c, _, _) in enumerate(items):
            GO.check_plane(got[p], area[p], box[p], GO.expected(c, h, w), h, w)
    got, area, box, status = GO.run_decode(hip.mask_rle_decode_host, [([0, 0, 33 * 31], 33, 31), ([0, 33 * 31], 33, 31)])
    assert status == 0 and area.tolist() == [0, 33 * 31] and not got[0].any()


def refusal_cases():
    """name -> (items, overrides of run_decode, planes that must come out refused, planes whose slice is not stored)."""
    good = ragged_items()[2:6]                                        # (1, 32) (8, 33) (33, 31) (32, 63)
    W = GO.WORD_GUARD
    n = [len(c) for c, _, _ in good]
    ro = np.concatenate([[0], np.cumsum(n)]) + W
    total = int(ro[-1]) + W
    out = {}

    def swap(p, counts, h=None, w=None):
        items = list(good)
        items[p] = (np.asarray(counts, dtype=np.int64), good[p][1] if h is None else h, good[p][2] if w is None else w)
        return items
    c1 = good[1][0]
    out["negative"] = (swap(1, list(c1[:-1]) + [c1[-1] + 1, -1]), {}, [1], [])
    out["one_short"] = (swap(1, list(c1[:-1]) + [c1[-1] - 1]), {}, [1], [])
    out["one_long"] = (swap(1, list(c1[:-1]) + [c1[-1] + 1]), {}, [1], [])
    out["wraps_32_bits"] = ([good[0], (np.asarray([2 ** 30, 2 ** 30, 2 ** 30, 2 ** 30 + 4]), 2, 2), good[2]], {}, [1], [])
    out["two_of_2_30"] = ([good[0], (np.asarray([2 ** 30, 2 ** 30]), 2, 2), good[2]], {}, [1], [])
    # plane 1's slice is empty; the later ones take the counts that follow
    out["empty_slice"] = ([good[0], good[1], good[1], good[1]], dict(run_offsets=[W, W + n[0], W + n[0], W + n[0] + n[1], W + n[0] + 2 * n[1]]),
                          [1], [])
    back = ro.copy()
    back[2] = back[1] - 1                                             # plane 1 runs backwards, plane 2 starts inside plane 0's counts
    out["backwards"] = (good, dict(run_offsets=back), [1, 2], [])
    below = ro.copy()
    below[0] = -1
    out["starts_below_zero"] = (good, dict(run_offsets=below), [0], [])
    beyond = ro.copy()
    beyond[-1] = total + 1
    out["ends_beyond_total"] = (good, dict(run_offsets=beyond), [3], [])
    out["total_cuts_the_last"] = (good, dict(total=int(ro[-1]) - 1), [3], [])
    out["max_pixels_too_small"] = (good, dict(max_pixels=33 * 31 - 1), [2, 3], [])
    _, off, nb, _ = SO.tables([(h, w) for _, h, w in good])
    bad = off.copy()
    bad[2:] += 4
    out["table_slice_too_long"] = (good, dict(bit_offsets=bad), [1], [1])
    out["table_end_beyond"] = (good, dict(nbytes=int(off[-1]) - 4), [3], [3])
    for first in (-4, GO.GUARD + 2):
        bad = off.copy()
        bad[0] = first
        out[f"table_start_{first}"] = (good, dict(bit_offsets=bad), [0], [0])
    for size in ((0, 32), (1, -2), (1, 16385), (2 ** 31 - 1, 2 ** 31 - 1)):
        dims = [list(size)] + [[h, w] for _, h, w in good[1:]]
        out[f"size_{size}"] = (good, dict(dims=dims), [0], [0])
    return out


@pytest.mark.parametrize("name", list(refusal_cases()))
def test_host_decode_refuses_whole_planes(name):
    items, over, refused, unstored = refusal_cases()[name]
    got, area, box, status = GO.run_decode(hip.mask_rle_decode_host, items, **over)
    assert status == 1
    for p, (c, h, w) in enumerate(items):
        if p in unstored:
            assert got[p] is None and area[p] == 0 and box[p].tolist() == [-1] * 4
        elif p in refused:
            GO.check_plane(got[p], area[p], box[p], None, h, w)
        else:
            GO.check_plane(got[p], area[p], box[p], GO.expected(c, h, w), h, w)


# ---- the host entry of the intersections -------------------------------------------------------------------------------------------------------
def all_pairs(n):
    return [(a, b) for a in range(n) for b in range(n)]


@pytest.mark.parametrize("h,w", GO.INTER_SHAPES)
def test_host_inter_equals_the_oracle(h, w):
    A = GO.inter_planes(h, w)
    B = list(reversed(GO.inter_planes(h, w + 0)))
    pairs = all_pairs(len(A))
    pairs = pairs[::-1] + pairs[:5] + pairs[:5]                       # out of order, repeated
    for garbage in (False, True):
        got, status = GO.run_inter(hip.mask_inter_sized_host, A, B, pairs, garbage=garbage)
        assert status == 0 and np.array_equal(got, GO.inter_oracle(A, B, pairs)), garbage
        same, status = GO.run_inter(hip.mask_inter_sized_host, A, None, pairs, garbage=garbage)
        assert status == 0 and np.array_equal(same, GO.inter_oracle(A, A, pairs))
        diag = same[[pairs.index((i, i)) for i in range(len(A))]]
        assert diag.tolist() == [int(m.sum()) for m in A]             # a plane with itself: its area
    assert GO.inter_oracle(A, A, [(3, 4)])[0] == 0                    # the two halves are disjoint


def inter_refusals():
    A = GO.inter_planes(33, 31)[:3] + GO.inter_planes(1, 32)[:2]
    B = GO.inter_planes(33, 31)[1:4]
    pairs = [(0, 0), (-1, 0), (1, 1), (5, 1), (2, 3), (0, -1), (3, 0), (2, 2), (4, 1), (1, 0)]
    return A, B, pairs


def test_host_inter_refuses_pairs():
    A, B, pairs = inter_refusals()
    want = GO.inter_oracle(A, B, pairs)
    assert (want == -1).sum() == 6
    got, status = GO.run_inter(hip.mask_inter_sized_host, A, B, pairs)
    assert status == 1 and np.array_equal(got, want)
    _, off, nb, _ = SO.tables([m.shape for m in B])
    bad = off.copy()
    bad[1:] += 4                                                      # plane 0 of B: a slice four bytes too long; plane 1 starts off its rows
    got, status = GO.run_inter(hip.mask_inter_sized_host, A, B, [(0, 0), (1, 1), (2, 2)], b_tables=(None, bad, None))
    assert status == 1 and got[0] == -1 and got[2] >= 0
    got, status = GO.run_inter(hip.mask_inter_sized_host, A, B, [(0, 0), (1, 1), (2, 2)], b_tables=(None, None, int(off[-1]) - 4))
    assert status == 1 and got.tolist()[:2] == GO.inter_oracle(A, B, [(0, 0), (1, 1)]).tolist() and got[2] == -1
    got, status = GO.run_inter(hip.mask_inter_sized_host, A, B, [(0, 0), (1, 1)], max_words=1)      # a smaller grid, the same sums
    assert status == 0 and np.array_equal(got, GO.inter_oracle(A, B, [(0, 0), (1, 1)]))


# ---- the pure host checks ----------------------------------------------------------------------------------------------------------------------
def test_rle_decode_request_accepts_and_refuses():
    m = GO.planes(8, 33)["random_0.5"]
    c = RO.plane_counts(m)
    counts, off, sizes = rle_decode_request([{"size": [8, 33], "counts": c.tolist()}, {"size": (np.int64(8), 33), "counts": rle.counts_to_string(c)},
                                             {"size": [8, 33], "counts": rle.counts_to_string(c).decode("ascii")},
                                             {"size": [2, 3], "counts": np.asarray([0, 0, 6])}, {"size": [1, 1], "counts": [1, 0]}])
    assert counts.dtype == np.int32 and off.dtype == np.int64 and sizes == [(8, 33)] * 3 + [(2, 3), (1, 1)]
    assert off.tolist() == [0, c.size, 2 * c.size, 3 * c.size, 3 * c.size + 3, 3 * c.size + 5]
    assert np.array_equal(counts[:c.size], c) and np.array_equal(counts[c.size:2 * c.size], c) and counts[-5:].tolist() == [0, 0, 6, 1, 0]
    ok = {"size": [2, 3], "counts": [1, 5]}
    bad = [None, 7, "abc", {}, ok, [], [ok, 5], [{"size": [2, 3]}], [{"counts": [6]}], [{"size": [2], "counts": [6]}], [{"size": "23", "counts": [6]}],
           [{"size": [2.0, 3], "counts": [6]}], [{"size": [True, 3], "counts": [3]}], [{"size": [0, 3], "counts": [0]}],
           [{"size": [2, 16385], "counts": [2 * 16385]}], [{"size": [2, 3], "counts": []}], [{"size": [2, 3], "counts": [5]}],
           [{"size": [2, 3], "counts": [7]}], [{"size": [2, 3], "counts": [7, -1]}], [{"size": [2, 3], "counts": [3.0, 3]}],
           [{"size": [2, 3], "counts": [True, 5]}], [{"size": [2, 3], "counts": 6}], [{"size": [2, 3], "counts": [[1, 5]]}],
           [{"size": [2, 3], "counts": "\x01"}], [{"size": [2, 3], "counts": b"o"}], [{"size": [2, 3], "counts": np.asarray([1.0, 5.0])}]]
    for r in bad:
        with pytest.raises(ValueError):
            rle_decode_request(r)
    with pytest.raises(ValueError, match="SAM.rle_decode"):
        rle_decode_request(None, who="SAM.rle_decode")


def test_pairs_request_accepts_and_refuses():
    a, b = [(3, 4)] * 4, [(3, 4)] * 3
    assert pairs_request(a, b, pairs=[(0, 0), (3, 2), (0, 0)]).tolist() == [[0, 0], [3, 2], [0, 0]]
    got = pairs_request(a, b, a_image=[0, 0, 1, 1], b_image=[1, 0, 1])
    assert got.dtype == np.int32 and got.tolist() == [[0, 1], [1, 1], [2, 0], [2, 2], [3, 0], [3, 2]]      # ordered by p, then q
    assert pairs_request(a, b, pairs=torch.tensor([[1, 1]])).tolist() == [[1, 1]]
    bad = [dict(), dict(pairs=[(0, 0)], a_image=[0] * 4, b_image=[0] * 3), dict(a_image=[0] * 4), dict(b_image=[0] * 3), dict(pairs=[]),
           dict(pairs=[(0, 0, 0)]), dict(pairs=[0, 0]), dict(pairs=[(0.0, 0.0)]), dict(pairs=[(-1, 0)]), dict(pairs=[(4, 0)]), dict(pairs=[(0, 3)]),
           dict(pairs="ab"), dict(a_image=[0] * 3, b_image=[0] * 3), dict(a_image=[0] * 4, b_image=[0.0] * 3), dict(a_image=[True] * 4, b_image=[0] * 3),
           dict(a_image=[0] * 4, b_image=[1] * 3), dict(a_image="0000", b_image=[0] * 3)]
    for kw in bad:
        with pytest.raises(ValueError):
            pairs_request(a, b, **kw)


class OnDevice:
    """What ground_truth_request asks of a tensor."""
    is_cuda = True


def fake_gt(sizes, area=True, cuda=True):
    return SizedMasks(bits=OnDevice() if cuda else torch.zeros(4, dtype=torch.uint8), offsets=None, area=torch.zeros(len(sizes)) if area else None,
                      box=None, status=None, sizes=list(sizes), level=0)


def test_ground_truth_request_accepts_and_refuses():
    sreq = sized_request(sizes=[(213, 320), (480, 641)], n=2)
    assert ground_truth_request(None, sreq, 2) is None and ground_truth_request(None, None, 2) is None
    gt = fake_gt([(213, 320), (213, 320), (480, 641)])
    assert ground_truth_request((gt, [0, 0, 1]), sreq, 2) == (gt, [0, 0, 1])
    assert ground_truth_request([gt, np.asarray([0, 0, 1])], sreq, 2)[1] == [0, 0, 1]
    bad = [(gt, None), (gt, [0, 0, 1], 3), gt, (gt, [0, 0]), (gt, [0, 0, 1, 1]), (gt, [0, 1, 1]), (gt, [1, 0, 1]), (gt, [0, 0, 2]), (gt, [0, 0, -1]),
           (gt, [0, 0, 1.0]), (gt, [0, 0, True]), (gt, "001"), ("gt", [0, 0, 1]), (gt.bits, [0, 0, 1]),
           (fake_gt(gt.sizes, area=False), [0, 0, 1]), (fake_gt(gt.sizes, cuda=False), [0, 0, 1])]
    for g in bad:
        with pytest.raises(ValueError):
            ground_truth_request(g, sreq, 2)
    with pytest.raises(ValueError, match="sizes="):
        ground_truth_request((gt, [0, 0, 1]), None, 2)
    with pytest.raises(ValueError, match="infer_classes"):
        ground_truth_request((gt, [0, 0, 1]), None, 2, who="infer_classes")


def test_sized_overlaps_iou_is_the_formula():
    pairs = torch.tensor([[0, 0], [1, 0], [2, 1], [0, 2], [3, 1], [1, 2]], dtype=torch.int32)
    inter = torch.tensor([5, 0, -1, 7, 12, 3], dtype=torch.int32)
    a = torch.tensor([10, 20, 30, 10, 12, 20], dtype=torch.int32)
    b = torch.tensor([8, 8, 9, 7, 40, 7], dtype=torch.int32)
    o = SizedOverlaps(pairs=pairs, inter=inter, area_a=a, area_b=b, status=torch.tensor([1], dtype=torch.int32))
    assert [f.name for f in dataclasses.fields(o)] == ["pairs", "inter", "area_a", "area_b", "status"]
    got = o.iou()
    assert got.dtype == np.float64 and np.array_equal(got, GO.iou_formula(inter.tolist(), a.tolist(), b.tolist(), [False] * 6))
    assert got.tolist() == [5 / 13, 0.0, -1.0, 0.7, 12 / 40, 3 / 24]
    crowd = [False, True, True]
    got = o.iou(iscrowd=crowd)
    assert np.array_equal(got, GO.iou_formula(inter.tolist(), a.tolist(), b.tolist(), [crowd[q] for q in pairs[:, 1].tolist()]))
    assert got.tolist() == [5 / 13, 0.0, -1.0, 0.7, 1.0, 3 / 20]
    with pytest.raises(RuntimeError):
        o.check()
    o.status = torch.zeros(1, dtype=torch.int32)
    o.check()


def test_decoded_planes_report_refusals_and_hypotheses_keep_their_fields():
    s = SizedMasks(bits=torch.zeros(4, dtype=torch.uint8), offsets=torch.tensor([0, 4]), area=None, box=None,
                   status=torch.ones(1, dtype=torch.int32), sizes=[(1, 1)], level=0)
    with pytest.raises(RuntimeError, match="rle_decode"):
        s.check()
    t = torch.zeros(1)
    h = ClassHypotheses(classes=t, pass1_logits=t, masks=t, edges=t, logits=t, pred=t)
    assert h.gt_overlaps is None
    assert [f.name for f in dataclasses.fields(h)] == ["classes", "pass1_logits", "masks", "edges", "logits", "pred"]
    assert ClassHypotheses(classes=t, pass1_logits=t, masks=None, edges=None, logits=t, pred=t, gt_overlaps="g").gt_overlaps == "g"


# ---- CVLM_E_BADARG, before the device is touched ------------------------------------------------------------------------------------------------
def test_decode_entries_refuse_bad_arguments_without_gpu():
    lib = hip.load()
    p = 1 << 20
    one = lib.cvlm_mask_rle_decode_workspace_bytes(1, 64)
    assert one == 32 and lib.cvlm_mask_rle_decode_workspace_bytes(3, 65) == 3 * 32 and lib.cvlm_mask_rle_decode_workspace_bytes(1, 1) == 32
    for P, mp in ((0, 64), (65536, 64), (1, 0), (1, 2 ** 28 + 1)):
        assert lib.cvlm_mask_rle_decode_workspace_bytes(P, mp) == -1
    base = dict(counts=p, total=8, ro=p + 4096, dims=p + 8192, bo=p + 12288, P=1, mp=64, bits=p + 16384, nb=8, area=p + 20480, box=p + 24576,
                status=p + 28672, ws=p + 65536, wsb=one)
    order = ("counts", "total", "ro", "dims", "bo", "P", "mp", "bits", "nb", "area", "box", "status")
    bad = [dict(counts=None), dict(ro=None), dict(dims=None), dict(bo=None), dict(bits=None), dict(status=None), dict(area=None), dict(box=None),
           dict(counts=p + 2), dict(dims=p + 8194), dict(bits=p + 16385), dict(area=p + 20482), dict(box=p + 24577), dict(status=p + 28674),
           dict(ro=p + 4100), dict(bo=p + 12292), dict(P=0), dict(P=65536), dict(total=0), dict(nb=3), dict(mp=0), dict(mp=2 ** 28 + 1)]
    for kw in bad:
        k = dict(base, **kw)
        args = [k[n] for n in order]
        assert lib.cvlm_debug_mask_rle_decode_host(*args) == -1, kw
        assert lib.cvlm_mask_rle_decode(*args, k["ws"], k["wsb"], None) == -1, kw
    args = [base[n] for n in order]
    for ws, wsb in ((None, one), (p + 65544, one), (p + 65536, one - 16)):
        assert lib.cvlm_mask_rle_decode(*args, ws, wsb, None) == -1, (ws, wsb)


def test_inter_entries_refuse_bad_arguments_without_gpu():
    lib = hip.load()
    p = 1 << 20
    base = dict(ab=p, an=8, ao=p + 4096, ad=p + 8192, Pa=1, bb=p + 12288, bn=8, bo=p + 16384, bd=p + 20480, Pb=1, pairs=p + 24576, N=1, mw=1,
                inter=p + 28672, status=p + 32768)
    order = ("ab", "an", "ao", "ad", "Pa", "bb", "bn", "bo", "bd", "Pb", "pairs", "N", "mw", "inter", "status")
    bad = [dict(ab=None), dict(ao=None), dict(ad=None), dict(bb=None), dict(bo=None), dict(bd=None), dict(pairs=None), dict(inter=None),
           dict(status=None), dict(ab=p + 1), dict(ad=p + 8194), dict(bb=p + 12290), dict(bd=p + 20481), dict(pairs=p + 24578), dict(inter=p + 28673),
           dict(status=p + 32770), dict(ao=p + 4100), dict(bo=p + 16388), dict(Pa=0), dict(Pa=65536), dict(Pb=0), dict(Pb=65536), dict(N=0),
           dict(N=2 ** 20 + 1), dict(an=3), dict(bn=0), dict(mw=0), dict(mw=16384 * 512 + 1)]
    for kw in bad:
        args = [dict(base, **kw)[n] for n in order]
        assert lib.cvlm_debug_mask_inter_sized_host(*args) == -1, kw
        assert lib.cvlm_mask_inter_sized(*args, None) == -1, kw


def test_new_symbols_are_exported_at_abi_12():
    lib = hip.load()
    assert hip.ABI_VERSION == 12 and lib.cvlm_abi_version() == 12
    for name in ("cvlm_mask_rle_decode", "cvlm_mask_rle_decode_workspace_bytes", "cvlm_debug_mask_rle_decode_host", "cvlm_mask_inter_sized",
                 "cvlm_debug_mask_inter_sized_host"):
        assert name in hip.EXPORTS and hasattr(lib, name)
    assert hip._SIGNATURES["cvlm_mask_rle_decode"] == hip._SIGNATURES["cvlm_debug_mask_rle_decode_host"] + "pls"
    assert hip._SIGNATURES["cvlm_mask_inter_sized"] == hip._SIGNATURES["cvlm_debug_mask_inter_sized_host"] + "s"
