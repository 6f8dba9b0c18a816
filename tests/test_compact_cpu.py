"""CPU: packed masks, areas, boxes and overlaps of class hypotheses -- the host check of the masks= / overlaps=
arguments (engine.compact_request), the numpy oracle (tests/compact_oracle.py) on hand-made planes, on the reference's own bits
(tests/golden/demo_classes_digest.npz) and on the tiny hypotheses of tests/classes_oracle.py, the result type's new fields, and the
argument checks of the two C-ABI entries (no GPU needed: they refuse before launching)."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from camouflaged_vlm_amd import hip, spec, synth
from camouflaged_vlm_amd.engine import ClassHypotheses, compact_request
from oracle import cvlm_oracle as O
import classes_oracle as CO
import compact_oracle as XO


# ---- the host request ----------------------------------------------------------------------------------------------------------
def test_compact_request_accepts_and_refuses():
    assert compact_request(n=2, K=3) == (True, False, False)                      # the default: logits only
    assert compact_request(masks="logits", overlaps=False, n=2, K=3) == (True, False, False)
    assert compact_request(masks="bits", n=2, K=3) == (False, True, False)
    assert compact_request(masks="both", n=2, K=3) == (True, True, False)
    assert compact_request(masks="bits", overlaps=True, n=2, K=3) == (False, True, True)
    assert compact_request(masks="both", overlaps=True, n=8, K=61) == (True, True, True)
    assert compact_request(masks="bits", overlaps=True, n=1, K=1024) == (False, True, True)
    assert compact_request(masks="bits", overlaps=False, n=1, K=4817) == (False, True, False)   # no overlap launch: K is free
    assert compact_request(masks="both", overlaps=np.bool_(True), n=1, K=2) == (True, True, True)
    bad = [dict(masks="bit"), dict(masks=None), dict(masks=1), dict(masks="BITS"), dict(masks=["bits"]),
           dict(overlaps=True), dict(masks="logits", overlaps=True),
           dict(masks="bits", overlaps=True, K=1025), dict(masks="both", overlaps=True, K=1025),
           dict(masks="bits", overlaps=True, n=64, K=1024),                       # 65536 planes: one more than the entry takes
           dict(masks="bits", overlaps=1), dict(masks="bits", overlaps="yes")]
    for kw in bad:
        with pytest.raises(ValueError):
            compact_request(**dict(dict(n=2, K=3), **kw))
    with pytest.raises(ValueError, match="infer_classes"):
        compact_request(masks="x", n=1, K=1, who="infer_classes")


def test_class_hypotheses_new_fields_are_optional():
    t = torch.zeros(1)
    h = ClassHypotheses(classes=t, pass1_logits=t, masks=t, edges=t, logits=t, pred=t)          # as every earlier caller builds it
    assert h.iou is None and h.mask_bits is None and h.area is None and h.box is None and h.inter is None
    assert [f.name for f in dataclasses.fields(h)] == ["classes", "pass1_logits", "masks", "edges", "logits", "pred"]
    h = ClassHypotheses(classes=t, pass1_logits=t, masks=None, edges=None, logits=t, pred=t, mask_bits=t, area=t, box=t, inter=t)
    assert h.masks is None and h.mask_bits is t and h.area is t and h.box is t and h.inter is t and h.iou is None


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def test_oracle_on_hand_made_planes():
    H, W = 8, 12
    m = np.full((9, H, W), -1.0, np.float32)
    m[1] = 1.0                                                                    # full
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    for p, (y, x) in enumerate(corners):
        m[2 + p, y, x] = 0.5
    m[6, 2:5, 3:10] = 2.0                                                         # a rectangle: rows 2..4, columns 3..9
    m[7, 3, 7] = 1e-30                                                            # one interior pixel
    m[8, 0, 0], m[8, H - 1, W - 1] = 3.0, 3.0                                     # two opposite corners
    bits, area, box = XO.pack(m)
    assert bits.shape == (9, H * W // 8) and bits.dtype == np.uint8
    assert area.tolist() == [0, H * W, 1, 1, 1, 1, 21, 1, 2]
    assert box.tolist() == [[-1] * 4, [0, 0, W - 1, H - 1], [0, 0, 0, 0], [W - 1, 0, W - 1, 0], [0, H - 1, 0, H - 1],
                            [W - 1, H - 1, W - 1, H - 1], [3, 2, 9, 4], [7, 3, 7, 3], [0, 0, W - 1, H - 1]]
    assert bits[0].tolist() == [0] * 12 and bits[1].tolist() == [255] * 12
    assert bits[2].tolist() == [0x80] + [0] * 11                                  # pixel 0 is the top bit of byte 0
    assert bits[5].tolist() == [0] * 11 + [0x01]                                  # the last pixel the bottom bit of the last byte
    assert bits[7, (3 * W + 7) >> 3] == 0x80 >> ((3 * W + 7) & 7)
    assert np.array_equal(XO.unpack(bits, H, W), m > 0)
    it = XO.inter(bits[None])[0]
    assert np.array_equal(it, it.T) and np.array_equal(np.diagonal(it), area)
    assert it[1].tolist() == area.tolist() and it[0].tolist() == [0] * 9          # the full plane meets all of each, the empty none
    assert it[2, 8] == 1 and it[5, 8] == 1 and it[3, 8] == 0 and it[6, 7] == 1 and it[6, 2] == 0
    # not greater than zero: -0.0, NaN, -inf; greater: the smallest denormal
    s = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-38] + [0.0] * 24, np.float32).reshape(1, 4, 8)
    assert XO.pack(s)[0][0].tolist() == [0b00010101, 0, 0, 0] and XO.pack(s)[1].tolist() == [3]


@pytest.fixture(scope="module")
def dgold(golden_dir):
    with np.load(os.path.join(golden_dir, "demo_classes_digest.npz")) as z:
        return {k: z[k] for k in z.files}


def test_oracle_on_the_reference_bits(dgold):
    S = spec.DEMO_SAM.inp_size
    bits = dgold["mask_bits"]
    n, K, nb = bits.shape
    assert nb == S * S // 8
    planes = XO.unpack(bits, S, S)
    area, box = XO.stats(planes)
    it = XO.inter(bits)
    assert np.array_equal(area, np.unpackbits(bits, axis=-1).sum(-1))
    assert area.min() > 0 and area.max() < S * S                                  # non-degenerate
    for i in range(n):
        assert np.array_equal(it[i], it[i].T) and np.array_equal(np.diagonal(it[i]), area[i])
        assert (it[i] <= np.minimum(area[i][:, None], area[i][None, :])).all()
        for a in range(K):
            x0, y0, x1, y1 = box[i, a]
            assert planes[i, a, y0:y1 + 1, x0:x1 + 1].sum() == area[i, a]         # nothing outside the box, and it is tight
            assert planes[i, a, y0].any() and planes[i, a, y1].any() and planes[i, a, :, x0].any() and planes[i, a, :, x1].any()
            for b in range(K):
                assert it[i, a, b] == np.count_nonzero(planes[i, a] & planes[i, b])
    iou = [it[i, a, b] / (area[i, a] + area[i, b] - it[i, a, b]) for i in range(n) for a in range(K) for b in range(a + 1, K)]
    print("reference bits: areas", area.tolist(), "pairwise IoU", [f"{v:.3f}" for v in iou])
    assert 0.0 < min(iou) and max(iou) < 1.0


def test_packed_tiny_hypotheses_agree_with_the_reference_sign(golden_dir):
    """tests/classes_oracle.py's full-resolution masks, packed, against the sign of the reference's own upsampled values
    (masks_at_pos) wherever those are further than 1e-3 from zero -- the gate the oracle is held to."""
    with np.load(os.path.join(golden_dir, "tiny_classes.npz")) as z:
        gold = {k: z[k] for k in z.files}
    g, c = spec.TINY_SAM, spec.TINY_CLIP
    sd = O.to_torch_sd(synth.make_full_state_dict(g, c))
    inp, ci, cm = (torch.from_numpy(t) for t in synth.make_inputs(g, c, 2))
    with torch.no_grad():
        tf = O.clip_text_features(sd, c, gold["eot_test"].tolist())
        r = CO.infer_classes(inp, ci, cm, sd, g, c, tf, torch.from_numpy(gold["bank_test"]), classes=torch.from_numpy(gold["classes"]))
    S = g.inp_size
    bits, area, box = XO.pack(r["masks"].numpy())
    B, K = gold["classes"].shape
    assert bits.shape == (B, K, S * S // 8)
    got = XO.unpack(bits, S, S).reshape(B, K, -1)[:, :, gold["pos"]]
    ref = gold["masks_at_pos"]
    clear = np.abs(ref) > 1e-3
    print(f"tiny hypotheses: {int((~clear).sum())} of {clear.size} reference values within 1e-3 of zero; areas {area.min()} .. {area.max()}")
    assert clear.mean() > 0.999 and np.array_equal(got[clear], (ref > 0)[clear])
    it = XO.inter(bits)
    assert all(np.array_equal(np.diagonal(it[b]), area[b]) for b in range(B))
    assert area.min() > 0 and (box[..., 0] <= box[..., 2]).all() and (box[..., 1] <= box[..., 3]).all()


# ---- the two entries refuse before they launch -------------------------------------------------------------------------------------
def test_mask_pack_refuses_bad_arguments_without_gpu():
    lib = hip.load()
    p = 4096
    ok = dict(logits=p, P=2, HW=64, W=8, bits=p, area=p, box=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cvlm_mask_pack(a["logits"], a["P"], a["HW"], a["W"], a["bits"], a["area"], a["box"], None)
    for kw in (dict(logits=None), dict(bits=None), dict(bits=p + 2), dict(area=None), dict(box=None), dict(P=0), dict(P=65536), dict(HW=0),
               dict(HW=-32), dict(HW=2 ** 31), dict(HW=2 ** 32 + 64), dict(HW=40, W=8), dict(HW=48, W=8), dict(W=0), dict(W=-8),
               dict(W=7), dict(HW=96, W=64)):
        assert call(**kw) == -1, kw


def test_mask_overlap_refuses_bad_arguments_without_gpu():
    lib = hip.load()
    p = 4096
    ok = dict(bits=p, n=2, K=3, words=8, inter=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cvlm_mask_overlap(a["bits"], a["n"], a["K"], a["words"], a["inter"], None)
    for kw in (dict(bits=None), dict(inter=None), dict(n=0), dict(K=0), dict(K=1025), dict(n=64, K=1024), dict(n=65536, K=1),
               dict(words=0), dict(words=-1), dict(words=2 ** 26), dict(words=2 ** 40)):
        assert call(**kw) == -1, kw
