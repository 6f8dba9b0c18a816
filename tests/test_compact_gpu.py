"""Packed masks, areas, boxes and overlaps of class hypotheses: the two kernels (cvlm_mask_pack, cvlm_mask_overlap)
against the numpy oracle (tests/compact_oracle.py), exactly -- every output is an integer --, masks="both" / "bits" and overlaps=True of
Cascade.infer_classes / decode against the default call and the oracle, the memory condition of masks="bits", and the demo geometry
against the reference's own bits (tests/golden/demo_classes_digest.npz) within the bounds set arithmetic gives."""
import dataclasses
import os
import sys
import types

import numpy as np
import pytest
import torch

import compact_oracle as XO
from test_classes_gpu import IOU, build_tiny, demo_engines, demo_inputs, demo_sd, dgold  # noqa: F401  (fixtures of the demo geometry)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def run_pack(planes: torch.Tensor, stats: bool = True):
    """hip.mask_pack on (P, H, W) device planes into sentinel-filled outputs -> numpy (bits, area, box)."""
    from camouflaged_vlm_amd import hip
    P, H, W = planes.shape
    bits = torch.full((P, H * W // 8), 0xA5, dtype=torch.uint8, device=planes.device)
    area = torch.full((P,), -77, dtype=torch.int32, device=planes.device) if stats else None
    box = torch.full((P, 4), -77, dtype=torch.int32, device=planes.device) if stats else None
    hip.mask_pack(planes, bits, area, box)
    torch.cuda.synchronize()
    return (bits.cpu().numpy(),) + ((area.cpu().numpy(), box.cpu().numpy()) if stats else ())


def assert_pack(m: np.ndarray, tag, shift: int = 0):
    """Exact equality of cvlm_mask_pack with the oracle on host planes m (P, H, W); shift: floats the base is moved off 16 bytes."""
    want = XO.pack(m)
    flat = torch.zeros(shift + m.size, device=DEV)
    flat[shift:] = torch.from_numpy(m).reshape(-1).to(DEV)
    planes = flat[shift:].view(m.shape)
    assert planes.data_ptr() % 16 == (4 * shift) % 16
    got = run_pack(planes)
    for name, g, w in zip(("bits", "area", "box"), got, want):
        assert np.array_equal(g, w), (tag, name)
    assert np.array_equal(run_pack(planes, stats=False)[0], want[0]), (tag, "bits alone")


# ---- cvlm_mask_pack --------------------------------------------------------------------------------------------------------------
# (1, 4, 8): one word; (3, 8, 12): 96 pixels, half a wave of 16-byte loads; (2, 16, 20): 320 pixels, not a multiple of 256;
# (5, 320, 320): the tiny geometry's planes, 100 workgroups each; (1000, 64, 64): three workgroups per plane walk four workgroups'
# worth in two rounds, the second one partly past the end
@pytest.mark.parametrize("P,H,W", [(1, 4, 8), (3, 8, 12), (2, 16, 20), (5, 320, 320), (1000, 64, 64)])
def test_mask_pack_is_packbits_area_and_box(P, H, W):
    rng = np.random.default_rng(100 * P + W)
    normal = rng.standard_normal((P, H, W)).astype(np.float32)
    assert_pack(normal, "N(0, 1)")
    assert_pack(normal, "N(0, 1), base 4 bytes off a 16-byte boundary", shift=1)
    if P > 5:
        return
    assert_pack(np.zeros((P, H, W), np.float32), "all zero")
    assert_pack(np.abs(normal) + 1e-3, "all positive")
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 3)):
        m = -np.abs(normal)
        m[:, y, x] = 0.25
        if P > 1:
            m[1, y, x] = -0.25                                     # and one plane left empty
        assert_pack(m, f"single pixel ({y}, {x})")
    sparse = np.where(rng.random((P, H, W)) < 0.02, 1.0, -1.0).astype(np.float32)
    assert_pack(sparse, "sparse")


def test_mask_pack_special_values():
    """logit > 0.0f: +0.0, -0.0, NaN (either sign), -inf, negative denormals and -1e-38 give 0; +inf, positive denormals, 1e-38 give 1."""
    vals = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -1e-40, 1e-38, -1e-38, 1.0, -1.0,
                     np.finfo(np.float32).max, -np.finfo(np.float32).max], np.float32)
    neg_nan = np.array([0xffc00001, 0x7f800001, 0xff800001, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000],
                       np.uint32).view(np.float32)                # quiet / signalling NaNs of both signs, the extreme denormals
    vals = np.concatenate([vals, neg_nan])
    rng = np.random.default_rng(7)
    m = vals[rng.integers(0, len(vals), (4, 16, 24))]
    m[0].reshape(-1)[:len(vals)] = vals                               # every value at least once, in a known place
    want_first = [0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 1]
    assert ((m[0].reshape(-1)[:len(vals)] > 0).astype(int).tolist()) == want_first
    assert_pack(m, "special values")
    assert_pack(m, "special values, element loads", shift=3)


def test_mask_pack_refuses_without_launching():
    from camouflaged_vlm_amd import hip
    lib = hip.load()
    logits = torch.randn(2, 96, device=DEV)
    bits = torch.full((2, 12), 0xA5, dtype=torch.uint8, device=DEV)
    area = torch.full((2,), -77, dtype=torch.int32, device=DEV)
    box = torch.full((2, 4), -77, dtype=torch.int32, device=DEV)
    call = lambda P, HW, W, a, b: lib.cvlm_mask_pack(logits.data_ptr(), P, HW, W, bits.data_ptr(), a, b, None)
    assert call(2, 40, 8, area.data_ptr(), box.data_ptr()) == -1      # HW not a multiple of 32
    assert call(2, 96, 36, area.data_ptr(), box.data_ptr()) == -1     # W does not divide HW
    assert call(2, 96, 12, area.data_ptr(), None) == -1               # area without box
    assert call(2, 96, 12, None, box.data_ptr()) == -1                # box without area
    with pytest.raises(AssertionError):
        hip.mask_pack(logits.view(2, 8, 12), bits, area, None)
    torch.cuda.synchronize()
    assert bool((bits == 0xA5).all()) and bool((area == -77).all()) and bool((box == -77).all())
    assert call(2, 96, 12, area.data_ptr(), box.data_ptr()) == 0      # and the same buffers are served
    torch.cuda.synchronize()
    want = XO.pack(logits.cpu().numpy().reshape(2, 8, 12))
    assert np.array_equal(bits.cpu().numpy(), want[0]) and np.array_equal(area.cpu().numpy(), want[1])
    assert np.array_equal(box.cpu().numpy(), want[2])


def test_mask_pack_offsets_past_2_31_bytes():
    """520 planes of 1024 x 1024: the last plane starts 2.03 GiB into the logits.  A few pixels in the first and the last plane."""
    P, S = 520, 1024
    planes = torch.zeros(P, S, S, device=DEV)
    px = {0: [(0, 0), (5, 1000), (1023, 1023)], P - 1: [(3, 7), (700, 2), (1023, 0), (512, 512)]}
    for p, pts in px.items():
        for y, x in pts:
            planes[p, y, x] = 1.0
    from camouflaged_vlm_amd import hip
    bits = torch.full((P, S * S // 8), 0xA5, dtype=torch.uint8, device=DEV)
    area = torch.full((P,), -77, dtype=torch.int32, device=DEV)
    box = torch.full((P, 4), -77, dtype=torch.int32, device=DEV)
    hip.mask_pack(planes, bits, area, box)
    torch.cuda.synchronize()
    for p in px:
        wb, wa, wx = XO.pack(planes[p].cpu().numpy()[None])
        assert np.array_equal(bits[p].cpu().numpy(), wb[0]) and int(area[p]) == int(wa[0]) == len(px[p])
        assert box[p].tolist() == wx[0].tolist()
    assert box[0].tolist() == [0, 0, 1023, 1023] and box[P - 1].tolist() == [0, 3, 512, 1023]
    assert not bool(bits[1:P - 1].any()) and not bool(area[1:P - 1].any()) and bool((box[1:P - 1] == -1).all())


# ---- cvlm_mask_overlap -----------------------------------------------------------------------------------------------------------
def random_bits(rng, n: int, K: int, words: int) -> np.ndarray:
    """uint8 [n][K][4 * words]: planes of density 0.1 / 0.5 / 0.9 in turn, an all-zero and an all-ones plane among them."""
    dens = np.array([0.1, 0.5, 0.9])[(np.arange(n * K) % 3)].reshape(n, K, 1)
    bits = np.packbits(rng.random((n, K, 32 * words)) < dens, axis=-1)
    if K >= 3:
        bits[0, 1], bits[0, 2] = 0, 255
    elif K == 2:
        bits[0, 0], bits[n - 1, 1] = 255, 0
    elif n >= 3:
        bits[1, 0], bits[2, 0] = 0, 255
    return bits


def assert_overlap(bits: np.ndarray, tag):
    from camouflaged_vlm_amd import hip
    n, K, _ = bits.shape
    inter = torch.full((n, K, K), -12345, dtype=torch.int32, device=DEV)          # garbage: the call zeroes it
    hip.mask_overlap(torch.from_numpy(bits).to(DEV), inter)
    torch.cuda.synchronize()
    assert np.array_equal(inter.cpu().numpy(), XO.inter(bits)), tag


# K = 65: one more than a wave, three tiles of 32 rows; words = 1 and 3: element loads, a fraction of one staged tile; words = 1000:
# 16-byte loads, eight staged tiles, the last one partial
@pytest.mark.parametrize("words", [1, 3, 1000])
@pytest.mark.parametrize("K", [1, 2, 5, 61, 65])
def test_mask_overlap_is_the_boolean_matrix_product(K, words):
    rng = np.random.default_rng(1000 * K + words)
    for n in (1, 3):
        assert_overlap(random_bits(rng, n, K, words), (n, K, words))


def test_mask_overlap_long_rows_many_images():
    """20 images x 33 hypotheses x 2600 words: 60 pair tiles leave 17 workgroups per tile for 21 staged tiles of words, so every
    workgroup walks two -- the loop the demo geometry runs (32 768 words per plane)."""
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 256, (20, 33, 4 * 2600), dtype=np.uint8)               # density 1 / 2 ...
    bits[:, ::2] &= rng.integers(0, 256, (20, 17, 4 * 2600), dtype=np.uint8)      # ... and 1 / 4 on every other plane
    assert_overlap(bits, "long rows")


def test_mask_overlap_refuses_without_launching():
    from camouflaged_vlm_amd import hip
    lib = hip.load()
    bits = torch.zeros(1025 * 4, dtype=torch.uint8, device=DEV)
    inter = torch.full((8,), -12345, dtype=torch.int32, device=DEV)
    assert lib.cvlm_mask_overlap(bits.data_ptr(), 1, 1025, 1, inter.data_ptr(), None) == -1
    assert lib.cvlm_mask_overlap(bits.data_ptr(), 1, 0, 1, inter.data_ptr(), None) == -1
    assert lib.cvlm_mask_overlap(None, 1, 2, 1, inter.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert bool((inter == -12345).all())


# ---- tiny geometry, exact ----------------------------------------------------------------------------------------------------------
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


KEPT = ("classes", "pass1_logits", "logits", "pred")
COMPACT = ("mask_bits", "area", "box", "inter")


def snapshot(h):
    """Copies of a default call's tensors: a later call may reuse nothing of them, but the comparison should not depend on that."""
    return types.SimpleNamespace(**{f: getattr(h, f).clone() for f in KEPT + ("masks", "edges")})


def equal_fields(x, y, fields) -> bool:
    return all(torch.equal(getattr(x, f), getattr(y, f)) for f in fields)


def assert_compact_is_oracle(h, masks: torch.Tensor):
    """mask_bits = packbits(masks > 0); area, box and inter = the oracle on those bits."""
    n, K, S, _ = masks.shape
    wb, wa, wx = XO.pack(masks.cpu().numpy())
    assert h.mask_bits.shape == (n, K, S * S // 8) and h.mask_bits.dtype == torch.uint8
    assert h.area.shape == (n, K) and h.area.dtype == torch.int32 and h.box.shape == (n, K, 4) and h.box.dtype == torch.int32
    assert h.inter.shape == (n, K, K) and h.inter.dtype == torch.int32
    assert np.array_equal(h.mask_bits.cpu().numpy(), wb)
    assert np.array_equal(h.area.cpu().numpy(), wa) and np.array_equal(h.box.cpu().numpy(), wx)
    assert np.array_equal(h.inter.cpu().numpy(), XO.inter(wb))


def check_both_and_bits(default, call):
    """`call(**kw)` runs one entry point with the arguments of `default`'s call plus kw."""
    both = call(masks="both", overlaps=True)
    torch.cuda.synchronize()
    assert equal_fields(both, default, KEPT + ("masks", "edges"))
    assert_compact_is_oracle(both, both.masks)
    area = both.area.cpu().numpy()
    print("areas", area.tolist(), "of", both.masks.shape[-1] ** 2)
    assert area.min() > 0                                                         # non-degenerate: the hypotheses have pixels
    kept = {f: getattr(both, f).clone() for f in KEPT + COMPACT}
    bits = call(masks="bits", overlaps=True)
    torch.cuda.synchronize()
    assert bits.masks is None and bits.edges is None
    for f, t in kept.items():
        assert torch.equal(getattr(bits, f), t), f
    plain = call(masks="bits")
    torch.cuda.synchronize()
    assert plain.inter is None and plain.masks is None and equal_fields(plain, bits, KEPT + COMPACT[:3])
    return both, bits


def test_infer_classes_both_and_bits(tiny, cas):
    _, _, _, (inp, ci, cm), _ = tiny
    default = cas.infer_classes(inp, ci, cm, topk=5)
    assert default.mask_bits is None and default.area is None and default.box is None and default.inter is None
    default = snapshot(default)
    check_both_and_bits(default, lambda **kw: cas.infer_classes(inp, ci, cm, topk=5, **kw))


def test_infer_classes_bits_with_quality(tiny, cas):
    _, _, _, (inp, ci, cm), _ = tiny
    default = cas.infer_classes(inp, ci, cm, topk=5, quality=True)
    want_iou = default.iou.clone()
    default = snapshot(default)
    both, bits = check_both_and_bits(default, lambda **kw: cas.infer_classes(inp, ci, cm, topk=5, quality=True, **kw))
    assert torch.equal(both.iou, want_iou) and torch.equal(bits.iou, want_iou)


@pytest.mark.parametrize("images", [None, [1, 0, 1]])
def test_decode_both_and_bits(tiny, cas, images):
    _, _, _, (inp, ci, cm), _ = tiny
    enc = cas.encode(inp, ci, cm)
    default = snapshot(cas.decode(enc, topk=5, images=images))
    both, bits = check_both_and_bits(default, lambda **kw: cas.decode(enc, topk=5, images=images, **kw))
    assert both.mask_bits.shape[0] == (2 if images is None else 3)
    if images is not None:                                        # images 1, 0, 1: rows 0 and 2 are the same hypotheses
        assert torch.equal(bits.mask_bits[0], bits.mask_bits[2]) and torch.equal(bits.inter[0], bits.inter[2])
    q = cas.decode(enc, topk=5, images=images, quality=True)
    want_iou = q.iou.clone()
    qb = cas.decode(enc, topk=5, images=images, quality=True, masks="bits", overlaps=True)
    torch.cuda.synchronize()
    assert torch.equal(qb.iou, want_iou) and equal_fields(qb, bits, KEPT + COMPACT) and qb.masks is None
    s = cas.decode(enc, topk=5, images=images, stage2=False, masks="bits", overlaps=True)
    torch.cuda.synchronize()
    assert s.logits is None and s.pred is None and equal_fields(s, bits, COMPACT + ("classes",))


def test_nan_pass1_row_gives_empty_masks(tiny, gold):
    """A pass-1 row holding a NaN has no order (as tests/test_classes_gpu.py plants one for cvlm_topk_select): classes -1, masks NaN
    -- zero bits, area 0, box -1 and a zero row and column in `inter`; the other image is served as ever.  An engine of its own and
    no stage 2: no NaN reaches the CLIP tower of the module's engine."""
    _, _, _, (inp, ci, cm), _ = tiny
    cas = build_tiny(tiny, gold)
    enc = cas.encode(inp, ci, cm)
    good = cas.decode(enc, topk=3, masks="bits", overlaps=True, stage2=False)
    good = {f: getattr(good, f).clone() for f in COMPACT}
    p1 = enc.pass1_logits.clone()
    p1[1, 2] = float("nan")
    for mode in ("both", "bits"):
        h = cas.decode(dataclasses.replace(enc, pass1_logits=p1), topk=3, masks=mode, overlaps=True, stage2=False)
        torch.cuda.synchronize()
        assert h.classes[1].tolist() == [-1] * 3 and h.classes[0].tolist() == torch.topk(enc.pass1_logits[0], 3).indices.tolist()
        if mode == "both":
            assert bool(torch.isnan(h.masks[1]).all())
        assert not bool(h.mask_bits[1].any()) and h.area[1].tolist() == [0] * 3 and h.box[1].tolist() == [[-1] * 4] * 3
        assert not bool(h.inter[1].any())
        for f, t in good.items():
            assert torch.equal(getattr(h, f)[0], t[0]), f


def test_pack_masks_of_infer_test(tiny, cas):
    g, _, _, (inp, ci, cm), _ = tiny
    m = cas.infer_test(inp, ci, cm).clone()                       # (B, 1, S, S)
    want = XO.pack(m[:, 0].cpu().numpy())
    for arg in (m, m[:, 0]):
        got = cas.pack_masks(arg)
        torch.cuda.synchronize()
        assert all(np.array_equal(t.cpu().numpy(), w) for t, w in zip(got, want))
    for bad in (m.double(), m.cpu(), m[0, 0], m.expand(2, 2, g.inp_size, g.inp_size), m[:, :, :5, :5], [m]):
        with pytest.raises(ValueError):
            cas.pack_masks(bad)


def test_bad_compact_requests_raise_and_launch_nothing(tiny, cas):
    from camouflaged_vlm_amd import hip
    _, _, _, (inp, ci, cm), _ = tiny
    enc = cas.encode(inp, ci, cm)
    torch.cuda.synchronize()
    calls = []
    names = ("gemm", "layernorm", "topk_select", "patchify", "split_f32", "expand_blocks", "bilinear", "mask_pack", "mask_overlap")
    saved = {n: getattr(hip, n) for n in names}
    for n in saved:
        setattr(hip, n, lambda *a, _n=n, **k: calls.append(_n))
    try:
        for kw in (dict(masks="packed"), dict(masks=None), dict(overlaps=True), dict(masks="logits", overlaps=True),
                   dict(masks="bits", overlaps=1)):
            with pytest.raises(ValueError):
                cas.infer_classes(inp, ci, cm, topk=2, **kw)
            with pytest.raises(ValueError):
                cas.decode(enc, topk=2, **kw)
        big = torch.zeros(2, 1025, dtype=torch.int64)                         # K = 1025 hypotheses: one more than the overlap takes
        with pytest.raises(ValueError):
            cas.infer_classes(inp, ci, cm, classes=big, masks="bits", overlaps=True)
        with pytest.raises(ValueError):
            cas.decode(enc, classes=big, masks="both", overlaps=True)
    finally:
        for n, f in saved.items():
            setattr(hip, n, f)
    assert calls == []


def test_bits_mode_allocates_no_plane_tensor(tiny, cas, monkeypatch):
    """10 prompts in 3 passes of at most 4: after one call per mode has sized the grow-only workspace, the peak of a masks="bits"
    call over its starting level stays below P * S * S * 4 bytes -- one (n, K, S, S) f32 tensor; the default call allocates two."""
    g, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    P, S = 10, g.inp_size
    plane_bytes = P * S * S * 4
    modes = {"logits": dict(), "bits": dict(masks="bits", overlaps=True)}
    for kw in modes.values():
        cas.infer_classes(inp, ci, cm, topk=5, **kw)
    torch.cuda.synchronize()
    peak = {}
    for name, kw in modes.items():
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        h = cas.infer_classes(inp, ci, cm, topk=5, **kw)
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - start
        del h
    print(f"peak over the starting level, 10 prompts of {S} x {S}: default {peak['logits']} B, bits {peak['bits']} B; "
          f"one plane tensor {plane_bytes} B")
    assert peak["bits"] < plane_bytes
    assert peak["logits"] >= 2 * plane_bytes


# ---- drop-in ---------------------------------------------------------------------------------------------------------------------
def test_dropin_passes_masks_and_overlaps_through(tiny, gold, golden_dir):
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
    with torch.no_grad():
        want = model.cascade().infer_classes(inp, ci, cm, topk=3, masks="bits", overlaps=True)
        want = {f: getattr(want, f).clone() for f in KEPT + COMPACT}
        got = model.infer_classes(inp, ci, cm, topk=3, masks="bits", overlaps=True)
        dec = model.decode_classes(model.encode_images(inp, ci, cm), topk=3, masks="both", overlaps=True)
        torch.cuda.synchronize()
        assert got.masks is None and all(torch.equal(getattr(got, f), t) for f, t in want.items())
        assert_compact_is_oracle(dec, dec.masks)
        m = model.infer_test(inp, ci, cm)
        b, a, x = model.pack_masks(m)
        torch.cuda.synchronize()
        wb, wa, wx = XO.pack(m[:, 0].cpu().numpy())
        assert np.array_equal(b.cpu().numpy(), wb) and np.array_equal(a.cpu().numpy(), wa) and np.array_equal(x.cpu().numpy(), wx)


# ---- demo geometry, mx: against the reference's own bits -----------------------------------------------------------------------------
def test_demo_bits_against_the_reference_bits(demo_engines, dgold, demo_inputs):
    """Per hypothesis d = |engine XOR reference|.  With A the engine's mask and R the reference's: |A & R| = (|A| + |R| - d) / 2 and
    |A | R| = (|A| + |R| + d) / 2, so the IoU follows from `area` and d (gate: the project's 0.999); ||A| - |R|| <= d; and an
    intersection of two hypotheses moves by at most the pixels either one changed, d_a + d_b."""
    cas = demo_engines["mx"]
    inp, ci, cm = demo_inputs
    h = cas.infer_classes(inp, ci, cm, classes=torch.from_numpy(dgold["classes"]), masks="bits", overlaps=True)
    torch.cuda.synchronize()
    ref = dgold["mask_bits"]
    B, K, nb = ref.shape
    assert h.masks is None and h.edges is None and tuple(h.mask_bits.shape) == (B, K, nb)
    got = h.mask_bits.cpu().numpy()
    area, box, inter = h.area.cpu().numpy(), h.box.cpu().numpy(), h.inter.cpu().numpy()
    S = cas.g.inp_size
    ra, rx = XO.stats(XO.unpack(ref, S, S))
    ri = XO.inter(ref)
    d = np.unpackbits(got ^ ref, axis=-1).sum(-1).astype(np.int64)
    # the engine's counts are those of its own bits, exactly
    wa, wx = XO.stats(XO.unpack(got, S, S))
    assert np.array_equal(area, wa) and np.array_equal(box, wx) and np.array_equal(inter, XO.inter(got))
    for b in range(B):
        for k in range(K):
            io = (area[b, k] + ra[b, k] - d[b, k]) / max(area[b, k] + ra[b, k] + d[b, k], 1)
            print(f"demo mx image {b} class {int(dgold['classes'][b, k])}: d = {d[b, k]}, area {area[b, k]} / {ra[b, k]}, IoU {io:.6f}, "
                  f"box {box[b, k].tolist()} / {rx[b, k].tolist()}")
            assert io >= IOU and abs(int(area[b, k]) - int(ra[b, k])) <= d[b, k]
            for j in range(K):
                assert abs(int(inter[b, k, j]) - int(ri[b, k, j])) <= d[b, k] + d[b, j], (b, k, j)
    assert h.pred.tolist() == dgold["pred"].tolist()
