"""Masks at each image's own size on the device: cvlm_mask_pack_sized against tests/sized_oracle.py -- the arithmetic
cases under the rule of the oracle module (a pixel is left out only where the fp64 value of 255 v lies within 2.5e-4 of the level, at
most max(2, 1e-4 pixels) of a plane), the geometry cases exactly --, ragged planes in one launch with guard bands inside the same
tensor, tables that disagree with their sizes, a logits base off 16 bytes; cvlm_mask_rle_count_w / cvlm_mask_rle_emit_w against
tests/rle_oracle.py's definition on the unpadded plane; Cascade.pack_masks_sized / mask_rle_sized; sizes= / rle="sized" of
Cascade.infer_classes / decode / the drop-in against the oracle on the call's own planes and against the call without them.

Figures of the MI355X run this file was written with are in DESIGN.md §19."""
import os
import sys

import numpy as np
import pytest
import torch

import rle_oracle as RO
import sized_oracle as SO
from test_classes_gpu import build_tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def device_pack():
    from camouflaged_vlm_amd import hip
    return hip.mask_pack_sized


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", SO.ARITH)
def test_field_equals_the_oracle(src, dst):
    logits = SO.field(src, dst)
    for level in SO.LEVELS:
        _, planes, area, box, status = SO.run(device_pack(), logits[None], [dst], level, dev=DEV)
        assert status == 0
        SO.compare(planes[0], area[0], box[0], logits, *dst, level)


def test_geometry_cases_are_exact():
    """All cases of one source size as the planes of ONE call per level (they are ragged: 32 sizes), the others on their own: all bits,
    pad bits, area and box, no pixel left out."""
    cases = SO.geometry_cases()
    shared = [c for c in cases if c[1].shape == (24, 40)]
    assert len(shared) >= 30
    for level in SO.GEOMETRY_LEVELS:
        logits = np.stack([c[1] for c in shared])
        sizes = [c[2] for c in shared]
        _, planes, area, box, status = SO.run(device_pack(), logits, sizes, level, dev=DEV)
        assert status == 0
        for p, (name, lg, (h, w)) in enumerate(shared):
            SO.compare(planes[p], area[p], box[p], lg, h, w, level, exact=True)
            if name == "nan":
                assert area[p] == 0 and box[p].tolist() == [-1] * 4 and not planes[p].any()
        for name, lg, (h, w) in cases:
            if lg.shape != (24, 40):
                _, planes, area, box, status = SO.run(device_pack(), lg[None], [(h, w)], level, dev=DEV)
                assert status == 0
                SO.compare(planes[0], area[0], box[0], lg, h, w, level, exact=True)


@pytest.fixture(scope="module")
def ragged():
    rng = np.random.default_rng(19)
    logits = rng.normal(0, 3, (7, 24, 40)).astype(np.float32)
    _, planes, area, box, status = SO.run(device_pack(), logits, SO.RAGGED, 128, dev=DEV)
    assert status == 0
    return logits, planes, area, box


def test_ragged_planes_in_one_launch(ragged):
    """Seven planes of seven sizes in one call; the bands before the first and behind the last plane keep their sentinel (SO.run), the
    pad bits inside the planes are 0 (SO.compare).  Without statistics the bits are the same."""
    logits, planes, area, box = ragged
    for p, (h, w) in enumerate(SO.RAGGED):
        SO.compare(planes[p], area[p], box[p], logits[p], h, w, 128)
    _, bare, a, _, status = SO.run(device_pack(), logits, SO.RAGGED, 128, dev=DEV, stats_out=False)
    assert status == 0 and a is None and all(np.array_equal(x, y) for x, y in zip(bare, planes))


def test_tables_that_disagree_are_refused_not_overrun(ragged):
    """A plane whose slice is not its size's length, an end beyond the byte length, a negative and a misaligned start: status 1, the
    refused plane's slice and every band untouched -- a refused slice is a band BETWEEN planes --, the other planes whole."""
    logits, planes, _, _ = ragged
    sizes = SO.RAGGED
    _, off, _, _ = SO.tables(sizes)
    bad = off.copy()
    bad[3:] += 4
    _, got, area, box, status = SO.run(device_pack(), logits, sizes, 128, dev=DEV, offsets=bad)
    assert status == 1 and got[2] is None and area[2] == 0 and box[2].tolist() == [-1] * 4
    assert all(np.array_equal(got[p], planes[p]) for p in (0, 1, 3, 4, 5, 6))
    _, got, area, _, status = SO.run(device_pack(), logits, sizes, 128, dev=DEV, nbytes=int(off[-1]) - 4)
    assert status == 1 and got[6] is None and area[6] == 0 and all(np.array_equal(got[p], planes[p]) for p in range(6))
    for first in (-4, SO.GUARD + 2):
        bad = off.copy()
        bad[0] = first
        _, got, _, _, status = SO.run(device_pack(), logits, sizes, 128, dev=DEV, offsets=bad)
        assert status == 1 and got[0] is None and all(np.array_equal(got[p], planes[p]) for p in range(1, 7))
    # sizes in the device table outside 1 .. 16384 (the wrapper checks them before upload; the kernel does not trust them)
    from camouflaged_vlm_amd import hip
    for size in ((0, 8), (8, -2), (8, 16385), (2 ** 31 - 1, 2 ** 31 - 1)):
        dims = torch.tensor([[4, 8], list(size)], dtype=torch.int32, device=DEV)
        o = torch.tensor([0, 16, 80], dtype=torch.int64, device=DEV)
        bits = torch.full((80,), SO.FILL, dtype=torch.uint8, device=DEV)
        a, b, s = (torch.empty(n, dtype=torch.int32, device=DEV) for n in ((2,), (2, 4), (1,)))
        hip.mask_pack_sized(torch.zeros(2, 8, 8, device=DEV), dims, o, 128, bits, 64, a, b, s)
        assert s.item() == 1 and bool((bits[16:] == SO.FILL).all()) and not bool(bits[:16].any()) and a.tolist() == [0, 0], size


def test_logits_off_a_sixteen_byte_boundary(ragged):
    logits, planes, area, box = ragged
    flat = torch.zeros(logits.size + 1, device=DEV)
    src = flat[1:].view(logits.shape)
    src.copy_(torch.from_numpy(logits))
    assert src.data_ptr() % 16 == 4
    _, got, a, b, status = SO.run(device_pack(), src, SO.RAGGED, 128, dev=DEV)
    assert status == 0 and np.array_equal(a, area) and np.array_equal(b, box) and all(np.array_equal(x, y) for x, y in zip(got, planes))


# ---- run-length encoding with a true width -----------------------------------------------------------------------------------------------
def device_rle_w(bits: np.ndarray, H: int, Wt: int, guard: int = 5):
    """hip.mask_rle_count_w then hip.mask_rle_emit_w into one sentinel-filled counts tensor with `guard` elements before, between and
    behind the slices -> (n_runs, each plane's counts)."""
    from camouflaged_vlm_amd import hip
    W = 32 * ((Wt + 31) // 32)
    b = torch.from_numpy(np.ascontiguousarray(bits)).to(DEV)
    P = b.shape[0]
    n = torch.full((P,), -7, dtype=torch.int32, device=DEV)
    hip.mask_rle_count_w(b, H, W, Wt, n)
    runs = n.cpu().numpy().astype(np.int64)
    off = np.zeros(P + 1, dtype=np.int64)
    off[1:] = np.cumsum(runs + guard)
    off += guard
    total = int(off[P]) + guard
    counts = torch.full((total,), -9, dtype=torch.int32, device=DEV)
    status = torch.full((1,), -3, dtype=torch.int32, device=DEV)
    ws = torch.empty(hip.mask_rle_workspace_bytes(P, H, W), dtype=torch.uint8, device=DEV)
    hip.mask_rle_emit_w(b, H, W, Wt, torch.from_numpy(off).to(DEV), counts, status, ws)
    torch.cuda.synchronize()
    assert status.item() == 0
    c = counts.cpu().numpy()
    keep = np.ones(total, dtype=bool)
    out = []
    for p in range(P):
        keep[off[p]:off[p] + runs[p]] = False
        out.append(c[off[p]:off[p] + runs[p]])
    assert (c[keep] == -9).all(), "an element outside the planes' counts was overwritten"
    return runs, out


@pytest.mark.parametrize("H,Wt", SO.RLE_SIZES)
def test_rle_with_a_true_width_equals_the_definition_on_the_unpadded_plane(H, Wt):
    from camouflaged_vlm_amd import rle
    cases = SO.rle_cases(H, Wt)
    planes = np.stack(list(cases.values()))
    want = [RO.plane_counts(m) for m in planes]
    for garbage in (False, True):                                     # whatever the pad bits hold
        n, got = device_rle_w(SO.pack_planes(planes, garbage, seed=H + Wt), H, Wt)
        assert n.tolist() == [len(w) for w in want]
        for name, g, w, m in zip(cases, got, want, planes):
            assert np.array_equal(g, w), (name, garbage)
            assert int(g.sum()) == H * Wt and np.array_equal(rle.decode(g, H, Wt), m), name


@pytest.mark.parametrize("H,W", [(8, 64), (33, 64), (65, 96)])
def test_true_width_equal_to_the_pitch_is_the_existing_entry(H, W):
    from camouflaged_vlm_amd import hip
    bits = RO.pack(np.stack(list(RO.cases(H, W).values())))
    n, got = device_rle_w(bits, H, W, guard=0)
    b = torch.from_numpy(bits).to(DEV)
    P = b.shape[0]
    old_n = torch.empty(P, dtype=torch.int32, device=DEV)
    hip.mask_rle_count(b, H, W, old_n)
    off = torch.zeros(P + 1, dtype=torch.int64, device=DEV)
    off[1:] = torch.cumsum(old_n.long(), 0)
    counts = torch.full((int(off[-1].item()),), -9, dtype=torch.int32, device=DEV)
    status = torch.empty(1, dtype=torch.int32, device=DEV)
    hip.mask_rle_emit(b, H, W, off, counts, status, torch.empty(hip.mask_rle_workspace_bytes(P, H, W), dtype=torch.uint8, device=DEV))
    assert status.item() == 0 and old_n.cpu().tolist() == n.tolist()
    assert np.array_equal(counts.cpu().numpy(), np.concatenate(got))


# ---- tiny geometry, exact ------------------------------------------------------------------------------------------------------------------
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


def assert_rle_is_oracle(r, masks: list):
    """A MaskRle = the definition on the given bool planes of any sizes: n_runs, offsets without gaps, counts; to_coco carries each
    plane's own size and decodes back, plain and compressed."""
    from camouflaged_vlm_amd import rle
    want = [RO.plane_counts(m) for m in masks]
    assert r.n_runs.cpu().tolist() == [len(w) for w in want]
    assert r.offsets.cpu().tolist() == [0] + np.cumsum([len(w) for w in want]).tolist()
    assert r.counts.dtype == torch.int32 and np.array_equal(r.counts.cpu().numpy(), np.concatenate(want))
    for compressed in (False, True):
        coco = r.to_coco(compressed=compressed)
        assert len(coco) == len(masks)
        for d, m in zip(coco, masks):
            c = rle.string_to_counts(d["counts"]) if compressed else d["counts"]
            assert d["size"] == list(m.shape) and int(np.sum(c)) == m.size and np.array_equal(rle.decode(c, *m.shape), m)


def test_pack_masks_sized_and_mask_rle_sized_on_ragged_planes(cas, ragged, monkeypatch):
    from camouflaged_vlm_amd.engine import SizedMasks
    logits, planes, area, box = ragged
    src = torch.from_numpy(logits).to(DEV)
    s = cas.pack_masks_sized(src[:, None], SO.RAGGED)
    assert isinstance(s, SizedMasks) and s.sizes == SO.RAGGED and s.level == 128
    s.check()
    assert np.array_equal(s.area.cpu().numpy(), area) and np.array_equal(s.box.cpu().numpy(), box)
    assert s.offsets.cpu().tolist() == (SO.tables(SO.RAGGED)[1] - SO.GUARD).tolist() and s.bits.numel() == s.offsets[-1].item()
    masks = []
    for p, (h, w) in enumerate(SO.RAGGED):
        assert np.array_equal(s.plane(p).cpu().numpy(), planes[p]) and s.plane(p).data_ptr() == s.bits.data_ptr() + s.byte_range(p)[0]
        masks.append(s.to_numpy(p))
        assert masks[-1].shape == (h, w) and np.array_equal(masks[-1], SO.unpack_rows(planes[p], w))
    overlay = cas.pack_masks_sized(src, SO.RAGGED, level=1)           # the demo's `> 0`
    assert all(int(overlay.area[p]) >= int(s.area[p]) for p in range(7)) and int(overlay.area.sum()) > int(s.area.sum())
    # the encoding: ONE synchronisation
    torch.cuda.synchronize()
    reads = []
    for name in ("item", "cpu", "tolist", "numpy"):
        real = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _real=real, _n=name, **k: (reads.append(_n), _real(self, *a, **k))[1])
    r = cas.mask_rle_sized(s)
    monkeypatch.undo()
    assert reads == ["item"], reads
    assert r.size is None and r.sizes == SO.RAGGED and r.status.numel() == 1
    assert_rle_is_oracle(r, masks)
    same = cas.mask_rle_sized(cas.pack_masks_sized(src[:3], [(33, 31)] * 3))                         # one run of three planes
    assert same.size == (33, 31)
    for bad in (dict(sizes=SO.RAGGED[:6]), dict(sizes=[(0, 1)] * 7), dict(level=0), dict(level=256), dict(sizes=None),
                dict(logits=src.cpu()), dict(logits=src.double()), dict(logits=src[0])):
        kw = dict(dict(logits=src, sizes=SO.RAGGED, level=128), **bad)
        with pytest.raises(ValueError):
            cas.pack_masks_sized(kw["logits"], kw["sizes"], level=kw["level"])
    with pytest.raises(ValueError):
        cas.mask_rle_sized(s.bits)


OTHER = ("classes", "pass1_logits", "masks", "edges", "logits", "pred", "iou", "mask_bits", "area", "box", "inter", "n_comp", "comps", "n_kept",
         "kept_bits", "kept_area", "kept_box", "n_holes", "holes", "n_filled", "filled_bits", "filled_area", "band_bits", "band_area",
         "band_inter", "edge_bits", "edge_area", "edge_band", "edge_inter")
SIZES = [(213, 320), (480, 641)]
CLASSES = [[0, 1, 2], [2, 1, 0]]                                                  # K = 3: a chunk of 4 crosses the image boundary


def check_call(call, sizes, K: int, masks: str):
    """`call(**kw)` runs one entry point with masks=`masks`: with sizes= and rle="sized" the sized planes are the oracle's on the call's
    own `masks` (where it returns them) under the rule, `rle` is the definition on the call's own sized bits, exactly, and every
    other field keeps the bits of the call without them.  -> the result."""
    plain = call(masks=masks)
    assert plain.sized is None and plain.rle is None
    plain = {f: getattr(plain, f).clone() for f in OTHER if getattr(plain, f) is not None}
    h = call(masks=masks, sizes=sizes, rle="sized")
    torch.cuda.synchronize()
    for f in OTHER:
        assert (getattr(h, f) is None) == (f not in plain), f
    for f, t in plain.items():                                                    # bit for bit, floats included
        assert torch.equal(getattr(h, f).contiguous().view(torch.uint8), t.contiguous().view(torch.uint8)), f
    s = h.sized
    s.check()
    assert s.sizes == [sz for sz in sizes for _ in range(K)] and s.level == 128 and s.status.numel() == -(-len(sizes) * K // 4)
    got = [s.to_numpy(p) for p in range(len(s.sizes))]
    assert s.area.cpu().tolist() == [int(m.sum()) for m in got]
    assert [SO.stats(m)[1] for m in got] == s.box.cpu().tolist()
    if h.masks is not None:
        lg = h.masks.reshape(-1, *h.masks.shape[-2:]).cpu().numpy()
        for p, (hh, ww) in enumerate(s.sizes):
            SO.compare(s.plane(p).cpu().numpy(), s.area[p].item(), s.box[p].tolist(), lg[p], hh, ww, 128)
    assert max(int(m.sum()) for m in got) > 0 and min(float(m.mean()) for m in got) < 1            # not only empty and full planes
    assert_rle_is_oracle(h.rle, got)
    assert h.rle.sizes == s.sizes
    return h


def test_infer_classes_sized(tiny, cas, monkeypatch):
    _, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    classes = torch.tensor(CLASSES)
    both = check_call(lambda **kw: cas.infer_classes(inp, ci, cm, classes=classes, **kw), SIZES, 3, "both")
    bits = check_call(lambda **kw: cas.infer_classes(inp, ci, cm, classes=classes, **kw), SIZES, 3, "bits")
    assert bits.masks is None and torch.equal(bits.sized.bits, both.sized.bits) and torch.equal(bits.sized.area, both.sized.area)
    assert torch.equal(bits.rle.counts, both.rle.counts)
    level1 = cas.infer_classes(inp, ci, cm, classes=classes, masks="bits", sizes=SIZES, sized_level=1)
    assert level1.rle is None and level1.sized.level == 1 and int(level1.sized.area.sum()) > int(bits.sized.area.sum())


def test_decode_sized(tiny, cas, monkeypatch):
    _, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    enc = cas.encode(inp, ci, cm)
    sizes = [SIZES[1], SIZES[0], SIZES[1]]                                        # one per decoded row
    both = check_call(lambda **kw: cas.decode(enc, topk=3, images=[1, 0, 1], **kw), sizes, 3, "both")
    bits = check_call(lambda **kw: cas.decode(enc, topk=3, images=[1, 0, 1], **kw), sizes, 3, "bits")
    assert torch.equal(bits.sized.bits, both.sized.bits)
    lo, hi = both.sized.byte_range(0)[0], both.sized.byte_range(3)[0]
    assert torch.equal(both.sized.bits[lo:hi], both.sized.bits[both.sized.byte_range(6)[0]:])      # rows 0 and 2: the same image, the same size


def test_bad_sized_requests_raise_and_launch_nothing(tiny, cas):
    from camouflaged_vlm_amd import hip
    _, _, _, (inp, ci, cm), _ = tiny
    enc = cas.encode(inp, ci, cm)
    torch.cuda.synchronize()
    calls = []
    names = ("gemm", "layernorm", "topk_select", "patchify", "split_f32", "expand_blocks", "bilinear", "mask_pack", "mask_pack_sized",
             "mask_rle_count", "mask_rle_emit", "mask_rle_count_w", "mask_rle_emit_w", "mask_overlap")
    saved = {n: getattr(hip, n) for n in names}
    for n in saved:
        setattr(hip, n, lambda *a, _n=n, **k: calls.append(_n))
    try:
        for kw in (dict(masks="bits", sizes=SIZES[:1]), dict(masks="bits", sizes=SIZES + SIZES[:1]), dict(masks="bits", sizes=[(213, 320), (480.0, 641)]),
                   dict(masks="bits", sizes=[(213, 320), (True, 641)]), dict(masks="bits", sizes=[(213, 320), (0, 641)]),
                   dict(masks="bits", sizes=[(213, 320), (480, 16385)]), dict(masks="bits", sizes=SIZES, sized_level=0),
                   dict(masks="bits", sizes=SIZES, sized_level=256), dict(masks="bits", sizes=SIZES, sized_level=1.5),
                   dict(masks="logits", sizes=SIZES), dict(sizes=SIZES), dict(masks="bits", rle="sized"), dict(masks="both", rle="sized")):
            with pytest.raises(ValueError):
                cas.infer_classes(inp, ci, cm, topk=2, **kw)
            with pytest.raises(ValueError):
                cas.decode(enc, topk=2, **kw)
    finally:
        for n, f in saved.items():
            setattr(hip, n, f)
    assert calls == []


def test_sized_memory_is_the_results_and_the_rle_workspace(tiny, cas, monkeypatch):
    """After one call per mode has sized the grow-only workspaces, sizes= peaks above the same call without it by no more than the new
    result tensors and the uploaded table -- the pack has no workspace --, and rle="sized" adds its results and cumsum's temporaries;
    the workspace "cls_rle" is no larger than RLE_WS_CAP."""
    from camouflaged_vlm_amd import engine
    _, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    modes = {"plain": dict(masks="bits"), "sized": dict(masks="bits", sizes=SIZES), "rle": dict(masks="bits", sizes=SIZES, rle="sized")}
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
        s = h.sized
        results[name] = 0 if s is None else block([s.bits, s.offsets, s.area, s.box, s.status])
        if h.rle is not None:
            results[name] += block([h.rle.counts, h.rle.offsets, h.rle.n_runs, h.rle.status])
        del h, s
    print(f"peak over the starting level: {peak}; new results {results}")
    assert 0 < peak["sized"] - peak["plain"] <= results["sized"] + 2 * 512                         # + the dims table
    assert 0 < peak["rle"] - peak["sized"] <= results["rle"] - results["sized"] + 4 * 512           # + the runs' status words, cumsum


# ---- drop-in -------------------------------------------------------------------------------------------------------------------------------
def test_dropin_passes_sizes_through(tiny, gold, golden_dir):
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
        check_call(lambda **kw: model.infer_classes(inp, ci, cm, topk=3, **kw), SIZES, 3, "both")
        enc = model.encode_images(inp, ci, cm)
        check_call(lambda **kw: model.decode_classes(enc, topk=3, **kw), SIZES, 3, "bits")
        m = model.infer_test(inp, ci, cm)
        s = model.pack_masks_sized(m, SIZES)
        lg = m[:, 0].cpu().numpy()
        masks = []
        for p, (h, w) in enumerate(SIZES):
            SO.compare(s.plane(p).cpu().numpy(), s.area[p].item(), s.box[p].tolist(), lg[p], h, w, 128)
            masks.append(s.to_numpy(p))
        assert_rle_is_oracle(model.mask_rle_sized(s), masks)
