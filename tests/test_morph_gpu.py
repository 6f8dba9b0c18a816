"""Morphology of packed masks: cvlm_mask_morph against the oracle (tests/morph_oracle.py) and against
cvlm_debug_mask_morph_host, exactly -- every output is a bit or an integer -- and into sentinel-filled outputs: the operator cases, shapes
around the kernel's tile, many planes, the reference's own planes (tests/golden/demo_classes_digest.npz), the element-load path, offsets
past 2^31; then band= of Cascade.infer_classes / decode / the drop-in against the oracle on the call's own mask_bits and against the call
without it, alone and together with components= and holes=, and the utility Cascade.mask_morph."""
import os
import sys

import numpy as np
import pytest
import torch

import compact_oracle as XO
import components_oracle as CC
import holes_oracle as HO
import morph_oracle as MO
from test_classes_gpu import build_tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAIRS = ("dil", "ero", "band")
TILE_ROWS, TILE_WORDS = 128, 16                                                   # the kernel's tile (csrc/morph.hip: MO_TH, MO_TW)
BAND = ("band_bits", "band_area", "band_inter")


def sentinels(b: torch.Tensor, pairs) -> dict:
    out = {}
    for name in pairs:
        out[name + "_bits"] = torch.full_like(b, 0xA5)
        out[name + "_area"] = torch.full((b.shape[0],), -7, dtype=torch.int32, device=b.device)
    return out


def run_morph(bits, H: int, W: int, r: int, pairs=PAIRS, host: bool = True) -> dict:
    """hip.mask_morph on host or device bits (P, H * W / 8) into sentinel-filled outputs -> the oracle's dict of numpy arrays; with
    `host` the same call through cvlm_debug_mask_morph_host must give the same."""
    from camouflaged_vlm_amd import hip
    b = (torch.from_numpy(np.ascontiguousarray(bits)) if isinstance(bits, np.ndarray) else bits).to(DEV)
    out = sentinels(b, pairs)
    hip.mask_morph(b, H, W, r, **out)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    if host:
        cpu = b.cpu()
        ref = sentinels(cpu, pairs)
        hip.mask_morph_host(cpu, H, W, r, **ref)
        assert_equal(got, {k: v.numpy() for k, v in ref.items()}, "the host entry")
    return got


def assert_equal(got: dict, want: dict, what) -> None:
    assert set(got) <= set(want), what
    for k, v in got.items():
        assert v.dtype == want[k].dtype and np.array_equal(v, want[k]), (what, k)


def blobs(rng, P: int, H: int, W: int) -> np.ndarray:
    """Planes of a few solid rectangles XORed together plus sparse specks: something is left of them at r = 16 whenever they are large
    enough, and the specks and the rectangles' corners exercise every small radius."""
    planes = rng.random((P, H, W)) < 0.002
    for p in range(P):
        for _ in range(4):
            y0, x0 = rng.integers(0, H), rng.integers(0, W)
            planes[p, y0:y0 + rng.integers(1, max(2, H // 2)), x0:x0 + rng.integers(1, max(2, W // 2))] ^= True
    return planes


# ---- the entry -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MO.operator_cases()))
def test_operator_cases_equal_the_oracle(name):
    planes, radii = MO.operator_cases()[name]
    P, H, W = planes.shape
    bits = MO.pack(planes)
    dev_bits = torch.from_numpy(bits).to(DEV)
    for r in radii:
        assert_equal(run_morph(dev_bits, H, W, r), MO.morph(bits, H, W, r), (name, r))
    r = radii[-1]
    full = run_morph(dev_bits, H, W, r)
    for pairs in (("dil",), ("ero",), ("band",), ("dil", "band"), ("ero", "band"), ("dil", "ero")):   # every subset: the same bits
        assert_equal(run_morph(dev_bits, H, W, r, pairs), full, (name, r, pairs))


@pytest.mark.parametrize("H,wpr", [(TILE_ROWS - 1, TILE_WORDS - 1), (TILE_ROWS + 1, TILE_WORDS + 1), (2 * TILE_ROWS + 1, 2 * TILE_WORDS - 1),
                                   (2 * TILE_ROWS - 1, 2 * TILE_WORDS + 1), (TILE_ROWS + 1, 2 * TILE_WORDS)])
def test_shapes_around_the_tile(H, wpr):
    """H and W / 32 one less and one more than a multiple of the tile: ragged tiles at the right and at the bottom, halo rows that
    belong to the next tile, and (W / 32 = 32) the same with 16-byte loads."""
    W = 32 * wpr
    rng = np.random.default_rng(H * 100 + wpr)
    planes = np.concatenate([blobs(rng, 2, H, W), rng.random((1, H, W)) < 0.5])
    planes[1, TILE_ROWS - 2:min(H, TILE_ROWS + 1)] = True                         # set rows across the seam of two row tiles
    planes[:2, 20:70, 40:140] = True                                              # a solid block: something is left of it at r = 16
    bits = MO.pack(planes)
    for r in (1, 16):
        want = MO.morph(bits, H, W, r)
        assert_equal(run_morph(bits, H, W, r), want, (H, wpr, r))
        if r == 16:
            assert (want["ero_area"][:2] > 0).all() and (want["band_area"][:2] < H * W).all()      # not degenerate at the largest radius


@pytest.mark.parametrize("H,W", [(200, 32), (8, 1536)])
def test_one_column_of_tiles_and_one_row_of_tiles(H, W):
    rng = np.random.default_rng(H)
    planes = np.concatenate([blobs(rng, 2, H, W), rng.random((1, H, W)) < 0.9])
    bits = MO.pack(planes)
    for r in (1, 2, 16):
        assert_equal(run_morph(bits, H, W, r), MO.morph(bits, H, W, r), (H, W, r))


@pytest.mark.parametrize("P,H,W", [(1000, 8, 32), (130, 32, 64)])
def test_many_planes(P, H, W):
    rng = np.random.default_rng(P)
    planes = rng.random((P, H, W)) < rng.uniform(0.02, 0.98, (P, 1, 1))
    planes[17], planes[P - 1] = False, True
    bits = MO.pack(planes)
    for r in (1, 3):
        want = MO.morph(bits, H, W, r)
        assert (want["band_area"] > 0).sum() > P // 2
        assert_equal(run_morph(bits, H, W, r), want, (P, r))


@pytest.fixture(scope="module")
def ref_bits(golden_dir):
    with np.load(os.path.join(golden_dir, "demo_classes_digest.npz")) as z:
        bits = z["mask_bits"]
    return np.ascontiguousarray(bits.reshape(-1, bits.shape[-1]))


@pytest.mark.parametrize("r", [1, 2])
def test_reference_planes_equal_the_oracle_and_repeat(ref_bits, r):
    from camouflaged_vlm_amd import spec
    S = spec.DEMO_SAM.inp_size
    want = MO.morph(ref_bits, S, S, r)
    assert (want["ero_area"] > 0).all() and (want["band_area"] < S * S).all()     # not degenerate at these radii
    dev_bits = torch.from_numpy(ref_bits).to(DEV)
    got = run_morph(dev_bits, S, S, r)
    assert_equal(got, want, r)
    print(f"reference planes, r = {r}: " + ", ".join(f"{k} {v.tolist()}" for k, v in got.items() if k.endswith("area")))
    assert_equal(run_morph(dev_bits, S, S, r, host=False), got, "second run")
    for p in range(6):                                                            # plane by plane
        assert_equal(run_morph(dev_bits[p:p + 1], S, S, r, host=False), {k: v[p:p + 1] for k, v in got.items()}, ("plane", p))


def test_bits_at_an_odd_four_byte_offset_take_the_element_loads():
    """W / 32 = 32 from a 16-byte aligned pointer takes 16-byte loads; the same planes 4 bytes further on must give the same."""
    from camouflaged_vlm_amd import hip
    rng = np.random.default_rng(4)
    P, H, W = 2, 150, 1024
    bits = MO.pack(blobs(rng, P, H, W))
    buf = torch.zeros(bits.size + 16, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    for r in (2, 16):
        want = MO.morph(bits, H, W, r)
        for off in (0, 4):
            b = buf[off:off + bits.size].view(P, -1)
            b.copy_(torch.from_numpy(bits))
            assert b.data_ptr() % 16 == off
            out = sentinels(b, PAIRS)
            hip.mask_morph(b, H, W, r, **out)
            torch.cuda.synchronize()
            assert_equal({k: v.cpu().numpy() for k, v in out.items()}, want, (r, off))


def test_offsets_past_two_to_the_31():
    """16 400 planes of 1024 x 1024, all zero but the last, band only: the last plane starts 2^31 + 2 MiB into the bits."""
    from camouflaged_vlm_amd import hip
    P, S, r = 16400, 1024, 2
    try:
        bits = torch.zeros(P, S * S // 8, dtype=torch.uint8, device=DEV)
        band = torch.full_like(bits, 0xA5)
    except torch.cuda.OutOfMemoryError:
        pytest.skip("4.3 GiB of device memory for the 16 400 planes and their bands could not be allocated")
    last = MO.pack(blobs(np.random.default_rng(31), 1, S, S))
    bits[P - 1].copy_(torch.from_numpy(last[0]))
    area = torch.full((P,), -7, dtype=torch.int32, device=DEV)
    hip.mask_morph(bits, S, S, r, band_bits=band, band_area=area)
    torch.cuda.synchronize()
    want = MO.morph(last, S, S, r)
    assert 0 < want["band_area"][0] < S * S
    assert np.array_equal(band[P - 1].cpu().numpy(), want["band_bits"][0]) and int(area[P - 1]) == want["band_area"][0]
    assert not area[:P - 1].any() and not band[:P - 1].any()


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


REGIONS = ("n_comp", "comps", "n_kept", "kept_bits", "kept_area", "kept_box")
HOLES = ("n_holes", "holes", "n_filled", "filled_bits", "filled_area")
OTHER = ("classes", "pass1_logits", "masks", "edges", "logits", "pred", "mask_bits", "area", "box", "inter") + REGIONS + HOLES
RADIUS = 2                                                                        # the reference's; check_call asserts it is not degenerate
CLASSES = [[0, 1, 2, 3, 4], [4, 3, 2, 1, 0]]                                      # 10 prompts in passes of 4, 4 and 2


def assert_band_is_oracle(h, S: int, r: int, inter: bool):
    """The new fields of a result = the oracle on the result's own mask_bits, and compact_oracle's intersections of band_bits."""
    n, K, nb = h.mask_bits.shape
    want = MO.morph(h.mask_bits.cpu().numpy().reshape(n * K, nb), S, S, r)
    assert tuple(h.band_bits.shape) == (n, K, nb) and h.band_bits.dtype == torch.uint8
    assert tuple(h.band_area.shape) == (n, K) and h.band_area.dtype == torch.int32
    assert np.array_equal(h.band_bits.cpu().numpy().reshape(n * K, nb), want["band_bits"])
    assert np.array_equal(h.band_area.cpu().numpy().ravel(), want["band_area"])
    if inter:
        assert tuple(h.band_inter.shape) == (n, K, K) and h.band_inter.dtype == torch.int32
        assert np.array_equal(h.band_inter.cpu().numpy(), XO.inter(h.band_bits.cpu().numpy()))
        assert torch.equal(torch.diagonal(h.band_inter, dim1=1, dim2=2), h.band_area)
    else:
        assert h.band_inter is None
    return want


def check_call(call, S: int, **more):
    """`call(**kw)` runs one entry point: with band=RADIUS the new fields are the oracle's and every other field keeps the bits of the
    call without it."""
    plain = call(**more)
    assert all(getattr(plain, f) is None for f in BAND)
    plain = {f: getattr(plain, f).clone() for f in OTHER if getattr(plain, f) is not None}
    h = call(band=RADIUS, **more)
    torch.cuda.synchronize()
    for f in OTHER:
        assert (getattr(h, f) is None) == (f not in plain), f
    for f, t in plain.items():                                                    # bit for bit, floats included
        assert torch.equal(getattr(h, f).contiguous().view(torch.uint8), t.contiguous().view(torch.uint8)), f
    want = assert_band_is_oracle(h, S, RADIUS, h.inter is not None)               # band_inter exactly when overlaps=True
    print("band_area", want["band_area"].tolist(), "area", h.area.cpu().ravel().tolist())
    live = h.area.cpu().numpy().ravel() > 0
    assert live.any() and (want["band_area"][live] > 0).all() and (want["band_area"] < S * S).all()   # neither empty nor the whole plane
    return h


@pytest.mark.parametrize("masks", ["bits", "both"])
def test_infer_classes_band(tiny, cas, monkeypatch, masks):
    g, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    classes = torch.tensor(CLASSES)
    check_call(lambda **kw: cas.infer_classes(inp, ci, cm, classes=classes, masks=masks, overlaps=True, **kw), g.inp_size)
    h = cas.infer_classes(inp, ci, cm, classes=classes, masks=masks, band=1)      # without overlaps: no band_inter, another radius
    torch.cuda.synchronize()
    assert h.inter is None
    assert_band_is_oracle(h, g.inp_size, 1, False)


def test_decode_band(tiny, cas, monkeypatch):
    g, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    enc = cas.encode(inp, ci, cm)
    h = check_call(lambda **kw: cas.decode(enc, topk=5, images=[1, 0, 1], masks="bits", overlaps=True, **kw), g.inp_size)
    for f in BAND:                                                                # images 1, 0, 1: rows 0 and 2 are the same hypotheses
        assert torch.equal(getattr(h, f)[0], getattr(h, f)[2]), f


def test_band_with_components_and_holes(tiny, cas, monkeypatch):
    g, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    classes = torch.tensor(CLASSES)
    more = dict(components=4, min_area=16, holes=4, fill_holes=16, overlaps=True)
    h = check_call(lambda **kw: cas.infer_classes(inp, ci, cm, classes=classes, masks="bits", **kw), g.inp_size, **more)
    S = g.inp_size
    flat = h.mask_bits.cpu().numpy().reshape(-1, h.mask_bits.shape[-1])
    want = CC.components(flat, S, S, 8, 4, 16)
    for f in REGIONS:                                                             # all of them stay functions of mask_bits
        assert np.array_equal(getattr(h, f).cpu().numpy().reshape(want[f].shape), want[f]), f
    want = HO.holes(flat, S, S, 8, 4, 16)
    for f in HOLES:
        assert np.array_equal(getattr(h, f).cpu().numpy().reshape(want[f].shape), want[f]), f
    assert np.array_equal(h.inter.cpu().numpy(), XO.inter(h.mask_bits.cpu().numpy()))


def test_empty_hypothesis_has_an_empty_band(cas):
    """Zero bits -- what a hypothesis of class -1 packs to -- give three empty planes."""
    S = cas.g.inp_size
    r = cas.mask_morph(torch.zeros(2, S * S // 8, dtype=torch.uint8, device=DEV), S, S, radius=16, dilate=True, erode=True)
    torch.cuda.synchronize()
    assert not any(t.any() for t in (r.dil_bits, r.dil_area, r.ero_bits, r.ero_area, r.band_bits, r.band_area))


def test_mask_morph_utility(tiny, cas):
    g, _, _, (inp, ci, cm), _ = tiny
    S = g.inp_size
    bits, area, box = cas.pack_masks(cas.infer_test(inp, ci, cm).clone())
    host = bits.cpu().numpy()
    for r in (1, 2, 16):
        want = MO.morph(host, S, S, r)
        got = cas.mask_morph(bits, S, S, radius=r, dilate=True, erode=True)
        torch.cuda.synchronize()
        for f in want:
            assert np.array_equal(getattr(got, f).cpu().numpy(), want[f]), (r, f)
    got = cas.mask_morph(bits, S, S)                                              # the default: the reference's band alone
    torch.cuda.synchronize()
    want = MO.morph(host, S, S, 2)
    assert got.dil_bits is None and got.dil_area is None and got.ero_bits is None and got.ero_area is None
    assert np.array_equal(got.band_bits.cpu().numpy(), want["band_bits"]) and np.array_equal(got.band_area.cpu().numpy(), want["band_area"])
    odd = torch.zeros(bits.numel() + 2, dtype=torch.uint8, device=DEV)[2:].view_as(bits)           # off a 4-byte boundary: cloned
    odd.copy_(bits)
    got = cas.mask_morph(odd, S, S, dilate=True, band=False)
    torch.cuda.synchronize()
    assert got.band_bits is None and np.array_equal(got.dil_bits.cpu().numpy(), want["dil_bits"])
    # closing then SAM's chain, through the utilities
    closed = cas.mask_morph(got.dil_bits, S, S, erode=True, band=False).ero_bits
    k = cas.mask_components(cas.mask_holes(closed, S, S, fill_holes=16).filled_bits, S, S, components=2, min_area=16)
    torch.cuda.synchronize()
    step = MO.morph(want["dil_bits"], S, S, 2)["ero_bits"]
    assert np.array_equal(closed.cpu().numpy(), step) and not (host & ~step).any()                  # closing is extensive
    chain = CC.components(HO.holes(step, S, S, 8, 1, 16)["filled_bits"], S, S, 8, 2, 16)
    for f in REGIONS:
        assert np.array_equal(getattr(k, f).cpu().numpy(), chain[f]), f
    for bad in (dict(bits=bits.cpu()), dict(bits=bits.int()), dict(bits=bits[0]), dict(W=S + 32), dict(W=S // 2 + 1), dict(radius=0),
                dict(radius=17), dict(radius=True), dict(radius=2.0), dict(band=False), dict(band=1), dict(dilate=None)):
        kw = dict(dict(bits=bits, H=S, W=S), **bad)
        with pytest.raises(ValueError):
            cas.mask_morph(kw.pop("bits"), kw.pop("H"), kw.pop("W"), **kw)


def test_bad_band_requests_raise_and_launch_nothing(tiny, cas):
    from camouflaged_vlm_amd import hip
    _, _, _, (inp, ci, cm), _ = tiny
    enc = cas.encode(inp, ci, cm)
    torch.cuda.synchronize()
    calls = []
    names = ("gemm", "layernorm", "topk_select", "patchify", "split_f32", "expand_blocks", "bilinear", "mask_pack", "mask_morph", "mask_overlap")
    saved = {n: getattr(hip, n) for n in names}
    for n in saved:
        setattr(hip, n, lambda *a, _n=n, **k: calls.append(_n))
    try:
        for kw in (dict(band=2), dict(masks="logits", band=1), dict(masks="bits", band=0), dict(masks="bits", band=17),
                   dict(masks="bits", band=2.0), dict(masks="both", band=True), dict(masks="bits", band="2")):
            with pytest.raises(ValueError):
                cas.infer_classes(inp, ci, cm, topk=2, **kw)
            with pytest.raises(ValueError):
                cas.decode(enc, topk=2, **kw)
    finally:
        for n, f in saved.items():
            setattr(hip, n, f)
    assert calls == []


def test_band_memory_is_the_results(tiny, cas, monkeypatch):
    """After one call per mode has sized the grow-only workspaces, masks="bits" with band peaks above the same call without it by
    exactly the new result tensors: cvlm_mask_morph has no workspace."""
    g, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    for overlaps in (False, True):
        modes = {"bits": dict(masks="bits", overlaps=overlaps), "band": dict(masks="bits", overlaps=overlaps, band=2)}
        for kw in modes.values():
            cas.infer_classes(inp, ci, cm, topk=5, **kw)
        torch.cuda.synchronize()
        peak, results = {}, 0
        for name, kw in modes.items():
            torch.cuda.reset_peak_memory_stats()
            start = torch.cuda.memory_allocated()
            h = cas.infer_classes(inp, ci, cm, topk=5, **kw)
            torch.cuda.synchronize()
            peak[name] = torch.cuda.max_memory_allocated() - start
            if name == "band":
                new = [getattr(h, f) for f in BAND if getattr(h, f) is not None]
                assert len(new) == (3 if overlaps else 2)
                results = sum(-(-t.numel() * t.element_size() // 512) * 512 for t in new)             # the allocator's 512-byte blocks
            del h
        print(f"overlaps={overlaps}: peak over the starting level: bits {peak['bits']} B, with band {peak['band']} B; new results {results} B")
        assert peak["band"] - peak["bits"] == results


# ---- drop-in -------------------------------------------------------------------------------------------------------------------------------
def test_dropin_passes_band_through(tiny, gold, golden_dir):
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
    S = g.inp_size
    with torch.no_grad():
        plain = model.infer_classes(inp, ci, cm, topk=3, masks="bits", overlaps=True)
        got = model.infer_classes(inp, ci, cm, topk=3, masks="bits", overlaps=True, band=RADIUS)
        dec = model.decode_classes(model.encode_images(inp, ci, cm), topk=3, masks="bits", overlaps=True, band=RADIUS)
        torch.cuda.synchronize()
        assert_band_is_oracle(got, S, RADIUS, True)
        assert_band_is_oracle(dec, S, RADIUS, True)
        for f in ("classes", "pass1_logits", "logits", "pred", "mask_bits", "area", "box", "inter"):
            assert torch.equal(getattr(got, f), getattr(plain, f)), f
        bits, _, _ = model.pack_masks(model.infer_test(inp, ci, cm))
        r = model.mask_morph(bits, S, S, radius=3, dilate=True, erode=True)
        torch.cuda.synchronize()
        want = MO.morph(bits.cpu().numpy(), S, S, 3)
        assert all(np.array_equal(getattr(r, f).cpu().numpy(), want[f]) for f in want)
