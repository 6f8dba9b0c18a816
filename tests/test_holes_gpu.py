"""Holes of packed masks: cvlm_mask_holes against the scipy oracle (tests/holes_oracle.py), exactly -- every output is
an integer -- and into sentinel-filled outputs: the operator cases, the rounds of a small workspace, the reference's own planes and
their complements (tests/golden/demo_classes_digest.npz), fill_below = 1 against cvlm_mask_pack; then holes= / fill_holes= of
Cascade.infer_classes / decode / the drop-in against the oracle on the call's own mask_bits and against the call without them, alone
and together with components=, and SAM's order -- fill, then despeckle -- through the two utilities."""
import os
import sys

import numpy as np
import pytest
import torch

import compact_oracle as XO
import components_oracle as CC
import holes_oracle as HO
from test_classes_gpu import build_tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HOLES = ("n_holes", "holes", "n_filled", "filled_bits", "filled_area")
REGIONS = ("n_comp", "comps", "n_kept", "kept_bits", "kept_area", "kept_box")


def run_holes(bits, H: int, W: int, conn: int, M: int, fill_below: int, ws_bytes: int = None) -> dict:
    """hip.mask_holes on host or device bits (P, H * W / 8) into sentinel-filled outputs -> the oracle's dict of numpy arrays."""
    from camouflaged_vlm_amd import hip
    b = (torch.from_numpy(np.ascontiguousarray(bits)) if isinstance(bits, np.ndarray) else bits).to(DEV)
    P = b.shape[0]
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=DEV)
    out = dict(n_holes=i32(P))
    if M:
        out["holes"] = i32(P, M, 6)
    if fill_below:
        out.update(n_filled=i32(P), filled_bits=torch.full_like(b, 0xA5), filled_area=i32(P))
    ws = torch.empty(hip.mask_holes_workspace_bytes(P, H, W) if ws_bytes is None else ws_bytes, dtype=torch.uint8, device=DEV)
    hip.mask_holes(b, H, W, conn, fill_below, ws, **out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_equal(got: dict, want: dict, what) -> None:
    assert set(got) <= set(want), what
    for k, v in got.items():
        assert v.dtype == want[k].dtype and np.array_equal(v, want[k]), (what, k)


# ---- the entry -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HO.operator_cases()))
def test_operator_cases_equal_the_oracle(name):
    planes = HO.operator_cases()[name]
    P, H, W = planes.shape
    bits = HO.pack(planes)
    dev_bits = torch.from_numpy(bits).to(DEV)
    for conn in (4, 8):
        above = int(HO.holes(bits, H, W, conn, 1, 0)["holes"][:, 0, 0].max()) + 1     # one above the largest hole: every hole is filled
        for M in (1, 5):
            for fill_below in (0, 1, 3, above):
                assert_equal(run_holes(dev_bits, H, W, conn, M, fill_below), HO.holes(bits, H, W, conn, M, fill_below),
                             (name, conn, M, fill_below))
        assert_equal(run_holes(dev_bits, H, W, conn, 1, H * W), HO.holes(bits, H, W, conn, 1, H * W), (name, conn, "every hole"))
    got = run_holes(dev_bits, H, W, 8, 0, 0)                                      # the count alone
    assert list(got) == ["n_holes"] and np.array_equal(got["n_holes"], HO.holes(bits, H, W, 8, 1, 0)["n_holes"])


def test_rounds_of_a_small_workspace():
    """130 planes of 32 x 64 with room for exactly 7: 19 rounds, the last one of 4 planes."""
    from camouflaged_vlm_amd import hip
    rng = np.random.default_rng(130)
    P, H, W = 130, 32, 64
    planes = rng.random((P, H, W)) < rng.uniform(0.3, 0.95, (P, 1, 1))
    planes[17], planes[129] = False, True
    bits = HO.pack(planes)
    ws_bytes = 7 * hip.mask_holes_workspace_bytes(1, H, W)
    for conn in (4, 8):
        want = HO.holes(bits, H, W, conn, 5, 3)
        assert (want["n_holes"] > 0).sum() > 100 and want["n_filled"].sum() > 0
        assert_equal(run_holes(bits, H, W, conn, 5, 3, ws_bytes), want, (conn, 5))
        assert_equal(run_holes(bits, H, W, conn, 1, 0, ws_bytes), HO.holes(bits, H, W, conn, 1, 0), (conn, 1))
    assert_equal(run_holes(bits, H, W, 8, 5, 3, ws_bytes + 100), HO.holes(bits, H, W, 8, 5, 3), "a fraction of a plane over")


def test_fill_below_one_is_mask_pack():
    from camouflaged_vlm_amd import hip
    rng = np.random.default_rng(1)
    P, H, W = 3, 64, 96
    logits = torch.from_numpy((rng.random((P, H, W)) - np.array([0.5, 0.3, 0.1]).reshape(3, 1, 1)).astype(np.float32)).to(DEV)
    bits = torch.empty(P, H * W // 8, dtype=torch.uint8, device=DEV)
    area = torch.empty(P, dtype=torch.int32, device=DEV)
    box = torch.empty(P, 4, dtype=torch.int32, device=DEV)
    hip.mask_pack(logits, bits, area, box)
    for conn in (4, 8):
        got = run_holes(bits, H, W, conn, 1, 1)
        assert np.array_equal(got["filled_bits"], bits.cpu().numpy()) and np.array_equal(got["filled_area"], area.cpu().numpy())
        assert (got["n_filled"] == 0).all() and (got["n_holes"] > 0).all()


@pytest.fixture(scope="module")
def ref_both(golden_dir):
    """The reference's six planes and their six complements."""
    with np.load(os.path.join(golden_dir, "demo_classes_digest.npz")) as z:
        bits = z["mask_bits"]
    bits = np.ascontiguousarray(bits.reshape(-1, bits.shape[-1]))
    return np.concatenate([bits, ~bits])


@pytest.fixture(scope="module")
def ref_want(ref_both):
    from camouflaged_vlm_amd import spec
    S = spec.DEMO_SAM.inp_size
    return {conn: HO.holes(ref_both, S, S, conn, 5, 64) for conn in (4, 8)}


@pytest.mark.parametrize("conn", [4, 8])
def test_reference_planes_and_complements_equal_the_oracle_and_repeat(ref_both, ref_want, conn):
    from camouflaged_vlm_amd import spec
    S = spec.DEMO_SAM.inp_size
    dev_bits = torch.from_numpy(ref_both).to(DEV)
    got = run_holes(dev_bits, S, S, conn, 5, 64)
    assert_equal(got, ref_want[conn], conn)
    print(f"reference planes and complements, connectivity {conn}: n_holes {got['n_holes'].tolist()} below 64 {got['n_filled'].tolist()}")
    assert_equal(run_holes(dev_bits, S, S, conn, 5, 64), got, "second run")
    one = run_holes(dev_bits, S, S, conn, 5, 64, 14 * S * S)                      # plane by plane: the one-plane minimum
    assert_equal(one, got, "one plane per round")


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


OTHER = ("classes", "pass1_logits", "logits", "pred", "mask_bits", "area", "box", "inter") + REGIONS


def assert_holes_are_oracle(h, S: int, conn: int, M: int, fill_below: int):
    """The five new fields of a result = the oracle on the result's own mask_bits."""
    n, K, nb = h.mask_bits.shape
    want = HO.holes(h.mask_bits.cpu().numpy().reshape(n * K, nb), S, S, conn, M, fill_below)
    shapes = dict(n_holes=(n, K), holes=(n, K, M, 6), n_filled=(n, K), filled_bits=(n, K, nb), filled_area=(n, K))
    for f in HOLES:
        t = getattr(h, f)
        assert tuple(t.shape) == shapes[f] and t.dtype == (torch.uint8 if f == "filled_bits" else torch.int32), f
        assert np.array_equal(t.cpu().numpy().reshape(want[f].shape), want[f]), f
    return want


def check_call(call, S: int, **more):
    """`call(**kw)` runs one entry point with masks="bits" plus kw: with holes=4, fill_holes=16 the new fields are the oracle's and
    every other field -- with `more`, the components' and the overlaps too -- keeps the bits of the call without them."""
    plain = call(**more)
    assert all(getattr(plain, f) is None for f in HOLES)
    plain = {f: getattr(plain, f).clone() for f in OTHER if getattr(plain, f) is not None}
    assert ("kept_bits" in plain) == ("min_area" in more) and ("inter" in plain) == ("overlaps" in more)
    h = call(holes=4, fill_holes=16, **more)
    torch.cuda.synchronize()
    assert h.masks is None
    for f in OTHER:
        assert (getattr(h, f) is None) == (f not in plain), f
    for f, t in plain.items():
        assert torch.equal(getattr(h, f), t), f
    want = assert_holes_are_oracle(h, S, 8, 4, 16)
    print("n_holes", want["n_holes"].tolist(), "n_filled", want["n_filled"].tolist(), "filled area", want["filled_area"].tolist())
    h4 = call(holes=0, connectivity=4, **more)
    torch.cuda.synchronize()
    assert h4.holes is None and h4.n_filled is None and h4.filled_bits is None and h4.filled_area is None
    n, K, nb = h4.mask_bits.shape
    assert np.array_equal(h4.n_holes.cpu().numpy().ravel(), HO.holes(h4.mask_bits.cpu().numpy().reshape(n * K, nb), S, S, 4, 1, 0)["n_holes"])
    return h


WITH_COMPONENTS = dict(components=4, min_area=16, overlaps=True)


@pytest.mark.parametrize("more", [{}, WITH_COMPONENTS], ids=["alone", "with_components"])
def test_infer_classes_holes(tiny, cas, gold, monkeypatch, more):
    g, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)                            # 6 prompts in passes of 4 and 2
    classes = torch.from_numpy(gold["classes"])
    h = check_call(lambda **kw: cas.infer_classes(inp, ci, cm, classes=classes, masks="bits", **kw), g.inp_size, **more)
    if more:
        want = CC.components(h.mask_bits.cpu().numpy().reshape(-1, h.mask_bits.shape[-1]), g.inp_size, g.inp_size, 8, 4, 16)
        for f in REGIONS:                                                         # kept_* stay functions of mask_bits, not of filled_bits
            assert np.array_equal(getattr(h, f).cpu().numpy().reshape(want[f].shape), want[f]), f
        assert np.array_equal(h.inter.cpu().numpy(), XO.inter(h.mask_bits.cpu().numpy()))


@pytest.mark.parametrize("more", [{}, WITH_COMPONENTS], ids=["alone", "with_components"])
def test_decode_holes(tiny, cas, monkeypatch, more):
    g, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    enc = cas.encode(inp, ci, cm)
    h = check_call(lambda **kw: cas.decode(enc, topk=3, images=[1, 0, 1], masks="bits", **kw), g.inp_size, **more)
    for f in HOLES:                                                               # images 1, 0, 1: rows 0 and 2 are the same hypotheses
        assert torch.equal(getattr(h, f)[0], getattr(h, f)[2]), f


def test_empty_hypothesis_has_no_holes(cas):
    """Zero bits -- what a hypothesis of class -1 packs to -- give n_holes 0, filler rows and an empty filled plane."""
    S = cas.g.inp_size
    r = cas.mask_holes(torch.zeros(2, S * S // 8, dtype=torch.uint8, device=DEV), S, S, holes=2, fill_holes=S * S)
    torch.cuda.synchronize()
    assert not r.n_holes.any() and not r.n_filled.any() and not r.filled_bits.any() and not r.filled_area.any()
    assert r.holes.cpu().tolist() == [[list(HO.FILLER)] * 2] * 2


def test_fill_then_despeckle_through_the_utilities(tiny, cas):
    """SAM's order: remove_small_regions(mask, t, "holes"), then (..., "islands")."""
    g, _, _, (inp, ci, cm), _ = tiny
    S = g.inp_size
    bits, area, box = cas.pack_masks(cas.infer_test(inp, ci, cm).clone())
    host = bits.cpu().numpy()
    r = cas.mask_holes(bits, S, S, holes=3, fill_holes=16, connectivity=8)
    torch.cuda.synchronize()
    want = HO.holes(host, S, S, 8, 3, 16)
    for f in HOLES:
        assert np.array_equal(getattr(r, f).cpu().numpy(), want[f]), f
    k = cas.mask_components(r.filled_bits, S, S, components=3, min_area=16)
    torch.cuda.synchronize()
    chain = CC.components(want["filled_bits"], S, S, 8, 3, 16)
    for f in REGIONS:
        assert np.array_equal(getattr(k, f).cpu().numpy(), chain[f]), f
    print("holes", want["n_holes"].tolist(), "filled", want["n_filled"].tolist(), "regions after", chain["n_comp"].tolist(),
          "kept", chain["n_kept"].tolist())
    r = cas.mask_holes(bits, S, S, connectivity=4)
    torch.cuda.synchronize()
    assert r.n_filled is None and np.array_equal(r.holes.cpu().numpy(), HO.holes(host, S, S, 4, 1, 0)["holes"])
    r = cas.mask_holes(bits, S, S, holes=0, fill_holes=1)
    torch.cuda.synchronize()
    assert r.holes is None and torch.equal(r.filled_bits, bits) and torch.equal(r.filled_area, area)
    for bad in (dict(bits=bits.cpu()), dict(bits=bits.int()), dict(bits=bits[0]), dict(W=S + 32), dict(W=S // 2 + 1), dict(holes=65),
                dict(fill_holes=-1), dict(fill_holes=True), dict(connectivity=6)):
        kw = dict(dict(bits=bits, H=S, W=S, holes=1, fill_holes=0, connectivity=8), **bad)
        with pytest.raises(ValueError):
            cas.mask_holes(kw.pop("bits"), kw.pop("H"), kw.pop("W"), **kw)


def test_bad_hole_requests_raise_and_launch_nothing(tiny, cas):
    from camouflaged_vlm_amd import hip
    _, _, _, (inp, ci, cm), _ = tiny
    enc = cas.encode(inp, ci, cm)
    torch.cuda.synchronize()
    calls = []
    names = ("gemm", "layernorm", "topk_select", "patchify", "split_f32", "expand_blocks", "bilinear", "mask_pack", "mask_components",
             "mask_holes")
    saved = {n: getattr(hip, n) for n in names}
    for n in saved:
        setattr(hip, n, lambda *a, _n=n, **k: calls.append(_n))
    try:
        for kw in (dict(holes=2), dict(fill_holes=4), dict(masks="logits", holes=0), dict(masks="bits", holes=65),
                   dict(masks="bits", holes=-1), dict(masks="bits", holes=2.0), dict(masks="both", fill_holes=-1),
                   dict(masks="bits", fill_holes=True), dict(masks="bits", holes=1, connectivity=6)):
            with pytest.raises(ValueError):
                cas.infer_classes(inp, ci, cm, topk=2, **kw)
            with pytest.raises(ValueError):
                cas.decode(enc, topk=2, **kw)
    finally:
        for n, f in saved.items():
            setattr(hip, n, f)
    assert calls == []


def test_holes_memory_is_the_results_and_the_workspace(tiny, cas, monkeypatch):
    """After one call per mode has sized the grow-only workspaces, masks="bits" with holes peaks above the same call without them by no
    more than the new result tensors (the workspace "cls_comp", shared with components=, is below its cap and already there)."""
    from camouflaged_vlm_amd.engine import COMPONENTS_WS_CAP
    g, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    modes = {"bits": dict(masks="bits"), "holes": dict(masks="bits", holes=8, fill_holes=16)}
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
        if name == "holes":
            results = sum(-(-getattr(h, f).numel() * getattr(h, f).element_size() // 512) * 512 for f in HOLES)   # 512-byte blocks
        del h
    ws = cas.ws._flat[("u8", "cls_comp")].numel()
    print(f"peak over the starting level: bits {peak['bits']} B, with holes {peak['holes']} B; new results {results} B; cls_comp {ws} B")
    assert 14 * g.inp_size ** 2 <= ws <= COMPONENTS_WS_CAP <= 256 << 20
    assert peak["holes"] - peak["bits"] <= results


# ---- drop-in -------------------------------------------------------------------------------------------------------------------------------
def test_dropin_passes_holes_through(tiny, gold, golden_dir):
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
        plain = model.infer_classes(inp, ci, cm, topk=3, masks="bits")
        got = model.infer_classes(inp, ci, cm, topk=3, masks="bits", holes=4, fill_holes=16)
        dec = model.decode_classes(model.encode_images(inp, ci, cm), topk=3, masks="bits", holes=4, fill_holes=16)
        torch.cuda.synchronize()
        assert_holes_are_oracle(got, S, 8, 4, 16)
        assert_holes_are_oracle(dec, S, 8, 4, 16)
        for f in ("classes", "pass1_logits", "logits", "pred", "mask_bits", "area", "box"):
            assert torch.equal(getattr(got, f), getattr(plain, f)), f
        bits, _, _ = model.pack_masks(model.infer_test(inp, ci, cm))
        r = model.mask_holes(bits, S, S, holes=2, fill_holes=4)
        torch.cuda.synchronize()
        want = HO.holes(bits.cpu().numpy(), S, S, 8, 2, 4)
        assert all(np.array_equal(getattr(r, f).cpu().numpy(), want[f]) for f in HOLES)
