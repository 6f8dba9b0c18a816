"""Connected components of packed masks: cvlm_mask_components against the scipy oracle (tests/components_oracle.py),
exactly -- every output is an integer -- and into sentinel-filled outputs: the operator cases, the rounds of a small workspace, the
reference's own planes (tests/golden/demo_classes_digest.npz), min_area = 1 against cvlm_mask_pack; then components= / min_area= of
Cascade.infer_classes / decode / the drop-in against the oracle on the call's own mask_bits and against the call without them, and
the demo geometry against the reference's bits within the bound set arithmetic gives."""
import os
import sys

import numpy as np
import pytest
import torch

import compact_oracle as XO
import components_oracle as CC
from test_classes_gpu import build_tiny, demo_engines, demo_inputs, demo_sd, dgold  # noqa: F401  (fixtures of the demo geometry)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REGIONS = ("n_comp", "comps", "n_kept", "kept_bits", "kept_area", "kept_box")


def run_components(bits, H: int, W: int, conn: int, M: int, min_area: int, ws_bytes: int = None) -> dict:
    """hip.mask_components on host or device bits (P, H * W / 8) into sentinel-filled outputs -> the oracle's dict of numpy arrays."""
    from camouflaged_vlm_amd import hip
    b = (torch.from_numpy(np.ascontiguousarray(bits)) if isinstance(bits, np.ndarray) else bits).to(DEV)
    P = b.shape[0]
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=DEV)
    out = dict(n_comp=i32(P))
    if M:
        out["comps"] = i32(P, M, 6)
    if min_area:
        out.update(n_kept=i32(P), kept_bits=torch.full_like(b, 0xA5), kept_area=i32(P), kept_box=i32(P, 4))
    ws = torch.empty(hip.mask_components_workspace_bytes(P, H, W) if ws_bytes is None else ws_bytes, dtype=torch.uint8, device=DEV)
    hip.mask_components(b, H, W, conn, min_area, ws, **out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_equal(got: dict, want: dict, what) -> None:
    assert set(got) <= set(want), what
    for k, v in got.items():
        assert v.dtype == want[k].dtype and np.array_equal(v, want[k]), (what, k)


# ---- the entry -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CC.operator_cases()))
def test_operator_cases_equal_the_oracle(name):
    planes = CC.operator_cases()[name]
    P, H, W = planes.shape
    bits = CC.pack(planes)
    dev_bits = torch.from_numpy(bits).to(DEV)
    above = int(XO.stats(planes)[0].max()) + 1                                    # above any region's area: nothing is kept
    for conn in (4, 8):
        for M in (1, 5):
            for min_area in (0, 1, 3, above):
                assert_equal(run_components(dev_bits, H, W, conn, M, min_area), CC.components(bits, H, W, conn, M, min_area),
                             (name, conn, M, min_area))
    got = run_components(dev_bits, H, W, 8, 0, 0)                                 # the count alone
    assert list(got) == ["n_comp"] and np.array_equal(got["n_comp"], CC.components(bits, H, W, 8, 1, 0)["n_comp"])


def test_rounds_of_a_small_workspace():
    """130 planes of 32 x 64 with room for exactly 7: 19 rounds, the last one of 4 planes."""
    from camouflaged_vlm_amd import hip
    rng = np.random.default_rng(130)
    P, H, W = 130, 32, 64
    planes = rng.random((P, H, W)) < rng.uniform(0.05, 0.7, (P, 1, 1))
    planes[17], planes[129] = False, True
    bits = CC.pack(planes)
    ws_bytes = 7 * hip.mask_components_workspace_bytes(1, H, W)
    for conn in (4, 8):
        for M, min_area in ((1, 0), (5, 3)):
            assert_equal(run_components(bits, H, W, conn, M, min_area, ws_bytes), CC.components(bits, H, W, conn, M, min_area), (conn, M))
    assert_equal(run_components(bits, H, W, 8, 5, 3, ws_bytes + 100), CC.components(bits, H, W, 8, 5, 3), "a fraction of a plane over")


def test_min_area_one_is_mask_pack():
    from camouflaged_vlm_amd import hip
    rng = np.random.default_rng(1)
    P, H, W = 3, 64, 96
    logits = torch.from_numpy((rng.random((P, H, W)) - np.array([0.7, 0.5, 0.407]).reshape(3, 1, 1)).astype(np.float32)).to(DEV)
    bits = torch.empty(P, H * W // 8, dtype=torch.uint8, device=DEV)
    area = torch.empty(P, dtype=torch.int32, device=DEV)
    box = torch.empty(P, 4, dtype=torch.int32, device=DEV)
    hip.mask_pack(logits, bits, area, box)
    for conn in (4, 8):
        got = run_components(bits, H, W, conn, 1, 1)
        assert np.array_equal(got["kept_bits"], bits.cpu().numpy()) and np.array_equal(got["kept_area"], area.cpu().numpy())
        assert np.array_equal(got["kept_box"], box.cpu().numpy()) and np.array_equal(got["n_kept"], got["n_comp"])


@pytest.fixture(scope="module")
def ref_bits(dgold):
    bits = dgold["mask_bits"]
    return np.ascontiguousarray(bits.reshape(-1, bits.shape[-1]))


@pytest.mark.parametrize("conn", [4, 8])
def test_reference_planes_equal_the_oracle_and_repeat(ref_bits, conn):
    from camouflaged_vlm_amd import spec
    S = spec.DEMO_SAM.inp_size
    dev_bits = torch.from_numpy(ref_bits).to(DEV)
    got = run_components(dev_bits, S, S, conn, 5, 64)
    assert_equal(got, CC.components(ref_bits, S, S, conn, 5, 64), conn)
    print(f"reference planes, connectivity {conn}: n_comp {got['n_comp'].tolist()} kept at 64 {got['n_kept'].tolist()}")
    assert_equal(run_components(dev_bits, S, S, conn, 5, 64), got, "second run")
    one = run_components(dev_bits, S, S, conn, 5, 64, 14 * S * S)                  # plane by plane: the one-plane minimum
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


OTHER = ("classes", "pass1_logits", "logits", "pred", "mask_bits", "area", "box")


def assert_regions_are_oracle(h, S: int, conn: int, M: int, min_area: int):
    """The six new fields of a result = the oracle on the result's own mask_bits."""
    n, K, nb = h.mask_bits.shape
    want = CC.components(h.mask_bits.cpu().numpy().reshape(n * K, nb), S, S, conn, M, min_area)
    shapes = dict(n_comp=(n, K), comps=(n, K, M, 6), n_kept=(n, K), kept_bits=(n, K, nb), kept_area=(n, K), kept_box=(n, K, 4))
    for f in REGIONS:
        t = getattr(h, f)
        assert tuple(t.shape) == shapes[f] and t.dtype == (torch.uint8 if f == "kept_bits" else torch.int32), f
        assert np.array_equal(t.cpu().numpy().reshape(want[f].shape), want[f]), f
    return want


def check_call(call, S: int):
    """`call(**kw)` runs one entry point with masks="bits" plus kw: with components=4, min_area=16 the new fields are the oracle's
    and every other field keeps the bits of the call without them."""
    plain = call()
    assert all(getattr(plain, f) is None for f in REGIONS)
    plain = {f: getattr(plain, f).clone() for f in OTHER if getattr(plain, f) is not None}
    h = call(components=4, min_area=16)
    torch.cuda.synchronize()
    assert h.masks is None and h.inter is None
    for f, t in plain.items():
        assert torch.equal(getattr(h, f), t), f
    want = assert_regions_are_oracle(h, S, 8, 4, 16)
    print("n_comp", want["n_comp"].tolist(), "n_kept", want["n_kept"].tolist(), "kept area", want["kept_area"].tolist())
    h4 = call(components=0, connectivity=4)
    torch.cuda.synchronize()
    assert h4.comps is None and h4.n_kept is None and h4.kept_bits is None
    n, K, nb = h4.mask_bits.shape
    assert np.array_equal(h4.n_comp.cpu().numpy().ravel(), CC.components(h4.mask_bits.cpu().numpy().reshape(n * K, nb), S, S, 4, 1, 0)["n_comp"])
    return h


def test_infer_classes_components(tiny, cas, gold, monkeypatch):
    g, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)                            # 6 prompts in passes of 4 and 2
    classes = torch.from_numpy(gold["classes"])
    check_call(lambda **kw: cas.infer_classes(inp, ci, cm, classes=classes, masks="bits", **kw), g.inp_size)


def test_decode_components(tiny, cas, monkeypatch):
    g, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    enc = cas.encode(inp, ci, cm)
    h = check_call(lambda **kw: cas.decode(enc, topk=3, images=[1, 0, 1], masks="bits", **kw), g.inp_size)
    for f in REGIONS:                                                             # images 1, 0, 1: rows 0 and 2 are the same hypotheses
        assert torch.equal(getattr(h, f)[0], getattr(h, f)[2]), f
    both = cas.decode(enc, topk=3, masks="both", overlaps=True, components=4, min_area=16, stage2=False)
    torch.cuda.synchronize()
    assert_regions_are_oracle(both, g.inp_size, 8, 4, 16)
    assert np.array_equal(both.inter.cpu().numpy(), XO.inter(both.mask_bits.cpu().numpy()))     # inter stays the overlaps of mask_bits


def test_mask_components_of_pack_masks(tiny, cas):
    g, _, _, (inp, ci, cm), _ = tiny
    S = g.inp_size
    bits, area, box = cas.pack_masks(cas.infer_test(inp, ci, cm).clone())
    r = cas.mask_components(bits, S, S, components=3, min_area=1, connectivity=4)
    torch.cuda.synchronize()
    want = CC.components(bits.cpu().numpy(), S, S, 4, 3, 1)
    for f in REGIONS:
        assert np.array_equal(getattr(r, f).cpu().numpy(), want[f]), f
    assert torch.equal(r.kept_bits, bits) and torch.equal(r.kept_area, area) and torch.equal(r.kept_box, box)
    r = cas.mask_components(bits, S, S)
    torch.cuda.synchronize()
    assert r.n_kept is None and np.array_equal(r.comps.cpu().numpy(), CC.components(bits.cpu().numpy(), S, S, 8, 1, 0)["comps"])
    for bad in (dict(bits=bits.cpu()), dict(bits=bits.int()), dict(bits=bits[0]), dict(W=S + 32), dict(W=S // 2 + 1), dict(components=65),
                dict(min_area=-1), dict(connectivity=6)):
        kw = dict(dict(bits=bits, H=S, W=S, components=1, min_area=0, connectivity=8), **bad)
        with pytest.raises(ValueError):
            cas.mask_components(kw.pop("bits"), kw.pop("H"), kw.pop("W"), **kw)


def test_bad_component_requests_raise_and_launch_nothing(tiny, cas):
    from camouflaged_vlm_amd import hip
    _, _, _, (inp, ci, cm), _ = tiny
    enc = cas.encode(inp, ci, cm)
    torch.cuda.synchronize()
    calls = []
    names = ("gemm", "layernorm", "topk_select", "patchify", "split_f32", "expand_blocks", "bilinear", "mask_pack", "mask_components")
    saved = {n: getattr(hip, n) for n in names}
    for n in saved:
        setattr(hip, n, lambda *a, _n=n, **k: calls.append(_n))
    try:
        for kw in (dict(components=2), dict(min_area=4), dict(masks="logits", components=0), dict(masks="bits", components=65),
                   dict(masks="bits", components=-1), dict(masks="bits", components=2.0), dict(masks="both", min_area=-1),
                   dict(masks="bits", components=1, connectivity=6)):
            with pytest.raises(ValueError):
                cas.infer_classes(inp, ci, cm, topk=2, **kw)
            with pytest.raises(ValueError):
                cas.decode(enc, topk=2, **kw)
    finally:
        for n, f in saved.items():
            setattr(hip, n, f)
    assert calls == []


def test_components_memory_is_the_results_and_the_workspace(tiny, cas, monkeypatch):
    """After one call per mode has sized the grow-only workspaces, masks="bits" with components peaks above the same call without
    them by no more than the new result tensors (the workspace "cls_comp" is below its cap and already there)."""
    from camouflaged_vlm_amd.engine import COMPONENTS_WS_CAP
    g, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    modes = {"bits": dict(masks="bits"), "regions": dict(masks="bits", components=8, min_area=16)}
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
        if name == "regions":
            results = sum(-(-getattr(h, f).numel() * getattr(h, f).element_size() // 512) * 512 for f in REGIONS)   # 512-byte blocks
        del h
    ws = cas.ws._flat[("u8", "cls_comp")].numel()
    print(f"peak over the starting level: bits {peak['bits']} B, with components {peak['regions']} B; new results {results} B; cls_comp {ws} B")
    assert 14 * g.inp_size ** 2 <= ws <= COMPONENTS_WS_CAP <= 256 << 20
    assert peak["regions"] - peak["bits"] <= results


# ---- drop-in -------------------------------------------------------------------------------------------------------------------------------
def test_dropin_passes_components_through(tiny, gold, golden_dir):
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
        got = model.infer_classes(inp, ci, cm, topk=3, masks="bits", components=4, min_area=16)
        dec = model.decode_classes(model.encode_images(inp, ci, cm), topk=3, masks="bits", components=4, min_area=16)
        torch.cuda.synchronize()
        assert_regions_are_oracle(got, S, 8, 4, 16)
        assert_regions_are_oracle(dec, S, 8, 4, 16)
        bits, _, _ = model.pack_masks(model.infer_test(inp, ci, cm))
        r = model.mask_components(bits, S, S, components=2, min_area=4)
        torch.cuda.synchronize()
        want = CC.components(bits.cpu().numpy(), S, S, 8, 2, 4)
        assert all(np.array_equal(getattr(r, f).cpu().numpy(), want[f]) for f in REGIONS)


# ---- demo geometry, mx ---------------------------------------------------------------------------------------------------------------------
def test_demo_components_against_the_oracle_and_the_reference_bits(demo_engines, dgold, demo_inputs):
    """The device equals the oracle on the engine's own bits.  Against the reference's bits: with d the pixels in which a plane
    differs from the reference's, |n_comp - n_ref| <= 3 d -- setting one pixel joins at most four regions into one (-3) or adds one
    (+1), clearing one does the reverse --, a bound of set arithmetic, not a tolerance."""
    cas = demo_engines["mx"]
    inp, ci, cm = demo_inputs
    S = cas.g.inp_size
    h = cas.infer_classes(inp, ci, cm, classes=torch.from_numpy(dgold["classes"]), masks="bits", components=4, min_area=64)
    torch.cuda.synchronize()
    assert_regions_are_oracle(h, S, 8, 4, 64)
    ref = dgold["mask_bits"]
    B, K, nb = ref.shape
    got = h.mask_bits.cpu().numpy()
    d = np.unpackbits(got ^ ref, axis=-1).sum(-1).astype(np.int64)
    n_ref = CC.components(ref.reshape(B * K, nb), S, S, 8, 1, 0)["n_comp"].reshape(B, K)
    n_dev = h.n_comp.cpu().numpy()
    for b in range(B):
        for k in range(K):
            print(f"demo mx image {b} class {int(dgold['classes'][b, k])}: d = {d[b, k]}, n_comp {n_dev[b, k]} / reference {n_ref[b, k]}")
            assert abs(int(n_dev[b, k]) - int(n_ref[b, k])) <= 3 * d[b, k]
