"""Packed edge maps: cvlm_edge_pack against the oracle (tests/edges_oracle.py) and against cvlm_debug_edge_pack_host,
exactly -- every output is a bit or an integer -- and into sentinel-filled outputs: the operator cases, shapes around the kernel's tile
for both of its instances, many planes, unaligned pointers, offsets past 2^31; then edge_threshold= of Cascade.infer_classes / decode /
the drop-in against the oracle on the call's own low-resolution edge maps and against the call without it, alone and together with
components= and holes=, and the utility Cascade.pack_edges."""
import os
import sys

import numpy as np
import pytest
import torch

import compact_oracle as XO
import components_oracle as CC
import edges_oracle as EO
import holes_oracle as HO
import morph_oracle as MO
from test_classes_gpu import build_tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE_ROWS, TILE_WORDS = 64, 8                                                     # the kernel's tile (csrc/edgepack_logic.h: EP_TH, EP_TW / 32)
f32 = np.float32


def to_dev(a):
    return (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a).to(DEV)


def run_pack(prob, hout: int, wout: int, t: float, with_bits=None, host: bool = True) -> dict:
    """hip.edge_pack on host or device planes (P, hin, win) into sentinel-filled outputs -> the oracle's dict of numpy arrays; with
    `host` the same call through cvlm_debug_edge_pack_host must give the same."""
    from camouflaged_vlm_amd import hip
    p = to_dev(prob)
    P = p.shape[0]

    def outputs(dev):
        out = dict(bits=torch.full((P, hout * wout // 8), 0xA5, dtype=torch.uint8, device=dev),
                   area=torch.full((P,), -7, dtype=torch.int32, device=dev))
        if with_bits is not None:
            out["with_inter"] = torch.full((P,), -7, dtype=torch.int32, device=dev)
        return out
    wb = None if with_bits is None else to_dev(with_bits)
    out = outputs(DEV)
    hip.edge_pack(p, hout, wout, t, out["bits"], out["area"], wb, out.get("with_inter"))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    if host:
        ref = outputs("cpu")
        hip.edge_pack_host(p.cpu(), hout, wout, t, ref["bits"], ref["area"], None if wb is None else wb.cpu(), ref.get("with_inter"))
        assert_equal(got, {k: v.numpy() for k, v in ref.items()}, "the host entry")
    return got


def assert_equal(got: dict, want: dict, what) -> None:
    assert set(got) == set(want), what
    for k, v in got.items():
        assert v.dtype == want[k].dtype and np.array_equal(v, want[k]), (what, k)


def smooth(rng, P: int, h: int, w: int) -> np.ndarray:
    """Planes in [0, 1] that cross every threshold many times: a few random low-frequency waves plus a little noise."""
    yy, xx = np.mgrid[0:h, 0:w].astype(f32)
    out = np.empty((P, h, w), f32)
    for p in range(P):
        a, b, c, d = rng.uniform(0.05, 0.9, 4)
        out[p] = 0.5 + 0.45 * np.sin(a * yy + c) * np.cos(b * xx + d) + rng.uniform(-0.04, 0.04, (h, w))
    return np.clip(out, 0, 1).astype(f32)


# ---- the entry -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EO.operator_cases()))
def test_operator_cases_equal_the_oracle(name):
    prob, ho, wo, thresholds = EO.operator_cases()[name]
    rng = np.random.default_rng(len(name))
    other = EO.pack(rng.random((prob.shape[0], ho, wo)) < 0.5)
    dev_prob = to_dev(prob)
    for t in thresholds:
        want = EO.edge_pack(prob, ho, wo, t, other)
        assert_equal(run_pack(dev_prob, ho, wo, t, other), want, (name, t))
        area_only = run_pack(dev_prob, ho, wo, t)                                  # with_* NULL: the same bits
        assert_equal(area_only, {k: want[k] for k in ("bits", "area")}, (name, t, "area only"))


def test_the_models_scale_on_the_reference_maps(golden_dir):
    """The fixture's own 80^2 maps to 320^2, at t = 0.25 / 0.5 / 0.9; twice and plane by plane with the same bits."""
    with np.load(os.path.join(golden_dir, "tiny_classes.npz")) as z:
        low = np.ascontiguousarray(z["low_edges"].reshape(-1, 80, 80))
    S = 320
    dev_prob = to_dev(low)
    other = EO.pack(np.random.default_rng(1).random((low.shape[0], S, S)) < 0.3)
    for t in (0.25, 0.5, 0.9):
        want = EO.edge_pack(low, S, S, t, other)
        got = run_pack(dev_prob, S, S, t, other)
        assert_equal(got, want, t)
        assert_equal(run_pack(dev_prob, S, S, t, other, host=False), got, "second run")
        for p in range(0, low.shape[0], 3):
            assert_equal(run_pack(dev_prob[p:p + 1], S, S, t, other[p:p + 1], host=False), {k: v[p:p + 1] for k, v in got.items()}, ("plane", p))
    frac = want["area"] / (S * S)
    assert (frac > 0.05).all() and (frac < 0.95).all()                             # t = 0.9: neither empty nor full


@pytest.mark.parametrize("staged", [True, False])
@pytest.mark.parametrize("hout,wpr", [(TILE_ROWS - 1, TILE_WORDS - 1), (TILE_ROWS + 1, TILE_WORDS + 1), (2 * TILE_ROWS + 1, 2 * TILE_WORDS - 1),
                                      (2 * TILE_ROWS - 1, 2 * TILE_WORDS + 1)])
def test_shapes_around_the_tile(hout, wpr, staged):
    """hout and wout / 32 one less and one more than a multiple of the tile: ragged tiles at the right and at the bottom, for the
    instance that stages the footprint (a non-integer scale near 4) and for the one that reads the planes directly (scale 1)."""
    from camouflaged_vlm_amd import hip
    wout = 32 * wpr
    hin, win = (hout // 4 + 1, wout // 4 + 3) if staged else (hout, wout)
    assert hip.edge_pack_staged(hin, win, hout, wout) == staged
    rng = np.random.default_rng(hout * 100 + wpr)
    prob = smooth(rng, 3, hin, win)
    other = EO.pack(rng.random((3, hout, wout)) < 0.5)
    for t in (0.25, 0.9):
        want = EO.edge_pack(prob, hout, wout, t, other)
        assert 0 < want["area"].min() and want["area"].max() < hout * wout
        assert_equal(run_pack(prob, hout, wout, t, other), want, (hout, wpr, staged, t))


@pytest.mark.parametrize("hin,win,hout,wout", [(300, 500, 100, 160), (130, 700, 130, 352), (90, 200, 200, 96)])
def test_scales_that_take_the_direct_instance(hin, win, hout, wout):
    from camouflaged_vlm_amd import hip
    assert not hip.edge_pack_staged(hin, win, hout, wout)
    rng = np.random.default_rng(hin)
    prob = smooth(rng, 2, hin, win)
    other = EO.pack(rng.random((2, hout, wout)) < 0.5)
    for t in (0.25, 0.5, 0.9):
        assert_equal(run_pack(prob, hout, wout, t, other), EO.edge_pack(prob, hout, wout, t, other), (hin, win, t))


def test_pointers_at_an_odd_four_byte_offset():
    """prob and with_bits 4 bytes past a 16-byte boundary against the same planes 16-byte aligned."""
    from camouflaged_vlm_amd import hip
    rng = np.random.default_rng(4)
    for (P, hin, win, hout, wout) in ((2, 64, 64, 256, 256), (2, 150, 256, 150, 256)):
        prob = smooth(rng, P, hin, win)
        other = EO.pack(rng.random((P, hout, wout)) < 0.5)
        want = EO.edge_pack(prob, hout, wout, 0.5, other)
        pbuf = torch.zeros(prob.size + 4, dtype=torch.float32, device=DEV)
        wbuf = torch.zeros(other.size + 16, dtype=torch.uint8, device=DEV)
        assert pbuf.data_ptr() % 16 == 0 and wbuf.data_ptr() % 16 == 0
        for off in (0, 1):
            p = pbuf[off:off + prob.size].view(P, hin, win)
            w = wbuf[4 * off:4 * off + other.size].view(P, -1)
            p.copy_(torch.from_numpy(prob))
            w.copy_(torch.from_numpy(other))
            assert p.data_ptr() % 16 == 4 * off and w.data_ptr() % 16 == 4 * off
            out = dict(bits=torch.full((P, hout * wout // 8), 0xA5, dtype=torch.uint8, device=DEV),
                       area=torch.full((P,), -7, dtype=torch.int32, device=DEV), with_inter=torch.full((P,), -7, dtype=torch.int32, device=DEV))
            hip.edge_pack(p, hout, wout, 0.5, out["bits"], out["area"], w, out["with_inter"])
            torch.cuda.synchronize()
            assert_equal({k: v.cpu().numpy() for k, v in out.items()}, want, (hin, off))


def test_a_thousand_small_planes():
    rng = np.random.default_rng(1000)
    prob = rng.random((1000, 2, 8)).astype(f32)
    prob[17], prob[999] = 0, 1
    other = EO.pack(rng.random((1000, 8, 32)) < 0.5)
    for t in (0.25, 0.9):
        want = EO.edge_pack(prob, 8, 32, t, other)
        assert want["area"][17] == 0 and want["area"][999] == 256 and (want["area"] > 0).sum() > 500
        assert_equal(run_pack(prob, 8, 32, t, other), want, t)


@pytest.mark.parametrize("density", [0.02, 0.5, 0.98])
def test_with_inter_is_the_popcount_of_the_and(density):
    rng = np.random.default_rng(int(density * 100))
    prob = smooth(rng, 4, 96, 96)
    other = EO.pack(rng.random((4, 384, 384)) < density)
    got = run_pack(prob, 384, 384, 0.5, other)
    assert_equal(got, EO.edge_pack(prob, 384, 384, 0.5, other), density)
    assert np.array_equal(got["with_inter"], EO.popcount(got["bits"] & other)) and (got["with_inter"] > 0).all()
    assert (got["with_inter"] < got["area"]).all()


def test_offsets_past_two_to_the_31():
    """16 400 planes of 192^2 -> 1024^2, all zero but the last: the last source plane starts 2^31 + 258 MiB into prob, the last output
    plane 2^31 + 1.9 MiB into bits."""
    from camouflaged_vlm_amd import hip
    P, L, S, t = 16400, 192, 1024, 0.5
    assert (P - 1) * L * L * 4 > 2 ** 31 and (P - 1) * S * S // 8 > 2 ** 31
    try:
        prob = torch.zeros(P, L, L, dtype=torch.float32, device=DEV)
        bits = torch.full((P, S * S // 8), 0xA5, dtype=torch.uint8, device=DEV)
    except torch.cuda.OutOfMemoryError:
        pytest.skip("4.4 GiB of device memory for the 16 400 planes and their bits could not be allocated")
    last = smooth(np.random.default_rng(31), 1, L, L)
    prob[P - 1].copy_(torch.from_numpy(last[0]))
    area = torch.full((P,), -7, dtype=torch.int32, device=DEV)
    hip.edge_pack(prob, S, S, t, bits, area)
    torch.cuda.synchronize()
    want = EO.edge_pack(last, S, S, t)
    assert 0 < want["area"][0] < S * S
    assert np.array_equal(bits[P - 1].cpu().numpy(), want["bits"][0]) and int(area[P - 1]) == want["area"][0]
    assert not area[:P - 1].any() and not bits[:P - 1].any()


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
BAND = ("band_bits", "band_area", "band_inter")
EDGE = ("edge_bits", "edge_area", "edge_band", "edge_inter")
OTHER = ("classes", "pass1_logits", "masks", "edges", "logits", "pred", "mask_bits", "area", "box", "inter") + REGIONS + HOLES + BAND
T = 0.9                                                                           # check_call asserts the maps are neither empty nor full at it
CLASSES = [[0, 1, 2, 3, 4], [4, 3, 2, 1, 0]]                                      # 10 prompts in passes of 4, 4 and 2


@pytest.fixture
def low_maps(monkeypatch):
    """Every low-resolution edge map handed to cvlm_edge_pack while the fixture lives, copied before the call: the chunks of a call,
    in order."""
    from camouflaged_vlm_amd import hip
    seen, real = [], hip.edge_pack

    def spy(prob, *a, **kw):
        seen.append(prob.clone())
        return real(prob, *a, **kw)
    monkeypatch.setattr(hip, "edge_pack", spy)
    return seen


def assert_edges_are_oracle(h, low: np.ndarray, S: int, t: float):
    """The new fields of a result = the oracle on the call's own low-resolution edge maps `low` (P, 4G, 4G); edge_band against the
    result's band_bits, edge_inter = compact_oracle's intersections of edge_bits."""
    n, K, nb = h.edge_bits.shape
    assert low.shape[0] == n * K and nb == S * S // 8 and h.edge_bits.dtype == torch.uint8
    band = None if h.band_bits is None else h.band_bits.cpu().numpy().reshape(n * K, nb)
    want = EO.edge_pack(low, S, S, t, band)
    assert np.array_equal(h.edge_bits.cpu().numpy().reshape(n * K, nb), want["bits"])
    assert tuple(h.edge_area.shape) == (n, K) and h.edge_area.dtype == torch.int32
    assert np.array_equal(h.edge_area.cpu().numpy().ravel(), want["area"])
    if band is None:
        assert h.edge_band is None
    else:
        assert tuple(h.edge_band.shape) == (n, K) and h.edge_band.dtype == torch.int32
        assert np.array_equal(h.edge_band.cpu().numpy().ravel(), want["with_inter"])
        assert np.array_equal(want["with_inter"], EO.popcount(want["bits"] & band))
    if h.inter is not None:                                                       # edge_inter exactly when overlaps=True
        assert tuple(h.edge_inter.shape) == (n, K, K) and h.edge_inter.dtype == torch.int32
        assert np.array_equal(h.edge_inter.cpu().numpy(), XO.inter(h.edge_bits.cpu().numpy()))
        assert torch.equal(torch.diagonal(h.edge_inter, dim1=1, dim2=2), h.edge_area)
    else:
        assert h.edge_inter is None
    return want


def check_call(call, low_maps, S: int, **more):
    """`call(**kw)` runs one entry point: with edge_threshold=T the new fields are the oracle's on the call's own low-resolution maps
    and every other field keeps the bits of the call without it; with masks="both" edge_bits differs from `edges > T` only where
    |edges - T| <= 2^-21."""
    plain = call(**more)
    assert all(getattr(plain, f) is None for f in EDGE) and low_maps == []
    plain = {f: getattr(plain, f).clone() for f in OTHER if getattr(plain, f) is not None}
    h = call(edge_threshold=T, **more)
    torch.cuda.synchronize()
    for f in OTHER:
        assert (getattr(h, f) is None) == (f not in plain), f
    for f, t in plain.items():                                                    # bit for bit, floats included
        assert torch.equal(getattr(h, f).contiguous().view(torch.uint8), t.contiguous().view(torch.uint8)), f
    low = torch.cat(low_maps).cpu().numpy()
    del low_maps[:]
    want = assert_edges_are_oracle(h, low, S, T)
    frac = want["area"] / (S * S)
    print("edge_area", want["area"].tolist(), "edge_band", want.get("with_inter", np.zeros(0)).tolist())
    assert (frac > 0.05).all() and (frac < 0.95).all()
    if "with_inter" in want:
        assert (want["with_inter"] > 0).any() and (want["with_inter"] <= want["area"]).all()
    if h.edges is not None:
        got = np.unpackbits(h.edge_bits.cpu().numpy(), axis=-1).reshape(h.edges.shape).astype(bool)
        e = h.edges.cpu().numpy()
        near = np.abs(e - f32(T)) <= EO.MARGIN
        differ = got != (e > f32(T))
        print(f"masks='both': {int(differ.sum())} pixels differ from edges > {T}, {int(near.sum())} lie within 2^-21 of it")
        assert not (differ & ~near).any()
    return h


@pytest.mark.parametrize("masks", ["bits", "both"])
def test_infer_classes_edge_threshold(tiny, cas, monkeypatch, low_maps, masks):
    g, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    classes = torch.tensor(CLASSES)
    check_call(lambda **kw: cas.infer_classes(inp, ci, cm, classes=classes, masks=masks, band=2, overlaps=True, **kw), low_maps, g.inp_size)
    h = cas.infer_classes(inp, ci, cm, classes=classes, masks=masks, edge_threshold=0.5)     # no band, no overlaps, another threshold
    torch.cuda.synchronize()
    assert h.edge_band is None and h.edge_inter is None and h.band_bits is None
    assert_edges_are_oracle(h, torch.cat(low_maps).cpu().numpy(), g.inp_size, 0.5)


def test_decode_edge_threshold(tiny, cas, monkeypatch, low_maps):
    g, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    enc = cas.encode(inp, ci, cm)
    h = check_call(lambda **kw: cas.decode(enc, topk=5, images=[1, 0, 1], masks="bits", band=2, overlaps=True, **kw), low_maps, g.inp_size)
    for f in EDGE:                                                                # images 1, 0, 1: rows 0 and 2 are the same hypotheses
        assert torch.equal(getattr(h, f)[0], getattr(h, f)[2]), f
    check_call(lambda **kw: cas.decode(enc, topk=5, images=[1, 0, 1], masks="both", band=2, quality=True, stage2=False, **kw), low_maps,
               g.inp_size)


def test_edge_threshold_with_components_and_holes(tiny, cas, monkeypatch, low_maps):
    g, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    classes = torch.tensor(CLASSES)
    more = dict(components=4, min_area=16, holes=4, fill_holes=16, overlaps=True, band=2)
    h = check_call(lambda **kw: cas.infer_classes(inp, ci, cm, classes=classes, masks="bits", **kw), low_maps, g.inp_size, **more)
    S = g.inp_size
    flat = h.mask_bits.cpu().numpy().reshape(-1, h.mask_bits.shape[-1])
    want = CC.components(flat, S, S, 8, 4, 16)
    for f in REGIONS:                                                             # all of them stay functions of mask_bits
        assert np.array_equal(getattr(h, f).cpu().numpy().reshape(want[f].shape), want[f]), f
    want = HO.holes(flat, S, S, 8, 4, 16)
    for f in HOLES:
        assert np.array_equal(getattr(h, f).cpu().numpy().reshape(want[f].shape), want[f]), f
    assert np.array_equal(h.band_bits.cpu().numpy().reshape(flat.shape), MO.morph(flat, S, S, 2)["band_bits"])


def test_a_hypothesis_of_nan_planes_has_no_edge(cas):
    """What a hypothesis of class -1 hands the kernel: NaN planes give zero bits and zero counts."""
    g = cas.g
    L, S = 4 * g.grid, g.inp_size
    prob = torch.full((2, L, L), float("nan"), device=DEV)
    band = torch.full((2, S * S // 8), 0xff, dtype=torch.uint8, device=DEV)
    r = cas.pack_edges(prob, (S, S), threshold=0.5, with_bits=band)
    torch.cuda.synchronize()
    assert not r.bits.any() and not r.area.any() and not r.inter.any()


def test_pack_edges_utility(tiny, cas):
    g, _, _, (inp, ci, cm), _ = tiny
    S, L = g.inp_size, 4 * g.grid
    ms = cas.infer_test_multimask(inp, ci, cm)
    edges = ms.edges.clone()                                                      # (B, S, S): a pure threshold pack
    host = edges.cpu().numpy()
    for t in (0.5, 0.9):
        got = cas.pack_edges(edges, threshold=t)
        torch.cuda.synchronize()
        want = EO.edge_pack(host, S, S, t)
        assert got.inter is None and np.array_equal(got.bits.cpu().numpy(), want["bits"]) and np.array_equal(got.area.cpu().numpy(), want["area"])
        assert np.array_equal(want["bits"], EO.pack(host > f32(t))) and 0 < want["area"].min() and want["area"].max() < S * S
    low = torch.from_numpy(smooth(np.random.default_rng(12), 3, L, L)).to(DEV)    # a low-resolution map with size=(S, S), 4-d, with a band
    mask_bits, _, _ = cas.pack_masks(torch.from_numpy(smooth(np.random.default_rng(13), 3, S, S) - f32(0.5)).to(DEV))
    band = cas.mask_morph(mask_bits, S, S).band_bits
    odd = torch.zeros(band.numel() + 2, dtype=torch.uint8, device=DEV)[2:].view_as(band)      # off a 4-byte boundary: cloned
    odd.copy_(band)
    got = cas.pack_edges(low.view(3, 1, L, L), (S, S), threshold=0.5, with_bits=odd)
    torch.cuda.synchronize()
    want = EO.edge_pack(low.cpu().numpy(), S, S, 0.5, band.cpu().numpy())
    for f, k in (("bits", "bits"), ("area", "area"), ("inter", "with_inter")):
        assert np.array_equal(getattr(got, f).cpu().numpy(), want[k]), f
    # chained: the regions of the packed edge map
    k = cas.mask_components(got.bits, S, S, components=3, min_area=8)
    torch.cuda.synchronize()
    chain = CC.components(want["bits"], S, S, 8, 3, 8)
    for f in REGIONS:
        assert np.array_equal(getattr(k, f).cpu().numpy(), chain[f]), f
    for bad in (dict(prob=low.cpu()), dict(prob=low.double()), dict(prob=low[0, 0]), dict(prob=low.view(1, 3, L, L)), dict(size=(S, S + 8)),
                dict(size=(0, S)), dict(size=S), dict(size=(S, S, S)), dict(size=(float(S), S)), dict(size=(True, S)), dict(threshold=0.0),
                dict(threshold=1), dict(threshold=True), dict(threshold=float("nan")), dict(threshold="0.5"), dict(threshold=None),
                dict(with_bits=band.cpu()), dict(with_bits=band[:2]), dict(with_bits=band.int()), dict(with_bits=band[:, :-4])):
        kw = dict(dict(prob=low, size=(S, S), threshold=0.5), **bad)
        with pytest.raises(ValueError):
            cas.pack_edges(kw.pop("prob"), kw.pop("size"), **kw)
    with pytest.raises(ValueError):
        cas.pack_edges(torch.zeros(2, 8, 40, device=DEV), threshold=0.5)          # size=None: the map's own width must be whole words


def test_bad_edge_requests_raise_and_launch_nothing(tiny, cas):
    from camouflaged_vlm_amd import hip
    _, _, _, (inp, ci, cm), _ = tiny
    enc = cas.encode(inp, ci, cm)
    torch.cuda.synchronize()
    calls = []
    names = ("gemm", "layernorm", "topk_select", "patchify", "split_f32", "expand_blocks", "bilinear", "mask_pack", "mask_morph", "mask_overlap",
             "edge_pack")
    saved = {n: getattr(hip, n) for n in names}
    for n in saved:
        setattr(hip, n, lambda *a, _n=n, **k: calls.append(_n))
    try:
        for kw in (dict(edge_threshold=0.5), dict(masks="logits", edge_threshold=0.5), dict(masks="bits", edge_threshold=0),
                   dict(masks="bits", edge_threshold=1.0), dict(masks="bits", edge_threshold=float("nan")), dict(masks="both", edge_threshold=True),
                   dict(masks="bits", edge_threshold="0.5"), dict(masks="bits", edge_threshold=1 - 1e-12), dict(masks="bits", edge_threshold=-0.1),
                   dict(masks="bits", band=2, edge_threshold=1.5)):
            with pytest.raises(ValueError):
                cas.infer_classes(inp, ci, cm, topk=2, **kw)
            with pytest.raises(ValueError):
                cas.decode(enc, topk=2, **kw)
            with pytest.raises(ValueError):
                cas.pack_edges(torch.zeros(1, 8, 32, device=DEV), threshold=kw["edge_threshold"] if kw["edge_threshold"] != 0.5 else 2.0)
    finally:
        for n, f in saved.items():
            setattr(hip, n, f)
    assert calls == []


def test_edge_memory_is_the_results(tiny, cas, monkeypatch):
    """After one call per mode has sized the grow-only workspaces, masks="bits" with edge_threshold peaks above the same call without
    it by exactly the new result tensors: cvlm_edge_pack has no workspace and no full-resolution edge map exists."""
    g, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    S = g.inp_size
    for overlaps in (False, True):
        modes = {"band": dict(masks="bits", overlaps=overlaps, band=2), "edge": dict(masks="bits", overlaps=overlaps, band=2, edge_threshold=T),
                 "both": dict(masks="both", overlaps=overlaps, band=2)}
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
            if name == "edge":
                new = [getattr(h, f) for f in EDGE if getattr(h, f) is not None]
                assert len(new) == (4 if overlaps else 3)
                results = sum(-(-t.numel() * t.element_size() // 512) * 512 for t in new)             # the allocator's 512-byte blocks
            del h
        print(f"overlaps={overlaps}: peak over the starting level: band {peak['band']} B, with edge_threshold {peak['edge']} B, "
              f"masks='both' {peak['both']} B; new results {results} B")
        assert peak["edge"] - peak["band"] == results
        assert peak["both"] - peak["band"] >= 2 * 10 * S * S * 4                  # what the parent needs to see the edge: two (B, K, S, S) f32


# ---- drop-in -------------------------------------------------------------------------------------------------------------------------------
def test_dropin_passes_edge_threshold_through(tiny, gold, golden_dir, low_maps):
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
        plain = model.infer_classes(inp, ci, cm, topk=3, masks="bits", overlaps=True, band=2)
        assert low_maps == []
        got = model.infer_classes(inp, ci, cm, topk=3, masks="bits", overlaps=True, band=2, edge_threshold=T)
        torch.cuda.synchronize()
        assert_edges_are_oracle(got, torch.cat(low_maps).cpu().numpy(), S, T)
        del low_maps[:]
        dec = model.decode_classes(model.encode_images(inp, ci, cm), topk=3, masks="bits", overlaps=True, band=2, edge_threshold=T)
        torch.cuda.synchronize()
        assert_edges_are_oracle(dec, torch.cat(low_maps).cpu().numpy(), S, T)
        for f in ("classes", "pass1_logits", "logits", "pred", "mask_bits", "area", "box", "inter") + BAND:
            assert torch.equal(getattr(got, f), getattr(plain, f)), f
        edges = model.infer_test_multimask(inp, ci, cm).edges.clone()
        r = model.pack_edges(edges, threshold=0.5)
        torch.cuda.synchronize()
        want = EO.edge_pack(edges.cpu().numpy(), S, S, 0.5)
        assert np.array_equal(r.bits.cpu().numpy(), want["bits"]) and np.array_equal(r.area.cpu().numpy(), want["area"])
