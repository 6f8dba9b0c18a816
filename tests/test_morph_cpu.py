"""CPU: morphology of packed masks -- the oracle (tests/morph_oracle.py: the reference's max_pool2d lines for the band,
scipy.ndimage for dilation and erosion) against the plain double loop over the clipped window, cvlm_debug_mask_morph_host (the kernel's
per-thread functions run sequentially on the CPU) against the oracle on every operator case and on the reference's own planes
(tests/golden/demo_classes_digest.npz), the set identities, the refusals of the entries (no GPU needed: they refuse before launching)
and the host check of the engine's argument (engine.morph_request)."""
import dataclasses
import itertools
import os

import numpy as np
import pytest
import torch

from camouflaged_vlm_amd import hip, spec
from camouflaged_vlm_amd.engine import ClassHypotheses, morph_request
import compact_oracle as XO
import morph_oracle as MO

PAIRS = ("dil", "ero", "band")


def host_morph(bits: np.ndarray, H: int, W: int, r: int, pairs=PAIRS) -> dict:
    """cvlm_debug_mask_morph_host into sentinel-filled outputs -> the oracle's dict, the pairs asked for only."""
    P = bits.shape[0]
    b = torch.from_numpy(np.ascontiguousarray(bits))
    out = {}
    for name in pairs:
        out[name + "_bits"] = torch.full_like(b, 0xa5)
        out[name + "_area"] = torch.full((P,), -7, dtype=torch.int32)
    hip.mask_morph_host(b, H, W, r, **out)
    return {k: v.numpy() for k, v in out.items()}


def assert_equal(got: dict, want: dict, what) -> None:
    assert set(got) <= set(want), what
    for k, v in got.items():
        assert v.dtype == want[k].dtype and np.array_equal(v, want[k]), (what, k)


def test_oracle_equals_the_plain_double_loop():
    """The reference's max_pool2d band and scipy's dilation / erosion against any / all over the clipped window, on a dozen 8 x 32
    planes at every radius."""
    rng = np.random.default_rng(5)
    planes = [rng.random((8, 32)) < d for d in (0.02, 0.05, 0.1, 0.3, 0.5, 0.7, 0.9, 0.95, 0.98)]
    planes += [np.zeros((8, 32), bool), np.ones((8, 32), bool), MO.operator_cases()["seam"][0][0, :, :32]]
    assert len(planes) == 12
    stack = np.stack(planes)
    for r in MO.RADII:
        dil, ero = MO.dilate_erode(stack, r)
        band = MO.reference_band(stack, r)
        for p, plane in enumerate(planes):
            d, e, b = MO.plain(plane, r)
            assert np.array_equal(dil[p], d) and np.array_equal(ero[p], e) and np.array_equal(band[p], b), (r, p)
        assert np.array_equal(band, dil & ~ero)


CASES = [(name, r) for name, (_, radii) in sorted(MO.operator_cases().items()) for r in radii]


@pytest.mark.parametrize("name,r", CASES)
def test_host_entry_equals_oracle_on_operator_cases(name, r):
    planes = MO.operator_cases()[name][0]
    P, H, W = planes.shape
    bits = MO.pack(planes)
    assert_equal(host_morph(bits, H, W, r), MO.morph(bits, H, W, r), (name, r))


def test_operator_cases_are_what_they_claim():
    c = MO.operator_cases()
    area = lambda name, r: {k: v.tolist() for k, v in MO.morph(MO.pack(c[name][0]), *c[name][0].shape[1:], r).items() if k.endswith("area")}
    for r in MO.RADII:
        a = area("one_word", r)                                                   # empty, full, one pixel at x = 13, alternating
        assert a["dil_area"] == [0, 32, min(13, r) + 1 + min(18, r), 32] and a["ero_area"] == [0, 32, 0, 0]
        assert a["band_area"] == [0, 0, a["dil_area"][2], 32]
        a = area("seam", r)                                                       # x = 31 and x = 32 of 64, rows 4 - r .. 4 + r of 8
        rows = min(4, r) + 1 + min(3, r)
        assert a["dil_area"] == [rows * (2 * r + 1)] * 2
        a = area("row_ends", r)                                                   # (10, 63) and (30, 0) of 40 x 64: r + 1 columns each
        assert a["dil_area"][0] == (min(10, r) + 1 + min(29, r) + min(30, r) + 1 + min(9, r)) * (r + 1)
        a = area("plane_ends", r)                                                 # the last row of plane 0 and the first of plane 3
        assert a["dil_area"] == [min(8, r + 1) * 64, 0, 0, min(8, r + 1) * 64] and a["ero_area"] == [0, 0, 0, 0]
        a = area("corner_interior", r)
        assert a["dil_area"] == [(r + 1) ** 2] * 4 + [(2 * r + 1) ** 2]
        a = area(f"squares_r{r}", r)
        assert a["ero_area"] == [1, 0] and a["dil_area"] == [(4 * r + 1) ** 2, (4 * r) ** 2] and a["band_area"][1] == a["dil_area"][1]
        a = area("full_pinhole_frame", r)                                         # H = 40: the frame's two sides meet from r = 20 on
        assert a["band_area"][0] == 0 and a["ero_area"][0] == 40 * 64 and a["ero_area"][1] == 40 * 64 - (2 * r + 1) ** 2
        assert a["ero_area"][2] == 40 * 64 - (r + 1) * (2 * r + 1) and a["ero_area"][3] == 0
        assert a["dil_area"][3] == 40 * 64 - max(0, 40 - 2 * (r + 1)) * (64 - 2 * (r + 1))
    a = area("three_words", 16)                                                   # x = 47 of 96: columns 31 .. 63, all 5 rows
    assert a["dil_area"] == [5 * 33, 5 * (16 + 32 + 16)]
    five = MO.morph(MO.pack(c["five_words"][0]), 5, 160, 16)["dil_bits"].reshape(2, 5, 5, 4)
    assert not five[:, :, 0].any() and not five[:, :, 4].any() and five[1, :, 1].any() and five[1, :, 3].any()
    a = area("blob", 16)                                                          # non-degenerate at the largest radius
    assert a == dict(dil_area=[72 * 102], ero_area=[8 * 38], band_area=[72 * 102 - 8 * 38])


def test_duality_inclusion_and_areas_on_random_planes():
    planes = MO.operator_cases()["random"][0]
    P, H, W = planes.shape
    bits = MO.pack(planes)
    for r in MO.RADII:
        got, neg = host_morph(bits, H, W, r), host_morph(~bits, H, W, r)
        assert np.array_equal(got["ero_bits"], ~neg["dil_bits"]) and np.array_equal(got["dil_bits"], ~neg["ero_bits"])   # ero(X) = ~dil(~X)
        assert np.array_equal(got["band_bits"], neg["band_bits"])
        assert not (got["ero_bits"] & ~bits).any() and not (bits & ~got["dil_bits"]).any()                                 # ero <= X <= dil
        assert np.array_equal(got["band_bits"], got["dil_bits"] & ~got["ero_bits"])
        for name in PAIRS:
            assert np.array_equal(got[name + "_area"], XO.stats(XO.unpack(got[name + "_bits"], H, W))[0])


def test_every_subset_of_the_pairs_gives_the_same_bits():
    planes = MO.operator_cases()["random"][0]
    P, H, W = planes.shape
    bits = MO.pack(planes)
    for r in (1, 16):
        full = host_morph(bits, H, W, r)
        for n in (1, 2):
            for pairs in itertools.combinations(PAIRS, n):
                got = host_morph(bits, H, W, r, pairs)
                assert sorted(got) == sorted(p + s for p in pairs for s in ("_bits", "_area"))
                assert_equal(got, full, (r, pairs))


@pytest.fixture(scope="module")
def ref_bits(golden_dir):
    with np.load(os.path.join(golden_dir, "demo_classes_digest.npz")) as z:
        bits = z["mask_bits"]
    return np.ascontiguousarray(bits.reshape(-1, bits.shape[-1]))


@pytest.mark.parametrize("r", [1, 2])
def test_host_entry_equals_oracle_on_the_reference_planes(ref_bits, r):
    """Also the figures that show the fixture is not degenerate at these radii: erosion leaves something, the band is not the plane."""
    S = spec.DEMO_SAM.inp_size
    assert ref_bits.shape == (6, S * S // 8)
    want = MO.morph(ref_bits, S, S, r)
    assert_equal(host_morph(ref_bits, S, S, r), want, r)
    print(f"reference planes, r = {r}: " + ", ".join(f"{k} {v.min()} - {v.max()}" for k, v in want.items() if k.endswith("area")))
    assert (want["ero_area"] > 0).all() and (want["band_area"] < S * S).all() and (want["band_area"] > 0).all()
    if r == 1:
        assert (want["dil_area"].min(), want["dil_area"].max()) == (365376, 445650)
        assert (want["ero_area"].min(), want["ero_area"].max()) == (24386, 46916)
        assert (want["band_area"].min(), want["band_area"].max()) == (340990, 398734)
    else:
        assert (want["ero_area"].min(), want["ero_area"].max()) == (777, 3059)
        assert (want["band_area"].min(), want["band_area"].max()) == (615999, 703031)


# ---- the entries refuse before they touch anything --------------------------------------------------------------------------------------
def test_mask_morph_refuses_bad_arguments_without_gpu():
    lib = hip.load()
    n = 2 * 4 * 64 // 8                                                            # bytes of the two planes
    p = 1 << 20
    ok = dict(bits=p, P=2, H=4, W=64, r=2, dil=p + 4096, dil_a=p + 65536, ero=p + 8192, ero_a=p + 65600, band=p + 12288, band_a=p + 65664)
    bad = [dict(bits=None), dict(bits=p + 2), dict(dil=p + 4098), dict(ero=p + 8193), dict(band=p + 12290), dict(P=0), dict(P=-1), dict(P=65536),
           dict(H=0), dict(H=-4), dict(W=0), dict(W=-64), dict(W=48), dict(W=8), dict(H=2 ** 16, W=2 ** 15), dict(H=2 ** 20, W=2 ** 20),
           dict(r=0), dict(r=-1), dict(r=17), dict(r=2 ** 20),
           dict(dil=None), dict(dil_a=None), dict(ero=None), dict(ero_a=None), dict(band=None), dict(band_a=None),     # a pair with one NULL
           dict(dil=None, dil_a=None, ero=None, ero_a=None, band=None, band_a=None),                                   # nothing asked for
           dict(dil=p), dict(ero=p), dict(band=p), dict(band=p + n - 4), dict(dil=p - n + 4),                          # an output on the input
           dict(ero=p + 4096), dict(band=p + 4096 + n - 4), dict(band=p + 8192 - n + 4),                               # ... on another output
           dict(dil=None, dil_a=None, ero=None, ero_a=None, band=p + 4)]                                               # band alone, in place

    def args(kw):
        a = dict(ok, **kw)
        return (a["bits"], a["P"], a["H"], a["W"], a["r"], a["dil"], a["dil_a"], a["ero"], a["ero_a"], a["band"], a["band_a"])
    for kw in bad:
        assert lib.cvlm_mask_morph(*args(kw), None) == -1, kw
        assert lib.cvlm_debug_mask_morph_host(*args(kw)) == -1, kw
    # what is accepted, on real host memory: ranges that touch but do not intersect, and band alone
    planes = MO.operator_cases()["seam"][0]
    bits = MO.pack(planes)
    buf = torch.zeros(4 * bits.size, dtype=torch.uint8)
    flat = bits.reshape(-1)
    buf[:flat.size] = torch.from_numpy(flat)
    src, dil, ero, band = (buf[k * flat.size:(k + 1) * flat.size].view(2, -1) for k in range(4))
    areas = torch.full((3, 2), -7, dtype=torch.int32)
    hip.mask_morph_host(src, 8, 64, 2, dil, areas[0], ero, areas[1], band, areas[2])
    want = MO.morph(bits, 8, 64, 2)
    assert np.array_equal(dil.numpy(), want["dil_bits"]) and np.array_equal(band.numpy(), want["band_bits"])
    assert np.array_equal(areas.numpy(), np.stack([want["dil_area"], want["ero_area"], want["band_area"]]))
    with pytest.raises(RuntimeError):
        hip.mask_morph_host(src, 8, 64, 2, band_bits=buf[4:4 + flat.size].view(2, -1), band_area=areas[2])


# ---- the host request -----------------------------------------------------------------------------------------------------------------------
def test_morph_request_accepts_and_refuses():
    assert morph_request(masks="logits") == (False, 0, False)                     # the default: nothing asked for
    assert morph_request(masks="bits", overlaps=True, side=48) == (False, 0, False)
    assert morph_request(band=2, masks="bits") == (True, 2, False)
    assert morph_request(band=1, masks="both", overlaps=True, side=1024) == (True, 1, True)
    assert morph_request(band=np.int64(16), masks="bits", side=320) == (True, 16, False)
    bad = [dict(band=0), dict(band=17), dict(band=-2), dict(band=2.0), dict(band="2"), dict(band=True), dict(band=np.bool_(True)),
           dict(band=2, masks="logits"), dict(band=2, side=48), dict(band=2, side=1000)]
    for kw in bad:
        with pytest.raises(ValueError):
            morph_request(**dict(dict(masks="bits"), **kw))
    with pytest.raises(ValueError, match="infer_classes"):
        morph_request(band=99, masks="bits", who="infer_classes")


def test_class_hypotheses_band_fields_are_optional():
    t = torch.zeros(1)
    h = ClassHypotheses(classes=t, pass1_logits=t, masks=t, edges=t, logits=t, pred=t)
    names = ("band_bits", "band_area", "band_inter")
    assert all(getattr(h, n) is None for n in names)
    assert [f.name for f in dataclasses.fields(h)] == ["classes", "pass1_logits", "masks", "edges", "logits", "pred"]
    h = ClassHypotheses(classes=t, pass1_logits=t, masks=None, edges=None, logits=t, pred=t, mask_bits=t, **{n: t for n in names})
    assert all(getattr(h, n) is t for n in names) and h.n_holes is None and h.kept_bits is None and h.inter is None


def test_new_symbols_are_exported_at_abi_12():
    assert hip.ABI_VERSION == 12 and hip.load().cvlm_abi_version() == 12
    assert "cvlm_mask_morph" in hip.EXPORTS and "cvlm_debug_mask_morph_host" in hip.EXPORTS
    assert hip._SIGNATURES["cvlm_mask_morph"] == hip._SIGNATURES["cvlm_debug_mask_morph_host"] + "s"
