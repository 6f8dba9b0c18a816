"""CPU: packed edge maps -- the oracle (tests/edges_oracle.py: the float32 bilinear value restated operation by operation)
against the plain double loop and against torch.nn.functional.interpolate on the reference's own low-resolution edge maps
(tests/golden/tiny_classes.npz), cvlm_debug_edge_pack_host (the kernel's per-pixel functions run sequentially on the CPU) against the
oracle on every operator case, the refusals of the entries (no GPU needed: they refuse before launching), the launcher's choice between
its two kernel instances and the host check of the engine's argument (engine.edge_request)."""
import dataclasses
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from camouflaged_vlm_amd import hip
from camouflaged_vlm_amd.engine import ClassHypotheses, edge_request
import edges_oracle as EO

f32 = np.float32


def host_pack(prob: np.ndarray, hout: int, wout: int, t: float, with_bits=None) -> dict:
    """cvlm_debug_edge_pack_host into sentinel-filled outputs -> the oracle's dict."""
    P = prob.shape[0]
    bits = torch.full((P, hout * wout // 8), 0xa5, dtype=torch.uint8)
    area = torch.full((P,), -7, dtype=torch.int32)
    out = dict(bits=bits, area=area)
    if with_bits is None:
        hip.edge_pack_host(torch.from_numpy(np.ascontiguousarray(prob)), hout, wout, t, bits, area)
    else:
        out["with_inter"] = torch.full((P,), -7, dtype=torch.int32)
        hip.edge_pack_host(torch.from_numpy(np.ascontiguousarray(prob)), hout, wout, t, bits, area,
                           torch.from_numpy(np.ascontiguousarray(with_bits)), out["with_inter"])
    return {k: v.numpy() for k, v in out.items()}


def assert_equal(got: dict, want: dict, what) -> None:
    assert set(got) == set(want), what
    for k, v in got.items():
        assert v.dtype == want[k].dtype and np.array_equal(v, want[k]), (what, k)


@pytest.fixture(scope="module")
def low_edges(golden_dir):
    with np.load(os.path.join(golden_dir, "tiny_classes.npz")) as z:
        return z["low_edges"]                                                      # (2, 5, 80, 80) f32: the reference's own maps


def test_oracle_equals_the_plain_double_loop():
    """The vectorised restatement against one output pixel at a time, on a dozen tiny planes: up-scales, a shrink, one-pixel axes,
    special values."""
    rng = np.random.default_rng(3)
    planes = [(rng.random((3, 5)).astype(f32), 7, 32), (rng.random((5, 3)).astype(f32), 13, 32), (rng.random((1, 1)).astype(f32), 3, 32),
              (rng.random((1, 9)).astype(f32), 1, 32), (rng.random((9, 1)).astype(f32), 9, 32), (rng.random((8, 8)).astype(f32), 8, 32),
              (rng.random((8, 8)).astype(f32), 32, 32), (rng.random((20, 70)).astype(f32), 6, 32), (rng.random((4, 4)).astype(f32), 16, 64),
              (rng.random((7, 11)).astype(f32) * f32(1e-40), 9, 32)]
    special = rng.random((6, 6)).astype(f32)
    special[2, 3], special[0, 0], special[5, 1] = np.nan, np.inf, -np.inf
    planes += [(special, 24, 32), (-rng.random((6, 6)).astype(f32), 5, 32)]
    assert len(planes) == 12
    for plane, ho, wo in planes:
        assert np.array_equal(EO.value(plane[None], ho, wo)[0], EO.plain(plane, ho, wo), equal_nan=True), (plane.shape, ho, wo)


def test_oracle_against_interpolate_on_the_reference_maps(low_edges):
    """|v - F.interpolate| <= 2^-21 on the reference's maps at 4 x (operands in [0, 1]: each of the at most nine roundings by which
    two evaluation orders differ is <= 2^-25), and a thresholded pixel differs from `interpolate > t` only inside that margin."""
    S = 320
    v = EO.value(low_edges, S, S)
    ref = F.interpolate(torch.from_numpy(low_edges), size=(S, S), mode="bilinear", align_corners=False).numpy()
    assert low_edges.min() >= 0 and low_edges.max() <= 1
    dev = float(np.abs(v - ref).max())
    print(f"max |oracle - interpolate| = {dev:.3g}")
    assert dev <= EO.MARGIN
    for t in (0.1, 0.5, 0.9):
        differ = EO.above(v, t) != (ref > f32(t))
        near = np.abs(ref - f32(t)) <= EO.MARGIN
        print(f"t = {t}: {int(differ.sum())} pixels differ, {int(near.sum())} lie within 2^-21 of t")
        assert not (differ & ~near).any()


def test_fixture_is_neither_empty_nor_full(low_edges):
    S = 320
    v = EO.value(low_edges, S, S)
    for t in (0.5, 0.9):
        frac = EO.above(v, t).mean(axis=(2, 3))
        print(f"t = {t}: set fractions {frac.min():.3f} .. {frac.max():.3f}")
        if t == 0.9:
            assert (frac > 0.05).all() and (frac < 0.95).all()


CASES = sorted(EO.operator_cases())


@pytest.mark.parametrize("name", CASES)
def test_host_entry_equals_oracle_on_operator_cases(name):
    prob, ho, wo, thresholds = EO.operator_cases()[name]
    rng = np.random.default_rng(len(name))
    for t in thresholds:
        want = EO.edge_pack(prob, ho, wo, t)
        assert_equal(host_pack(prob, ho, wo, t), want, (name, t))
        other = EO.pack(rng.random((prob.shape[0], ho, wo)) < 0.5)
        assert_equal(host_pack(prob, ho, wo, t, other), EO.edge_pack(prob, ho, wo, t, other), (name, t, "with"))


def test_operator_cases_are_what_they_claim():
    c = EO.operator_cases()
    prob, ho, wo, _ = c["identity"]
    for t in (0.25, 0.5, 0.9):                                                     # scale 1: prob > t
        assert np.array_equal(EO.edge_pack(prob, ho, wo, t)["bits"], EO.pack(prob > f32(t)))
    prob, ho, wo, _ = c["identity_at_threshold"]
    at = prob == f32(0.5)
    got = np.unpackbits(EO.edge_pack(prob, ho, wo, 0.5)["bits"], axis=1).reshape(prob.shape).astype(bool)
    assert at.sum() > 100 and not got[at].any() and np.array_equal(got, prob > f32(0.5))
    prob, ho, wo, _ = c["special_values"]
    got = np.unpackbits(EO.edge_pack(prob, ho, wo, 0.5)["bits"], axis=1).reshape(-1, ho, wo).astype(bool)
    v = EO.value(prob, ho, wo)
    assert np.isnan(v[0]).sum() >= 16 and not got[0][np.isnan(v[0])].any()         # the NaN's output neighbourhoods are clear
    ys, xs = np.nonzero(np.isnan(v[0]))
    assert ys.min() >= 4 * 4 - 2 and ys.max() <= 4 * 6 + 1 and xs.min() >= 4 * 6 - 2 and xs.max() <= 4 * 8 + 1   # source (5, 7) at 4 x
    assert got[1][v[1] == np.inf].all() and (v[1] == np.inf).any() and not got[1][v[1] == -np.inf].any()
    assert got[3].any() and not got[3][8:22, 12:34].any()                          # denormals stay below any threshold
    prob, ho, wo, _ = c["checkerboard"]
    got = np.unpackbits(EO.edge_pack(prob, ho, wo, 0.5)["bits"], axis=1).reshape(ho, wo)
    assert got.sum() == ho * wo // 2
    prob, ho, wo, _ = c["ramp"]
    got = np.unpackbits(EO.edge_pack(prob, ho, wo, 0.5)["bits"], axis=1).reshape(3, ho, wo)
    assert not got[0, :, :80].any() and got[0, :, 80:].all()                       # crosses between pixels 79 and 80 of word 2
    assert got[1, :, :80].all() and not got[1, :, 80:].any()
    assert not got[2, :, :32].any() and got[2, :, 32:].all()                       # ... between the last pixel of word 0 and the first of word 1


def test_with_inter_is_the_popcount_of_the_and(low_edges):
    prob = np.ascontiguousarray(low_edges[0, :3])
    rng = np.random.default_rng(8)
    for density in (0.02, 0.5, 0.98):
        other = EO.pack(rng.random((3, 320, 320)) < density)
        got = host_pack(prob, 320, 320, 0.9, other)
        assert_equal(got, EO.edge_pack(prob, 320, 320, 0.9, other), density)
        assert np.array_equal(got["with_inter"], EO.popcount(got["bits"] & other))
        assert np.array_equal(got["bits"], host_pack(prob, 320, 320, 0.9)["bits"])  # the area-only form: the same bits


# ---- the entries refuse before they touch anything --------------------------------------------------------------------------------------
def test_edge_pack_refuses_bad_arguments_without_gpu():
    lib = hip.load()
    p = 1 << 20
    n_in, n_out = 2 * 4 * 8 * 4, 2 * 8 * 32 // 8                                    # bytes of the two source planes and of their bits
    ok = dict(prob=p, P=2, hin=4, win=8, hout=8, wout=32, t=0.5, bits=p + 4096, area=p + 8192, wb=p + 12288, wi=p + 16384)
    nan, inf = float("nan"), float("inf")
    bad = [dict(prob=None), dict(bits=None), dict(area=None), dict(bits=p + 4098), dict(bits=p + 4097), dict(wb=p + 12290),
           dict(P=0), dict(P=-1), dict(P=65536), dict(hin=0), dict(hin=-4), dict(win=0), dict(win=-8), dict(hout=0), dict(hout=-8),
           dict(wout=0), dict(wout=-32), dict(wout=48), dict(wout=8), dict(hout=2 ** 16, wout=2 ** 15), dict(hout=2 ** 20, wout=2 ** 20),
           dict(hin=2 ** 16, win=2 ** 15), dict(hin=2 ** 20, win=2 ** 20),
           dict(t=0.0), dict(t=1.0), dict(t=-0.5), dict(t=1.5), dict(t=nan), dict(t=inf), dict(t=-inf), dict(t=-0.0),
           dict(wb=None), dict(wi=None),                                                                          # exactly one of the pair
           dict(bits=p), dict(bits=p + n_in - 4), dict(bits=p - n_out + 4), dict(area=p + 4), dict(wi=p + n_in - 4),   # an output on prob
           dict(bits=p + 12288), dict(bits=p + 12288 + n_out - 4), dict(area=p + 12288), dict(wi=p + 12288 + 4),    # ... on with_bits
           dict(area=p + 4096), dict(area=p + 4096 + n_out - 4), dict(wi=p + 4096), dict(wi=p + 8192), dict(wi=p + 8192 + 4),   # ... on another output
           dict(area=p + 4096 - 4), dict(wb=None, wi=None, bits=p), dict(wb=None, wi=None, area=p + 4096)]

    def args(kw):
        a = dict(ok, **kw)
        return (a["prob"], a["P"], a["hin"], a["win"], a["hout"], a["wout"], a["t"], a["bits"], a["area"], a["wb"], a["wi"])
    for kw in bad:
        assert lib.cvlm_edge_pack(*args(kw), None) == -1, kw
        assert lib.cvlm_debug_edge_pack_host(*args(kw)) == -1, kw
    # what is accepted, on real host memory: ranges that touch but do not intersect, and thresholds next to the interval's ends
    prob = np.random.default_rng(2).random((2, 4, 8)).astype(f32)
    buf = torch.zeros(n_in + 2 * n_out + 16, dtype=torch.uint8)
    src = buf[:n_in].view(torch.float32).view(2, 4, 8)
    src.copy_(torch.from_numpy(prob))
    bits, other = buf[n_in:n_in + n_out].view(2, -1), buf[n_in + n_out:n_in + 2 * n_out].view(2, -1)
    sums = buf[n_in + 2 * n_out:].view(torch.int32).view(2, 2)
    other.fill_(0xf0)
    for t in (0.5, float(np.nextafter(f32(0), f32(1))), float(np.nextafter(f32(1), f32(0)))):
        hip.edge_pack_host(src, 8, 32, t, bits, sums[0], other, sums[1])
        want = EO.edge_pack(prob, 8, 32, t, other.numpy().copy())
        assert np.array_equal(bits.numpy(), want["bits"]) and np.array_equal(sums.numpy(), np.stack([want["area"], want["with_inter"]]))
    with pytest.raises(RuntimeError):
        hip.edge_pack_host(src, 8, 32, 0.5, buf[n_in - 4:n_in - 4 + n_out].view(2, -1), sums[0])


def test_launcher_chooses_the_staged_instance_by_the_footprint():
    """cvlm_debug_edge_pack_staged is the launcher's own choice: the LDS-staged instance when a bound on a tile's source footprint
    (256 x 64 output pixels) fits 4864 floats, the direct one otherwise."""
    staged = hip.edge_pack_staged
    assert staged(80, 80, 320, 320) and staged(256, 256, 1024, 1024) and staged(192, 192, 1024, 1024)    # the model's 4 x and beyond
    assert staged(512, 512, 1024, 1024)                                                                    # 2 x: 132 x 36 <= 4864
    assert staged(1, 1, 1, 32) and staged(2, 2, 8, 32) and staged(32, 32, 32, 32) and staged(37, 53, 101, 96)   # small planes fit whole
    assert not staged(1024, 1024, 1024, 1024) and not staged(320, 320, 320, 320)                           # scale 1 on large planes
    assert not staged(100, 100, 32, 32) and not staged(2048, 2048, 1024, 1024) and not staged(640, 640, 320, 320)   # shrinks
    assert not staged(64, 4096, 64, 4096) and staged(16, 4096, 64, 16384)                                  # wide: 260 x 64 vs 68 x 16

    def bound(hin, win, hout, wout):
        cols, rows = min(win, int(win / wout * 256) + 4), min(hin, int(hin / hout * 64) + 4)
        return cols * rows <= 4864
    rng = np.random.default_rng(6)
    for _ in range(300):
        hin, win, hout = (int(v) for v in rng.integers(1, 700, 3))
        wout = 32 * int(rng.integers(1, 40))
        assert staged(hin, win, hout, wout) == bound(hin, win, hout, wout), (hin, win, hout, wout)
    for bad in ((0, 4, 4, 32), (4, 4, 4, 48), (4, 4, -1, 32), (4, 4, 2 ** 16, 2 ** 15), (2 ** 16, 2 ** 15, 4, 32)):
        with pytest.raises(RuntimeError):
            staged(*bad)


# ---- the host request -----------------------------------------------------------------------------------------------------------------------
def test_edge_request_accepts_and_refuses():
    assert edge_request(masks="logits") == (False, 0.0, False, False)              # the default: nothing asked for
    assert edge_request(masks="bits", overlaps=True, band=2, side=48) == (False, 0.0, False, False)
    assert edge_request(edge_threshold=0.5, masks="bits") == (True, 0.5, False, False)
    assert edge_request(edge_threshold=0.5, masks="both", overlaps=True, band=2, side=1024) == (True, 0.5, True, True)
    assert edge_request(edge_threshold=np.float32(0.9), masks="bits", band=1, side=320) == (True, float(f32(0.9)), True, False)
    assert edge_request(edge_threshold=0.9, masks="bits")[1] == float(f32(0.9))    # the float32 the kernel compares against
    bad = [dict(edge_threshold=0), dict(edge_threshold=1), dict(edge_threshold=0.0), dict(edge_threshold=1.0), dict(edge_threshold=-0.5),
           dict(edge_threshold=1.5), dict(edge_threshold=float("nan")), dict(edge_threshold=float("inf")), dict(edge_threshold=True),
           dict(edge_threshold=np.bool_(True)), dict(edge_threshold="0.5"), dict(edge_threshold=[0.5]), dict(edge_threshold=0.5 + 0j),
           dict(edge_threshold=1 - 1e-12), dict(edge_threshold=1e-60),                                  # float32 rounds them to 1 and to 0
           dict(edge_threshold=0.5, masks="logits"), dict(edge_threshold=0.5, side=48), dict(edge_threshold=0.5, side=1000)]
    for kw in bad:
        with pytest.raises(ValueError):
            edge_request(**dict(dict(masks="bits"), **kw))
    with pytest.raises(ValueError, match="infer_classes"):
        edge_request(edge_threshold=2, masks="bits", who="infer_classes")


def test_class_hypotheses_edge_fields_are_optional():
    t = torch.zeros(1)
    h = ClassHypotheses(classes=t, pass1_logits=t, masks=t, edges=t, logits=t, pred=t)
    names = ("edge_bits", "edge_area", "edge_band", "edge_inter")
    assert all(getattr(h, n) is None for n in names)
    assert [f.name for f in dataclasses.fields(h)] == ["classes", "pass1_logits", "masks", "edges", "logits", "pred"]
    h = ClassHypotheses(classes=t, pass1_logits=t, masks=None, edges=None, logits=t, pred=t, mask_bits=t, **{n: t for n in names})
    assert all(getattr(h, n) is t for n in names) and h.band_bits is None and h.kept_bits is None and h.inter is None


def test_new_symbols_are_exported_at_abi_12():
    assert hip.ABI_VERSION == 12 and hip.load().cvlm_abi_version() == 12
    assert "cvlm_edge_pack" in hip.EXPORTS and "cvlm_debug_edge_pack_host" in hip.EXPORTS
    assert hip._SIGNATURES["cvlm_edge_pack"] == hip._SIGNATURES["cvlm_debug_edge_pack_host"] + "s"
