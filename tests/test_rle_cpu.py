"""CPU: run-length encoding of packed masks -- the oracle (tests/rle_oracle.py: the definition in numpy) against a plain
pixel loop, cvlm_debug_mask_rle_host (the kernels' per-thread functions run sequentially on the CPU) against the oracle on every
operator case and on the reference's own planes (tests/golden/demo_classes_digest.npz), the host module rle.py (COCO's compressed
string, decode), the refusals of the entries (no GPU needed: they refuse before launching) and the host check of the engine's
argument (engine.rle_request).  Every comparison is exact and goes into sentinel-filled outputs."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from camouflaged_vlm_amd import hip, rle, spec
from camouflaged_vlm_amd.engine import ClassHypotheses, MaskRle, rle_request
import rle_oracle as RO

SHAPES = [(1, 32), (1, 64), (8, 64), (31, 64), (32, 64), (33, 64), (65, 96)]


def host_rle(bits: np.ndarray, H: int, W: int, gap: int = 0):
    """cvlm_debug_mask_rle_host, count then emit, into sentinel-filled outputs -> (n_runs, list of each plane's counts).  gap: spare
    elements of each plane's slice, which must keep their sentinel."""
    P = bits.shape[0]
    b = torch.from_numpy(np.ascontiguousarray(bits))
    n = torch.full((P,), -7, dtype=torch.int32)
    hip.mask_rle_host(b, H, W, n)
    first = n.clone()
    off = torch.zeros(P + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(n.long() + gap, 0)
    counts = torch.full((int(off[-1]),), -9, dtype=torch.int32)
    status = torch.full((1,), -3, dtype=torch.int32)
    n.fill_(-7)
    hip.mask_rle_host(b, H, W, n, off, counts, status)
    assert status.item() == 0 and torch.equal(n, first)
    c, o = counts.numpy(), off.numpy()
    for p in range(P):
        assert (c[o[p] + first[p]:o[p + 1]] == -9).all(), p
    return first.numpy(), [c[o[p]:o[p] + first[p]] for p in range(P)]


def test_oracle_equals_the_pixel_loop():
    """A dozen 8 x 32 planes: densities, empty, full, the corners."""
    rng = np.random.default_rng(18)
    planes = [rng.random((8, 32)) < d for d in (0.02, 0.1, 0.3, 0.5, 0.7, 0.9, 0.98)]
    planes += [RO.cases(8, 32)[k] for k in ("empty", "full", "first_pixel", "last_pixel", "checker")]
    assert len(planes) == 12
    for p, plane in enumerate(planes):
        assert RO.plane_counts(plane).tolist() == RO.plane_counts_loop(plane), p


def test_the_definitions_consequences():
    H, W = 8, 64
    c = RO.cases(H, W)
    assert RO.plane_counts(c["empty"]).tolist() == [H * W]
    assert RO.plane_counts(c["full"]).tolist() == [0, H * W]
    assert RO.plane_counts(c["first_pixel"]).tolist() == [0, 1, H * W - 1]
    assert RO.plane_counts(c["last_pixel"]).tolist() == [H * W - 1, 1]
    assert RO.plane_counts(c["column"]).tolist() == [33 * H, H, 30 * H]
    assert RO.plane_counts(c["seam_below"]).tolist() == [32 * H - 1, 1, 32 * H]      # (H - 1, 31) set, (0, 32) clear
    assert RO.plane_counts(c["seam_above"]).tolist() == [32 * H, 1, 31 * H + H - 1]  # the reverse
    assert len(RO.plane_counts(c["stripes"])) == H * W and len(RO.plane_counts(c["checker"])) == W * (H - 1) + 1


@pytest.mark.parametrize("H,W", SHAPES)
def test_host_entry_equals_oracle_on_operator_cases(H, W):
    """Every case of the shape as one batch of planes (so every plane has a neighbour it must not join), with and without spare room
    in the slices; decode returns the plane, the counts sum to H * W, the compressed string round-trips."""
    cases = RO.cases(H, W)
    planes = np.stack(list(cases.values()))
    bits = RO.pack(planes)
    want = RO.encode(bits, H, W)
    for gap in (0, 3):
        n, got = host_rle(bits, H, W, gap)
        assert n.tolist() == [len(w) for w in want]
        for name, g, w, plane in zip(cases, got, want, planes):
            assert g.dtype == np.int32 and np.array_equal(g, w), (name, gap)
            assert int(g.sum()) == H * W and np.array_equal(rle.decode(g, H, W), plane), name
            assert np.array_equal(rle.string_to_counts(rle.counts_to_string(g)), w), name


def test_two_planes_do_not_join():
    """Plane 0 ends on a set pixel, plane 1 starts on a clear one: plane 1's first run is its own."""
    H, W = 4, 32
    planes = np.zeros((2, H, W), dtype=bool)
    planes[0, H - 1, W - 1] = True
    planes[1, 1, 0] = True
    n, got = host_rle(RO.pack(planes), H, W)
    assert got[0].tolist() == [H * W - 1, 1] and got[1].tolist() == [1, 1, H * W - 2] and n.tolist() == [2, 3]
    planes[1, 0, 0] = True                                           # and a set first pixel starts with a 0 whatever plane 0 ended on
    assert host_rle(RO.pack(planes), H, W)[1][1].tolist() == [0, 2, H * W - 2]


def test_undersized_slot_is_refused_not_overrun():
    """One plane's slice one element short: status 1, nothing outside any slice written, the other planes whole."""
    H, W = 33, 64
    planes = np.stack([RO.cases(H, W)[k] for k in ("random_0.5", "checker", "random_0.01")])
    bits = torch.from_numpy(RO.pack(planes))
    want = RO.encode(bits.numpy(), H, W)
    n = torch.tensor([len(w) for w in want], dtype=torch.int32)
    sizes = n.long().clone()
    sizes[1] -= 1
    off = torch.zeros(4, dtype=torch.int64)
    off[1:] = torch.cumsum(sizes, 0)
    counts = torch.full((int(off[-1]) + 8,), -9, dtype=torch.int32)
    status = torch.full((1,), -3, dtype=torch.int32)
    hip.mask_rle_host(bits, H, W, torch.empty(3, dtype=torch.int32), off, counts, status)
    c = counts.numpy()
    assert status.item() == 1 and (c[off[-1]:] == -9).all()
    assert np.array_equal(c[off[0]:off[1]], want[0]) and np.array_equal(c[off[2]:off[3]], want[2])
    assert np.array_equal(c[off[1]:off[2]], want[1][:-1])             # the slice holds what fits; only the tail run was dropped
    for bad in ([-1, 5, 9, 12], [0, 5, 9, 10 ** 9]):                  # a slice that leaves counts: that plane is dropped whole
        counts.fill_(-9)
        hip.mask_rle_host(bits, H, W, torch.empty(3, dtype=torch.int32), torch.tensor(bad), counts, status)
        assert status.item() == 1


@pytest.fixture(scope="module")
def ref_bits(golden_dir):
    with np.load(os.path.join(golden_dir, "demo_classes_digest.npz")) as z:
        bits = z["mask_bits"]
    return np.ascontiguousarray(bits.reshape(-1, bits.shape[-1]))


def test_host_entry_equals_oracle_on_the_reference_planes(ref_bits):
    """Also the figures that show the fixture is not degenerate -- and that RLE is no compression here: 100 000 - 125 000 counts of 4
    bytes per plane against 128 KiB of bits."""
    S = spec.DEMO_SAM.inp_size
    assert ref_bits.shape == (6, S * S // 8)
    want = RO.encode(ref_bits, S, S)
    n, got = host_rle(ref_bits, S, S)
    print("reference planes: n_runs", n.tolist(), "most transitions in one column",
          [int(np.diff(RO.unpack(b[None], S, S)[0].astype(np.int8), axis=0, prepend=0).astype(bool).sum(0).max()) for b in ref_bits])
    assert (n >= 100000).all() and (n <= 125000).all()
    planes = RO.unpack(ref_bits, S, S)
    for p in range(6):
        assert np.array_equal(got[p], want[p]), p
        assert np.array_equal(rle.decode(got[p], S, S), planes[p])
        assert np.array_equal(rle.string_to_counts(rle.counts_to_string(got[p])), want[p])


# ---- rle.py -----------------------------------------------------------------------------------------------------------------------------------
# Derived by hand from the algorithm in rle.py's docstring (difference to counts[i - 2] for i > 2, 5-bit groups low first, 0x20 = more,
# 0x10 of the last group = sign, + 48), NOT taken from pycocotools, which is not a dependency of this project.
STRING_VECTORS = [([0, 5, 3, 100, 2], b"053o2O"), ([1048576], b"PPPP1"), ([0, 1048576], b"0PPPP1"),
                  ([7, 1, 1000, 1, 3, 40000, 16, 15, 17], b"71Xo00kPOoQW1=_nhN1")]


@pytest.mark.parametrize("counts,string", STRING_VECTORS)
def test_compressed_string_vectors(counts, string):
    assert rle.counts_to_string(counts) == string
    assert rle.counts_to_string(np.asarray(counts, dtype=np.int32)) == string
    assert rle.string_to_counts(string).tolist() == counts and rle.string_to_counts(string.decode()).tolist() == counts


def test_rle_module_refuses_what_is_no_encoding():
    with pytest.raises(ValueError):
        rle.decode([3, 4], 2, 32)
    with pytest.raises(ValueError):
        rle.decode([65, -1], 2, 32)
    with pytest.raises(ValueError):
        rle.string_to_counts(b"o")                                   # "more" and then nothing
    with pytest.raises(ValueError):
        rle.string_to_counts(b"0 1")
    assert rle.decode([0, 64], 2, 32).all() and not rle.decode([64], 2, 32).any()


def test_mask_rle_to_coco_on_host_tensors():
    """MaskRle is a plain container: to_coco works on whatever device its tensors live on."""
    H, W = 8, 64
    planes = np.stack([RO.cases(H, W)[k] for k in ("random_0.5", "empty", "full")])
    want = RO.encode(RO.pack(planes), H, W)
    off = np.concatenate([[0], np.cumsum([len(w) for w in want])])
    r = MaskRle(counts=torch.from_numpy(np.concatenate(want).astype(np.int32)), offsets=torch.from_numpy(off),
                n_runs=torch.tensor([len(w) for w in want], dtype=torch.int32), size=(H, W))
    assert [f.name for f in dataclasses.fields(r)] == ["counts", "offsets", "n_runs", "size"] and r.status is None
    plain, packed = r.to_coco(), r.to_coco(compressed=True)
    for p in range(3):
        assert plain[p]["size"] == [H, W] and plain[p]["counts"] == want[p].tolist() and isinstance(plain[p]["counts"], list)
        assert isinstance(packed[p]["counts"], bytes)
        assert np.array_equal(rle.decode(rle.string_to_counts(packed[p]["counts"]), H, W), planes[p])
    with pytest.raises(RuntimeError):
        MaskRle(counts=r.counts, offsets=r.offsets, n_runs=r.n_runs, size=(H, W), status=torch.ones(1, dtype=torch.int32)).to_coco()


# ---- the entries refuse before they touch anything --------------------------------------------------------------------------------------
def test_mask_rle_entries_refuse_bad_arguments_without_gpu():
    lib = hip.load()
    p = 1 << 20
    one = lib.cvlm_mask_rle_workspace_bytes(1, 4, 64)
    assert one == 4 * 64 // 32 * 12 and lib.cvlm_mask_rle_workspace_bytes(5, 4, 64) == 5 * one
    assert lib.cvlm_mask_rle_workspace_bytes(3, 33, 64) == 3 * 800      # 33 * 2 * 12 = 792 bytes, in 16-byte units
    assert lib.cvlm_mask_rle_workspace_bytes(1, 1024, 1024) == 1024 * 1024 * 3 // 8   # 0.375 byte per pixel
    ok = dict(bits=p, P=2, H=4, W=64, n=p + 4096, off=p + 8192, counts=p + 12288, total=64, status=p + 16384, ws=p + 65536, ws_bytes=2 * one)
    planes = [dict(bits=None), dict(bits=p + 2), dict(P=0), dict(P=-1), dict(P=65536), dict(H=0), dict(H=-4), dict(W=0), dict(W=-64),
              dict(W=48), dict(W=8), dict(H=2 ** 16, W=2 ** 15), dict(H=2 ** 20, W=2 ** 20)]
    emit = [dict(off=None), dict(off=p + 8196), dict(counts=None), dict(counts=p + 12290), dict(status=None), dict(status=p + 16385),
            dict(total=0), dict(total=-5)]
    space = [dict(ws=None), dict(ws=p + 65540), dict(ws_bytes=one - 1), dict(ws_bytes=0), dict(ws_bytes=-1)]
    a = lambda kw: dict(ok, **kw)
    for kw in planes + [dict(n=None), dict(n=p + 4097)]:
        k = a(kw)
        assert lib.cvlm_mask_rle_count(k["bits"], k["P"], k["H"], k["W"], k["n"], None) == -1, kw
        assert lib.cvlm_debug_mask_rle_host(k["bits"], k["P"], k["H"], k["W"], k["n"], None, None, 0, None) == -1, kw
    for kw in planes + emit + space:
        k = a(kw)
        assert lib.cvlm_mask_rle_emit(k["bits"], k["P"], k["H"], k["W"], k["off"], k["counts"], k["total"], k["status"], k["ws"],
                                      k["ws_bytes"], None) == -1, kw
    for kw in planes + emit + [dict(n=None)]:
        if kw == dict(counts=None):                                  # the host entry's count-only form, not a refusal
            continue
        k = a(kw)
        assert lib.cvlm_debug_mask_rle_host(k["bits"], k["P"], k["H"], k["W"], k["n"], k["off"], k["counts"], k["total"], k["status"]) == -1, kw
    for kw in planes[2:]:
        k = a(kw)
        assert lib.cvlm_mask_rle_workspace_bytes(k["P"], k["H"], k["W"]) == -1, kw
    with pytest.raises(RuntimeError):
        hip.mask_rle_workspace_bytes(1, 4, 48)


# ---- the host request -----------------------------------------------------------------------------------------------------------------------
def test_rle_request_accepts_and_refuses():
    assert rle_request(masks="logits") is None                       # the default: nothing asked for
    assert rle_request(masks="bits", side=48) is None
    assert rle_request(rle="mask", masks="bits") == "mask_bits"
    assert rle_request(rle="kept", masks="both", min_area=1, side=1024) == "kept_bits"
    assert rle_request(rle="filled", masks="bits", fill_holes=np.int64(16), side=320) == "filled_bits"
    bad = [dict(rle="bits"), dict(rle=""), dict(rle=True), dict(rle=1), dict(rle=b"mask"), dict(rle="mask", masks="logits"),
           dict(rle="kept"), dict(rle="kept", min_area=0), dict(rle="kept", fill_holes=5), dict(rle="filled"),
           dict(rle="filled", fill_holes=0), dict(rle="filled", min_area=5), dict(rle="mask", side=48), dict(rle="mask", side=1000)]
    for kw in bad:
        with pytest.raises(ValueError):
            rle_request(**dict(dict(masks="bits"), **kw))
    with pytest.raises(ValueError, match="infer_classes"):
        rle_request(rle="runs", masks="bits", who="infer_classes")


def test_class_hypotheses_rle_field_is_optional():
    t = torch.zeros(1)
    h = ClassHypotheses(classes=t, pass1_logits=t, masks=t, edges=t, logits=t, pred=t)
    assert h.rle is None
    assert [f.name for f in dataclasses.fields(h)] == ["classes", "pass1_logits", "masks", "edges", "logits", "pred"]
    h = ClassHypotheses(classes=t, pass1_logits=t, masks=None, edges=None, logits=t, pred=t, mask_bits=t, rle="r")
    assert h.rle == "r" and h.mask_bits is t and h.edge_bits is None


def test_new_symbols_are_exported_at_abi_12():
    assert hip.ABI_VERSION == 12 and hip.load().cvlm_abi_version() == 12
    for name in ("cvlm_mask_rle_workspace_bytes", "cvlm_mask_rle_count", "cvlm_mask_rle_emit", "cvlm_debug_mask_rle_host"):
        assert name in hip.EXPORTS
