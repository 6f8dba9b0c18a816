"""CPU: masks at each image's own size -- cvlm_debug_mask_pack_sized_host (the kernel's per-pixel functions run
sequentially on the CPU) against tests/sized_oracle.py on the arithmetic and geometry cases and on ragged planes in one call, into
sentinel-filled outputs; cvlm_debug_mask_rle_host_w against tests/rle_oracle.py's definition applied to the unpadded plane; the
refusals of the new entries (no GPU needed: they refuse before launching); the host checks engine.sized_request; the containers."""
import dataclasses

import numpy as np
import pytest
import torch

from camouflaged_vlm_amd import hip, rle
from camouflaged_vlm_amd.engine import ClassHypotheses, MaskRle, SizedMasks, rle_request, sized_request, sized_tables
import rle_oracle as RO
import sized_oracle as SO


# ---- the pack ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", SO.ARITH)
def test_host_entry_equals_oracle_on_the_field(src, dst):
    logits = SO.field(src, dst)
    for level in SO.LEVELS:
        _, planes, area, box, status = SO.run(hip.mask_pack_sized_host, logits[None], [dst], level)
        assert status == 0
        SO.compare(planes[0], area[0], box[0], logits, *dst, level)


def test_host_entry_is_exact_on_geometry_cases():
    """Blocky planes of +-30, every width around the word seam and the ballot halves, heights 1, 2, 33, the four source corners, one
    source row, one source column, +-inf, a NaN plane: all bits, pad bits, area and box, no pixel left out."""
    for name, logits, (h, w) in SO.geometry_cases():
        for level in SO.GEOMETRY_LEVELS:
            _, planes, area, box, status = SO.run(hip.mask_pack_sized_host, logits[None], [(h, w)], level)
            assert status == 0, name
            SO.compare(planes[0], area[0], box[0], logits, h, w, level, exact=True)
            if name == "nan":
                assert area[0] == 0 and box[0].tolist() == [-1] * 4 and not planes[0].any()


def test_identity_size_is_not_the_sign_of_the_logit():
    """At (Hs, Ws) the bits compare sigmoid(logit) * 255 with the level: level 128 needs a probability of 128 / 255 > 1 / 2."""
    logits = np.array([[0.0, 0.001, 0.02, -0.01] * 8], dtype=np.float32)
    _, planes, area, _, _ = SO.run(hip.mask_pack_sized_host, logits[None], [(1, 32)], 128)
    got = SO.unpack_rows(planes[0], 32)[0]
    assert got[:4].tolist() == [False, False, True, False] and area[0] == 8      # sigmoid(0.001) * 255 = 127.56: a positive logit, no bit


def test_ragged_planes_in_one_call_and_refused_tables():
    rng = np.random.default_rng(19)
    logits = (rng.normal(0, 3, (7, 24, 40))).astype(np.float32)
    sizes = SO.RAGGED
    _, planes, area, box, status = SO.run(hip.mask_pack_sized_host, logits, sizes, 128)
    assert status == 0
    for p, (h, w) in enumerate(sizes):
        SO.compare(planes[p], area[p], box[p], logits[p], h, w, 128)
    # no statistics: the same bits
    _, bare, a, b, status = SO.run(hip.mask_pack_sized_host, logits, sizes, 128, stats_out=False)
    assert status == 0 and a is None and all(np.array_equal(x, y) for x, y in zip(bare, planes))
    # plane 2's slice four bytes longer than its size: refused, not read, not stored; its neighbours whole, status 1
    dims, off, total, _ = SO.tables(sizes)
    bad = off.copy()
    bad[3:] += 4
    _, got, area, box, status = SO.run(hip.mask_pack_sized_host, logits, sizes, 128, offsets=bad)
    assert status == 1 and got[2] is None and area[2] == 0 and box[2].tolist() == [-1] * 4
    for p in (0, 1, 3, 4, 5, 6):
        assert np.array_equal(got[p], planes[p]), p
    # the end of the last plane beyond the byte length: that plane alone is dropped
    _, got, area, _, status = SO.run(hip.mask_pack_sized_host, logits, sizes, 128, nbytes=int(off[-1]) - 4)
    assert status == 1 and got[6] is None and area[6] == 0 and all(np.array_equal(got[p], planes[p]) for p in range(6))
    # a negative and a misaligned start
    for first in (-4, SO.GUARD + 2):
        bad = off.copy()
        bad[0] = first
        _, got, _, _, status = SO.run(hip.mask_pack_sized_host, logits, sizes, 128, offsets=bad)
        assert status == 1 and got[0] is None and np.array_equal(got[1], planes[1])


def test_table_sizes_outside_the_bounds_are_refused_by_the_kernel_logic():
    """h or w of the device table outside 1 .. 16384 (the wrapper checks them before upload; the kernel does not trust them)."""
    logits = np.zeros((2, 8, 8), dtype=np.float32)
    for bad in ((0, 8), (8, 0), (-3, 8), (8, 16385), (2 ** 31 - 1, 2 ** 31 - 1)):
        dims = torch.tensor([[4, 8], list(bad)], dtype=torch.int32)
        off = torch.tensor([0, 16, 16 + 64], dtype=torch.int64)
        bits = torch.full((16 + 64,), SO.FILL, dtype=torch.uint8)
        area, box, status = torch.empty(2, dtype=torch.int32), torch.empty(2, 4, dtype=torch.int32), torch.empty(1, dtype=torch.int32)
        hip.mask_pack_sized_host(torch.from_numpy(logits), dims, off, 128, bits, 64, area, box, status)
        assert status.item() == 1 and (bits[16:] == SO.FILL).all() and not bits[:16].any() and area.tolist() == [0, 0], bad


def test_sized_entries_refuse_bad_arguments_without_gpu():
    lib = hip.load()
    p = 1 << 20
    ok = dict(logits=p, P=2, Hs=8, Ws=8, dims=p + 4096, off=p + 8192, level=128, bits=p + 12288, nbytes=4096, words=64, area=p + 16384,
              box=p + 20480, status=p + 24576)
    bad = [dict(logits=None), dict(dims=None), dict(off=None), dict(bits=None), dict(status=None), dict(bits=p + 12290),
           dict(off=p + 8196), dict(dims=p + 4098), dict(logits=p + 1), dict(area=p + 16386), dict(box=p + 20481), dict(status=p + 24578),
           dict(P=0), dict(P=-1), dict(P=65536), dict(Hs=0), dict(Ws=0), dict(Hs=-8),
           dict(Hs=2 ** 16, Ws=2 ** 15), dict(level=0), dict(level=256), dict(level=-1), dict(area=None), dict(box=None),
           dict(nbytes=0), dict(words=0)]
    for kw in bad:
        k = dict(ok, **kw)
        args = (k["logits"], k["P"], k["Hs"], k["Ws"], k["dims"], k["off"], k["level"], k["bits"], k["nbytes"], k["words"], k["area"],
                k["box"], k["status"])
        assert lib.cvlm_mask_pack_sized(*args, None) == -1, kw
        assert lib.cvlm_debug_mask_pack_sized_host(*args) == -1, kw


# ---- run-length encoding with a true width -----------------------------------------------------------------------------------------------
def host_rle_w(bits: np.ndarray, H: int, Wt: int):
    """cvlm_debug_mask_rle_host_w, count then emit, into sentinel-filled outputs -> (n_runs, each plane's counts)."""
    P, W = bits.shape[0], 32 * ((Wt + 31) // 32)
    b = torch.from_numpy(np.ascontiguousarray(bits))
    n = torch.full((P,), -7, dtype=torch.int32)
    hip.mask_rle_host_w(b, H, W, Wt, n)
    first = n.clone()
    off = torch.zeros(P + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(n.long() + 3, 0)
    counts = torch.full((int(off[-1]),), -9, dtype=torch.int32)
    status = torch.full((1,), -3, dtype=torch.int32)
    hip.mask_rle_host_w(b, H, W, Wt, n, off, counts, status)
    assert status.item() == 0 and torch.equal(n, first)
    c, o = counts.numpy(), off.numpy()
    for p in range(P):
        assert (c[o[p] + first[p]:o[p + 1]] == -9).all(), p
    return first.numpy(), [c[o[p]:o[p] + first[p]] for p in range(P)]


@pytest.mark.parametrize("H,Wt", SO.RLE_SIZES)
def test_host_rle_with_a_true_width_equals_the_definition_on_the_unpadded_plane(H, Wt):
    cases = SO.rle_cases(H, Wt)
    planes = np.stack(list(cases.values()))
    want = [RO.plane_counts(m) for m in planes]
    for garbage in (False, True):                                     # whatever the pad bits hold
        n, got = host_rle_w(SO.pack_planes(planes, garbage, seed=H + Wt), H, Wt)
        assert n.tolist() == [len(w) for w in want]
        for name, g, w, m in zip(cases, got, want, planes):
            assert np.array_equal(g, w), (name, garbage)
            assert int(g.sum()) == H * Wt and np.array_equal(rle.decode(g, H, Wt), m), name
    assert want[2].tolist() == ([H * Wt - 1, 1] if H * Wt > 1 else [0, 1])         # pixel (H - 1, Wt - 1): no transition at H * Wt


@pytest.mark.parametrize("H,W", [(8, 64), (33, 64), (65, 96)])
def test_true_width_equal_to_the_pitch_is_the_existing_entry(H, W):
    bits = RO.pack(np.stack(list(RO.cases(H, W).values())))
    n, got = host_rle_w(bits, H, W)
    want = RO.encode(bits, H, W)
    b = torch.from_numpy(bits)
    old = torch.empty(bits.shape[0], dtype=torch.int32)
    hip.mask_rle_host(b, H, W, old)
    assert old.tolist() == n.tolist() and all(np.array_equal(g, w) for g, w in zip(got, want))


def test_rle_w_entries_refuse_bad_widths_without_gpu():
    lib = hip.load()
    p = 1 << 20
    one = lib.cvlm_mask_rle_workspace_bytes(1, 4, 64)
    for Wt, rc in ((64, None), (33, None), (32, -1), (65, -1), (0, -1), (-5, -1)):
        got = lib.cvlm_debug_mask_rle_host_w(p, 1, 4, 64, Wt, None, None, None, 0, None)     # n_runs NULL refuses after the widths pass
        assert got == -1
        if rc == -1:
            assert lib.cvlm_mask_rle_count_w(p, 1, 4, 64, Wt, p + 4096, None) == -1, Wt
            assert lib.cvlm_mask_rle_emit_w(p, 1, 4, 64, Wt, p + 8192, p + 12288, 8, p + 16384, p + 65536, one, None) == -1, Wt
    for kw in (dict(bits=None), dict(W=48), dict(H=0), dict(P=0)):
        k = dict(dict(bits=p, P=1, H=4, W=64), **kw)
        assert lib.cvlm_mask_rle_count_w(k["bits"], k["P"], k["H"], k["W"], k["W"], p + 4096, None) == -1, kw


# ---- the host request and the containers ---------------------------------------------------------------------------------------------------
def test_sized_request_accepts_and_refuses():
    assert sized_request(n=2) is None and sized_request(n=2, masks="logits") is None
    assert sized_request(sizes=[(3, 4), (5, 6)], n=2) == ([(3, 4), (5, 6)], 128)
    assert sized_request(sizes=((np.int64(3), 4),), sized_level=np.int32(1), n=1, masks="both", rle="sized") == ([(3, 4)], 1)
    assert sized_request(sizes=np.array([[16384, 1]]), n=1, sized_level=255) == ([(16384, 1)], 255)
    bad = [dict(sizes=[(3, 4)]), dict(sizes=[(3, 4)] * 3), dict(sizes=[(3, 4), (5,)]), dict(sizes=[(3, 4), (5, 6, 7)]), dict(sizes=[(3, 4), 5]),
           dict(sizes=[(3, 4), (5.0, 6)]), dict(sizes=[(3, 4), (True, 6)]), dict(sizes=[(3, 4), (0, 6)]), dict(sizes=[(3, 4), (5, 16385)]),
           dict(sizes=[(3, 4), (-1, 6)]), dict(sizes=[(3, 4), "56"]), dict(sizes="3456"), dict(sizes=7),
           dict(sizes=[(3, 4), (5, 6)], sized_level=0), dict(sizes=[(3, 4), (5, 6)], sized_level=256), dict(sized_level=0),
           dict(sizes=[(3, 4), (5, 6)], sized_level=128.0), dict(sizes=[(3, 4), (5, 6)], sized_level=True),
           dict(sizes=[(3, 4), (5, 6)], masks="logits"), dict(rle="sized"), dict(rle="sized", masks="both")]
    for kw in bad:
        with pytest.raises(ValueError):
            sized_request(**dict(dict(n=2), **kw))
    with pytest.raises(ValueError, match="infer_classes"):
        sized_request(rle="sized", n=1, who="infer_classes")
    assert rle_request(rle="sized", masks="bits") == "sized"
    with pytest.raises(ValueError):
        rle_request(rle="sized", masks="logits")


def test_sized_tables():
    dims, off, max_words = sized_tables([(1, 1), (70, 33), (5, 65)])
    assert dims.dtype == np.int32 and dims.tolist() == [[1, 1], [70, 33], [5, 65]]
    assert off.dtype == np.int64 and off.tolist() == [0, 4, 4 + 70 * 8, 4 + 70 * 8 + 5 * 12] and max_words == 140


def test_sized_masks_on_host_tensors():
    sizes = [(3, 33), (2, 5)]
    rng = np.random.default_rng(3)
    masks = [rng.random(s) < 0.5 for s in sizes]
    rows = [SO.pack_rows(m) for m in masks]
    bits = torch.from_numpy(np.concatenate([r.reshape(-1) for r in rows]))
    s = SizedMasks(bits=bits, offsets=torch.tensor([0, 24, 32]), area=torch.zeros(2, dtype=torch.int32), box=torch.zeros(2, 4, dtype=torch.int32),
                   status=torch.zeros(1, dtype=torch.int32), sizes=sizes)
    assert s.level == 128 and tuple(s.plane(0).shape) == (3, 8) and tuple(s.plane(1).shape) == (2, 4)
    assert s.plane(1).data_ptr() == bits.data_ptr() + 24                           # a view
    for p in range(2):
        assert np.array_equal(s.to_numpy(p), masks[p])
    s.check()
    s.status = torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(RuntimeError):
        s.check()


def test_mask_rle_carries_each_planes_size():
    sizes = [(3, 33), (2, 5)]
    rng = np.random.default_rng(4)
    masks = [rng.random(s) < 0.5 for s in sizes]
    want = [RO.plane_counts(m) for m in masks]
    off = np.concatenate([[0], np.cumsum([len(w) for w in want])])
    r = MaskRle(counts=torch.from_numpy(np.concatenate(want).astype(np.int32)), offsets=torch.from_numpy(off),
                n_runs=torch.tensor([len(w) for w in want], dtype=torch.int32), size=None, sizes=sizes)
    assert [f.name for f in dataclasses.fields(r)] == ["counts", "offsets", "n_runs", "size"]
    for compressed in (False, True):
        for p, d in enumerate(r.to_coco(compressed=compressed)):
            assert d["size"] == list(sizes[p])
            c = rle.string_to_counts(d["counts"]) if compressed else d["counts"]
            assert np.array_equal(rle.decode(c, *sizes[p]), masks[p])
    same = MaskRle(counts=r.counts, offsets=r.offsets, n_runs=r.n_runs, size=(4, 32))
    assert same.sizes is None and same.size_of(1) == (4, 32)


def test_class_hypotheses_sized_field_is_optional():
    t = torch.zeros(1)
    h = ClassHypotheses(classes=t, pass1_logits=t, masks=t, edges=t, logits=t, pred=t)
    assert h.sized is None
    assert [f.name for f in dataclasses.fields(h)] == ["classes", "pass1_logits", "masks", "edges", "logits", "pred"]
    assert ClassHypotheses(classes=t, pass1_logits=t, masks=None, edges=None, logits=t, pred=t, sized="s").sized == "s"


def test_new_symbols_are_exported_at_abi_12():
    assert hip.ABI_VERSION == 12 and hip.load().cvlm_abi_version() == 12
    for name in ("cvlm_mask_pack_sized", "cvlm_debug_mask_pack_sized_host", "cvlm_mask_rle_count_w", "cvlm_mask_rle_emit_w",
                 "cvlm_debug_mask_rle_host_w"):
        assert name in hip.EXPORTS
    assert hip._SIGNATURES["cvlm_mask_pack_sized"] == hip._SIGNATURES["cvlm_debug_mask_pack_sized_host"] + "s"
