"""Instances without a device: the sequential host entries cvlm_debug_mask_regions_sized_host and
cvlm_debug_region_alpha_host -- the kernels' own per-thread functions -- against the oracle (tests/regions_oracle.py) on every hand-made
plane as ONE ragged call, for M in {1, 5, 64}, both connectivities and min_area in {0, 1, 4}; pad bits; a refused plane; every refusal of
the C entries and of regions_request; the bookkeeping of MaskRegions.compact and instances_to_coco on host tensors; the slot layout; the
ABI.  Every comparison of bits, tables and counts is exact."""
import ctypes

import numpy as np
import pytest
import torch

pytest.importorskip("scipy.ndimage")
import regions_oracle as GO  # noqa: E402
import rowops_oracle as RO  # noqa: E402


def hip():
    from camouflaged_vlm_amd import hip as h
    return h


def maskpost():
    from camouflaged_vlm_amd import maskpost as m
    return m


ALL = [p for _, p in GO.planes()]
NAMES = [n for n, _ in GO.planes()]


@pytest.mark.parametrize("min_area", [0, 1, 4])
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("M", [1, 5, 64])
def test_host_entry_equals_the_oracle_on_one_ragged_call(M, connectivity, min_area):
    GO.same(GO.run(hip().mask_regions_sized_host, ALL, connectivity, M, min_area), GO.expected(connectivity, M, min_area))


def test_the_named_cases():
    at = {n: i for i, n in enumerate(NAMES)}
    e4, e8 = GO.expected(4, 5, 0), GO.expected(8, 5, 0)
    n4, n8 = (lambda name: int(e4["n_regions"][at[name]])), (lambda name: int(e8["n_regions"][at[name]]))
    assert (n4("row end 4x64"), n8("row end 4x64")) == (2, 2)
    assert (n4("diagonal seam 3x70"), n8("diagonal seam 3x70")) == (3, 1)
    assert (n4("diagonal_seam[0]"), n8("diagonal_seam[0]")) == (2, 1)
    assert (n4("board_and_u[0]"), n8("board_and_u[0]")) == (512, 1)                  # the full count, not capped at M = 5
    assert e4["table"][at["board_and_u[0]"]][:, 5].tolist() == [0, 2, 4, 6, 8]       # equal areas: the lowest seeds
    assert n8("serpentine_squares_three[0]") == 1 and n8("empty 5x33") == 0 and n8("full 5x33") == 1
    sq = e8["table"][at["serpentine_squares_three[1]"]]
    assert sq[0, 0] == sq[1, 0] == 25 and sq[0, 5] < sq[1, 5] and sq[2].tolist() == list(GO.FILLER)
    three = GO.expected(8, 5, 4)
    i = at["three 9x45"]
    assert int(e8["n_regions"][i]) == 3 and int(three["n_regions"][i]) == 2
    assert three["table"][i][:, 0].tolist() == [39, 10, 0, 0, 0]
    got = GO.run(hip().mask_regions_sized_host, [ALL[i]], 8, 5, 4)
    slots = got["out_bits"].reshape(5, -1)
    assert not slots[2:].any() and slots[0].any() and slots[1].any()                 # zero planes past the two real regions
    both = GO.unpack_rows(slots[0], 9, 45)[0] | GO.unpack_rows(slots[1], 9, 45)[0]
    assert int((ALL[i] & ~both).sum()) == 2                                          # the middle region of 2 pixels is dropped


def test_set_pad_bits_are_ignored():
    for connectivity in (4, 8):
        GO.same(GO.run(hip().mask_regions_sized_host, ALL, connectivity, 5, 0, dirty=True), GO.expected(connectivity, 5, 0))


def test_every_output_plane_has_clear_pad_bits_and_partitions_the_kept_pixels():
    got = GO.run(hip().mask_regions_sized_host, ALL, 8, 64, 0, dirty=True)
    _, off, _ = GO.tables([p.shape for p in ALL])
    for p, plane in enumerate(ALL):
        h, w = plane.shape
        size = int(off[p + 1] - off[p])
        union, total = np.zeros_like(plane), 0
        for m in range(64):
            lo = 64 * int(off[p]) + m * size
            s, pad = GO.unpack_rows(got["out_bits"][lo:lo + size], h, w)
            assert not pad
            total += int(s.sum())
            union |= s
        assert total == int(union.sum()) and not (union & ~plane).any()
        if got["n_regions"][p] <= 64:
            assert np.array_equal(union, plane), NAMES[p]


def test_the_slot_layout_is_sized_tables_of_the_repeated_sizes():
    sizes = [p.shape for p in ALL]
    _, off, _ = maskpost().sized_tables(sizes)
    for M in (1, 5, 64):
        _, rep, _ = maskpost().sized_tables([z for z in sizes for _ in range(M)])
        for p in range(len(sizes)):
            for m in range(M):
                assert rep[p * M + m] == M * off[p] + m * (off[p + 1] - off[p])
        assert rep[-1] == M * off[-1]
    # and the entry stores there: slot p * M + m read through SizedMasks' own tables is row m's plane
    pick = list(range(0, len(ALL), 3))
    regs = host_regions([ALL[i] for i in pick], 5)
    for p, i in enumerate(pick):
        want = GO.split(ALL[i], *GO.labelled(i, 8), 5, 0)[2]
        for m in range(5):
            assert np.array_equal(regs.masks.to_numpy(p * 5 + m), want[m]), (NAMES[i], m)


def test_a_plane_whose_slice_does_not_fit_is_refused():
    h = hip()
    planes = [ALL[0], np.ones((5, 33), bool), ALL[1]]
    dims, off, max_words = GO.tables([p.shape for p in planes])
    bits = torch.from_numpy(np.concatenate([GO.pack_rows(p) for p in planes]))
    dims = dims.copy()
    dims[1] = (6, 33)                                                 # six rows do not fit a slice of five
    M = 3
    n, table, status = torch.full((3,), -7, dtype=torch.int32), torch.full((3, M, 6), -7, dtype=torch.int32), torch.full((1,), 7, dtype=torch.int32)
    out = torch.full((M * bits.numel(),), 0xA5, dtype=torch.uint8)
    h.mask_regions_sized_host(bits, torch.from_numpy(off), torch.from_numpy(dims), max_words, 8, 0, n, table, out, status)
    assert int(status) == 1 and int(n[1]) == 0 and table[1].tolist() == [list(GO.FILLER)] * M
    assert not out[M * int(off[1]):M * int(off[2])].any()
    want = GO.run(h.mask_regions_sized_host, [planes[0], planes[2]], 8, M, 0)
    assert n[[0, 2]].tolist() == want["n_regions"].tolist() and np.array_equal(table[[0, 2]].numpy(), want["table"])
    # a plane of more words than max_words is refused as well: the grids would not cover it
    h.mask_regions_sized_host(bits, torch.from_numpy(off), torch.from_numpy(GO.tables([p.shape for p in planes])[0]), 1, 8, 0, n, table, out, status)
    assert int(status) == 1 and int(n[1]) == 0


def test_the_c_entries_refuse_what_the_header_lists():
    lib = hip().load()
    E = -1                                                            # CVLM_E_BADARG
    planes = [np.ones((5, 33), bool), np.ones((2, 64), bool)]
    dims, off, max_words = GO.tables([p.shape for p in planes])
    bits = torch.from_numpy(np.concatenate([GO.pack_rows(p) for p in planes]))
    M = 4
    d, o = torch.from_numpy(dims), torch.from_numpy(off)
    n, table, status = torch.zeros(2, dtype=torch.int32), torch.zeros(2, M, 6, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    out = torch.zeros(M * bits.numel(), dtype=torch.uint8)
    need = lib.cvlm_mask_regions_workspace_bytes(bits.numel(), 2, max_words)
    assert need == 112 * bits.numel() and lib.cvlm_mask_regions_workspace_bytes(4 * max_words, 1, max_words) == GO.WS_PER_WORD * max_words
    for bad in ((3, 1, 1), (8, 0, 1), (8, 65536, 1), (8, 1, 0), (8, 1, 16384 * 512 + 1)):
        assert lib.cvlm_mask_regions_workspace_bytes(*bad) == E
    ws = torch.zeros(need + 16, dtype=torch.uint8)
    good = dict(bits=bits.data_ptr(), nb=bits.numel(), off=o.data_ptr(), dims=d.data_ptr(), P=2, mw=max_words, conn=8, M=M, min_area=0,
                ws=ws.data_ptr(), wsb=need, n=n.data_ptr(), table=table.data_ptr(), out=out.data_ptr(), status=status.data_ptr())
    order = ("bits", "nb", "off", "dims", "P", "mw", "conn", "M", "min_area", "ws", "wsb", "n", "table", "out", "status")
    host_order = tuple(k for k in order if k not in ("ws", "wsb"))
    dev = lambda a: lib.cvlm_mask_regions_sized(*[a[k] for k in order], None)
    host = lambda a: lib.cvlm_debug_mask_regions_sized_host(*[a[k] for k in host_order])
    assert host(good) == 0
    bad = [dict(good, **{k: None}) for k in ("bits", "off", "dims", "n", "table", "out", "status")]
    bad += [dict(good, **{k: good[k] + 2}) for k in ("bits", "dims", "n", "table", "out", "status")] + [dict(good, off=good["off"] + 4)]
    bad += [dict(good, P=0), dict(good, P=65536), dict(good, nb=3), dict(good, mw=0), dict(good, mw=16384 * 512 + 1), dict(good, M=0),
            dict(good, M=65), dict(good, conn=5), dict(good, conn=0), dict(good, min_area=-1), dict(good, out=good["bits"]),
            dict(good, n=good["status"]), dict(good, table=good["dims"])]
    for i, a in enumerate(bad):
        assert host(a) == E, i
        assert dev(a) == E, i                                         # before anything touches the device: none is needed
    for a in (dict(good, ws=None), dict(good, ws=good["ws"] + 8), dict(good, wsb=GO.WS_PER_WORD * max_words - 1), dict(good, wsb=0),
              dict(good, ws=good["out"]), dict(good, ws=good["bits"])):
        assert dev(a) == E
    # cvlm_region_alpha
    alpha, src, res = torch.zeros(2, 8, 8), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 8, 8)
    g = dict(bits=bits.data_ptr(), nb=bits.numel(), off=o.data_ptr(), dims=d.data_ptr(), Q=2, alpha=alpha.data_ptr(), N=2, R=8,
             src=src.data_ptr(), out=res.data_ptr(), status=status.data_ptr())
    adev = lambda a: lib.cvlm_region_alpha(*a.values(), None)
    ahost = lambda a: lib.cvlm_debug_region_alpha_host(*a.values())
    assert ahost(g) == 0
    for a in [dict(g, **{k: None}) for k in ("bits", "off", "dims", "alpha", "src", "out", "status")] + \
            [dict(g, R=0), dict(g, R=-1), dict(g, Q=0), dict(g, N=0), dict(g, nb=0), dict(g, alpha=g["alpha"] + 2)]:
        assert ahost(a) == E and adev(a) == E


@pytest.mark.parametrize("R", [7, 56])
def test_region_alpha_host_against_the_oracle(R):
    rng = np.random.default_rng(R)
    planes = [np.ones((1, 1), bool), rng.random((5, 33)) < 0.5, rng.random((20, 30)) < 0.5, rng.random((R, R)) < 0.5, np.ones((R, R), bool),
              rng.random((90, 130)) < 0.5]
    alpha = torch.from_numpy(rng.random((3, R, R)).astype(np.float32))
    src = [0, 1, 2, 0, 1, 2]
    out, status = GO.run_alpha(hip().region_alpha_host, planes, alpha, src)
    assert status == 0
    err = RO.rowerr(out, GO.region_alpha(planes, alpha, src), row_dims=2)
    print(f"R = {R}: rowerr {err:.3g}")
    assert err <= 1e-6
    assert RO.same_bits(out[3], alpha[0] * torch.from_numpy(planes[3].astype(np.float32)))       # (R, R): the gate is the bit
    assert RO.same_bits(out[4], alpha[1])                                                        # a full (R, R) plane: alpha itself
    out, status = GO.run_alpha(hip().region_alpha_host, planes[:2], alpha, [0, 3])
    assert status == 1 and not out[1].any() and RO.same_bits(out[0], alpha[0])                   # a src outside [0, N): refused, zeroed


def test_regions_request_refuses_before_any_launch():
    req = maskpost().regions_request
    assert req([(5, 33)], regions=64, min_area=0, connectivity=4) == ([(5, 33)], 64, 0, 4)
    assert maskpost().REGIONS_MAXM == 64 == hip().REGIONS_MAXM
    for kw in (dict(regions=0), dict(regions=65), dict(regions=True), dict(regions=2.0), dict(regions=None), dict(min_area=-1),
               dict(min_area=2 ** 31), dict(min_area=1.5), dict(min_area=False), dict(connectivity=6), dict(connectivity="8"),
               dict(connectivity=True)):
        with pytest.raises(ValueError):
            req([(5, 33)], **kw)
    for sizes in ([], "ab", [(0, 3)], [(3, 16385)], [(3,)], [(True, 3)], [(2.0, 3)], None, [(1, 1)] * 65536):
        with pytest.raises(ValueError):
            req(sizes)


def host_regions(planes, M, connectivity=8, min_area=0):
    """A MaskRegions on host tensors, from the host entry."""
    mp = maskpost()
    got = GO.run(hip().mask_regions_sized_host, planes, connectivity, M, min_area)
    sizes = [p.shape for p in planes]
    slots = [z for z in sizes for _ in range(M)]
    table = torch.from_numpy(got["table"])
    masks = mp.SizedMasks(bits=torch.from_numpy(got["out_bits"]), offsets=torch.from_numpy(mp.sized_tables(slots)[1]),
                          area=table[..., 0].reshape(-1), box=table[..., 1:5].reshape(-1, 4), status=torch.tensor([got["status"]], dtype=torch.int32),
                          sizes=slots, level=128)
    return mp.MaskRegions(n_regions=torch.from_numpy(got["n_regions"]), table=table, masks=masks, M=M)


def test_compact_keeps_the_real_regions_in_slot_order():
    at = {n: i for i, n in enumerate(NAMES)}
    pick = [at["empty 5x33"], at["three 9x45"], at["board_and_u[0]"], at["full 1x1"], at["empty 5x33"]]
    planes = [ALL[i] for i in pick]
    regs = host_regions(planes, 4, connectivity=4)
    regs.check()
    out, plane_of, rank = regs.compact()
    assert plane_of.dtype == np.int64 and rank.dtype == np.int64
    assert plane_of.tolist() == [1, 1, 1, 2, 2, 2, 2, 3] and rank.tolist() == [0, 1, 2, 0, 1, 2, 3, 0]
    assert out.sizes == [(9, 45)] * 3 + [(32, 32)] * 4 + [(1, 1)] and out.level == 128
    assert out.area.tolist() == [39, 10, 2, 1, 1, 1, 1, 1] and out.box[0].tolist() == [30, 5, 42, 7]
    assert out.offsets.tolist() == maskpost().sized_tables(out.sizes)[1].tolist() and int(out.offsets[-1]) == out.bits.numel()
    want = GO.expected(4, 4, 0, which=pick)["out_bits"]
    _, off, _ = maskpost().sized_tables(regs.masks.sizes)
    for q, (p, m) in enumerate(zip(plane_of, rank)):
        lo, hi = out.byte_range(q)
        assert np.array_equal(out.bits[lo:hi].numpy(), want[int(off[p * 4 + m]):int(off[p * 4 + m + 1])])
        assert int(out.to_numpy(q).sum()) == int(out.area[q])
    # nothing real at all: empty tensors; a refused plane: RuntimeError
    none, p_of, r_of = host_regions([ALL[at["empty 5x33"]]], 2).compact()
    assert none.bits.numel() == 0 and none.sizes == [] and none.offsets.tolist() == [0] and p_of.size == 0 and r_of.size == 0
    regs.masks.status[0] = 1
    with pytest.raises(RuntimeError):
        regs.compact()
    with pytest.raises(RuntimeError):
        regs.check()


def test_instances_to_coco_builds_result_dicts():
    to_coco = maskpost().instances_to_coco
    rows = [{"size": [4, 5], "counts": [3, 2, 15]}, {"size": [2, 2], "counts": [0, 4]}]
    got = to_coco(rows, [7, 9], torch.tensor([3, 1]), np.array([0.5, 0.25], np.float32), boxes=torch.tensor([[1, 0, 2, 3], [0, 0, 1, 1]]))
    assert got == [{"image_id": 7, "category_id": 3, "segmentation": rows[0], "score": 0.5, "bbox": [1, 0, 2, 4]},
                   {"image_id": 9, "category_id": 1, "segmentation": rows[1], "score": 0.25, "bbox": [0, 0, 2, 2]}]
    assert all(type(d["image_id"]) is int and type(d["score"]) is float for d in got)
    assert "bbox" not in to_coco(rows, [7, 9], [3, 1], [0.5, 0.25])[0] and to_coco([], [], [], []) == []
    for args in ((rows, [7], [3, 1], [0.5, 0.25]), (rows, [7, 9], [3], [0.5, 0.25]), (rows, [7, 9], [3, 1], [0.5])):
        with pytest.raises(ValueError):
            to_coco(*args)
    with pytest.raises(ValueError):
        to_coco(rows, [7, 9], [3, 1], [0.5, 0.25], boxes=[[1, 2, 3, 4]])
    # a MaskRle on the host goes through its own to_coco
    mp = maskpost()
    rle = mp.MaskRle(counts=torch.tensor([3, 2, 15, 0, 4], dtype=torch.int32), offsets=torch.tensor([0, 3, 5]), n_runs=torch.tensor([3, 2], dtype=torch.int32),
                     size=None, sizes=[(4, 5), (2, 2)])
    assert [d["segmentation"] for d in to_coco(rle, [7, 9], [3, 1], [0.5, 0.25])] == rows


def test_the_abi_is_still_12_and_exports_the_new_entries():
    h = hip()
    assert h.load().cvlm_abi_version() == 12 == h.ABI_VERSION
    for name in ("cvlm_mask_regions_workspace_bytes", "cvlm_mask_regions_sized", "cvlm_debug_mask_regions_sized_host", "cvlm_region_alpha",
                 "cvlm_debug_region_alpha_host"):
        assert name in h.EXPORTS and isinstance(getattr(h.load(), name), ctypes._CFuncPtr)
