"""Thinning of sized planes without a device: the two forms of the oracle (tests/thin_oracle.py) against each other, the
known answers, the properties -- subset, idempotence, the 8-connected component count, max_iter, resume --, the sequential host entry
cvlm_debug_mask_thin_sized_host against the oracle on the whole list of the device tests, cvlm_mask_thin_resident on both sides of the
budget, every refusal, CVLM_E_BADARG and CVLM_E_WORKSPACE, every ValueError of the request with the launchers replaced by a recorder,
and surfeval.cldice for every combination of empty and non-empty.  Every comparison is exact."""
import ctypes
import math

import numpy as np
import pytest
import torch

import boundary_oracle as BO
import thin_oracle as TO


def host_entry():
    from camouflaged_vlm_amd import hip
    return hip.mask_thin_sized_host


_CACHE = {}


def gpu_list():
    """(planes, max_iters, the oracle's (plane, iters) of each), computed once and left unchanged."""
    if "list" not in _CACHE:
        planes, max_iters = TO.gpu_list()
        _CACHE["list"] = (planes, max_iters, [TO.thin(p, m) for p, m in zip(planes, max_iters)])
    return _CACHE["list"]


def random_planes(n: int, seed: int):
    """n planes at the issue's heights 1, 2, 33, 130 x widths 1 .. 129 and six densities, in turn."""
    rng = np.random.default_rng(seed)
    shapes = [(h, w) for h in (1, 2, 33, 130) for w in TO.WIDTHS]
    dens = (0.1, 0.3, 0.5, 0.7, 0.9, 0.98)
    return [rng.random(shapes[i % len(shapes)]) < dens[(i // len(shapes) + i) % 6] for i in range(n)]


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------------------
def test_the_two_forms_of_the_oracle_agree_on_150_planes():
    pytest.importorskip("scipy.ndimage")
    for i, x in enumerate(random_planes(150, 41)):
        m = (0, 0, 1, 3)[i % 4]
        a, na = TO.thin(x, m)
        b, nb = TO.thin_lut(x, m)
        assert np.array_equal(a, b) and na == nb, (i, x.shape, m)
    assert TO.lut(False).sum() > 0 and not np.array_equal(TO.lut(False), TO.lut(True))


def test_the_known_answers():
    full = lambda h, w: np.ones((h, w), dtype=bool)
    r, n = TO.thin(full(2, 2))
    assert np.argwhere(r).tolist() == [[1, 0]] and n == 1
    r, n = TO.thin(full(3, 3))
    assert np.argwhere(r).tolist() == [[1, 1]] and n == 1
    r, n = TO.thin(full(4, 6))
    assert np.argwhere(r).tolist() == [[2, 1], [2, 2], [2, 3]] and n == 2
    r, n = TO.thin(full(64, 64))
    assert int(r.sum()) == 1 and n == 32
    r, n = TO.thin(full(200, 300))
    assert int(r.sum()) == 101 and n == 100
    holed = full(20, 20)
    holed[8:12, 8:12] = False
    r, _ = TO.thin(holed)
    assert int(r.sum()) == 35
    pytest.importorskip("scipy.ndimage")
    from scipy import ndimage
    assert TO.components8(r) == 1 and ndimage.label(~r)[1] == 2        # one ring: the outside and one hole (4-connected background)
    assert TO.thin(np.zeros((5, 7), dtype=bool))[1] == 0 and TO.thin(r)[1] == 0                     # a fixed point takes 0 iterations


def test_subset_idempotence_and_components_on_every_test_plane():
    pytest.importorskip("scipy.ndimage")
    planes, max_iters, want = gpu_list()
    for i, (x, m, (r, n)) in enumerate(zip(planes, max_iters, want)):
        assert not (r & ~x).any(), i
        assert TO.components8(r) == TO.components8(x), (i, x.shape, m)
        if m == 0 or n < m:
            again, k = TO.thin(r)
            assert k == 0 and np.array_equal(again, r), i


def test_iterations_are_not_bounded_by_half_the_smaller_side():
    rng = np.random.default_rng(42)
    most = max(TO.thin(rng.random((33, 65)) < 0.9)[1] for _ in range(8))
    assert most > math.ceil(33 / 2), most


def test_max_iter_equals_that_many_iterations_and_resume():
    for i, x in enumerate(random_planes(32, 43)):
        full, n = TO.thin(x)
        step = x
        for m in range(1, 5):
            step = TO.iteration(step)
            got, k = TO.thin(x, m)
            assert np.array_equal(got, step) and k == min(m, n), (i, m)
            rest, more = TO.thin(got)
            assert np.array_equal(rest, full) and k + more == n, (i, m)


# ---- the host entry -----------------------------------------------------------------------------------------------------------------------------
def test_host_entry_equals_the_oracle_on_the_gpu_list():
    planes, max_iters, want = gpu_list()
    assert len(planes) == len(TO.WIDTHS) * len(TO.HEIGHTS) * len(TO.PATTERNS)
    res = TO.run(host_entry(), planes, max_iters)
    assert res["status"] == 0
    TO.check(res, planes, max_iters, want=want)
    bare = TO.run(host_entry(), planes[:60], max_iters[:60], stats=False, mode=1, steps=1)
    TO.check(bare, planes[:60], max_iters[:60], want=want[:60], stats=False)


def test_host_entry_on_the_known_answers():
    full = lambda h, w: np.ones((h, w), dtype=bool)
    planes = [full(2, 2), full(3, 3), full(4, 6), full(64, 64), full(200, 300)]
    res = TO.run(host_entry(), planes, [0] * 5)
    assert res["area"].tolist() == [1, 1, 3, 1, 101] and res["iters"].tolist() == [1, 1, 2, 32, 100] and res["done"].tolist() == [1] * 5
    assert res["box"][0].tolist() == [0, 1, 0, 1] and res["box"][2].tolist() == [1, 2, 3, 2]
    TO.check(res, planes, [0] * 5)


def ragged_planes(seed: int = 44):
    rng = np.random.default_rng(seed)
    return [rng.random(s) < d for s, d in zip(TO.RAGGED, (1.0, 0.9, 0.5, 0.98, 0.7, 0.9, 0.0))]


def test_host_entry_on_ragged_planes_used_outputs_dirty_pads_and_an_unaligned_base():
    fn = host_entry()
    planes, limits = ragged_planes(), [0, 1, 0, 2, 0, 0, 1]
    res = TO.run(fn, planes, limits)
    assert res["status"] == 0
    TO.check(res, planes, limits)
    other = [~p for p in planes]
    used = TO.run(fn, other, limits[::-1], outs=res["outs"])                              # other planes into used outputs and a used workspace
    assert used["status"] == 0
    TO.check(used, other, limits[::-1])
    dirty = TO.run(fn, planes, limits, shift=4, dirty_pads=True)                          # bits 4 bytes off a 16-byte boundary, pad bits set
    assert dirty["status"] == 0
    TO.check(dirty, planes, limits)


REFUSAL_SIZES = [(5, 40), (33, 65), (3, 7)]


def refusals():
    """(name, keywords of thin_oracle.run, max_iters, refused planes, untouched planes) on REFUSAL_SIZES: each kind of refused plane
    first, in the middle and last."""
    dims = np.asarray(REFUSAL_SIZES, dtype=np.int32)
    _, off, nbytes, _ = BO.tables(REFUSAL_SIZES)
    out = []
    for p, where in enumerate(("first", "middle", "last")):
        for kind, change in (("h = 0", (0, None)), ("w = 16385", (None, 16385)), ("a size that is not the slice's", (dims[p, 0] + 1, None))):
            d = dims.copy()
            d[p] = [d[p, 0] if change[0] is None else change[0], d[p, 1] if change[1] is None else change[1]]
            out.append((f"{kind}, {where}", dict(dims=d), [0, 0, 0], (p,), ()))
        for m in (-1, TO.MAX_ITER + 1):
            limits = [2, 0, 1]
            limits[p] = m
            out.append((f"max_iter {m}, {where}", {}, limits, (p,), ()))
    before, beyond, odd = off.copy(), off.copy(), off.copy()
    before[0] = -4
    beyond[3] = nbytes + 4
    odd[1] += 2
    out.append(("a slice that starts before the buffer", dict(offsets=before), [0, 0, 0], (), (0,)))
    out.append(("a slice that ends beyond the buffer", dict(offsets=beyond), [0, 0, 0], (), (2,)))
    out.append(("a seam off a word", dict(offsets=odd), [0, 0, 0], (), (0, 1)))
    return out


@pytest.mark.parametrize("name", [c[0] for c in refusals()])
def test_host_entry_refuses_whole_planes(name):
    _, kw, limits, refused, untouched = next(c for c in refusals() if c[0] == name)
    rng = np.random.default_rng(45)
    planes = [rng.random(s) < 0.8 for s in REFUSAL_SIZES]
    res = TO.run(host_entry(), planes, limits, **kw)
    assert res["status"] == 1
    TO.check(res, planes, limits, refused=refused, untouched=untouched)                   # the neighbours are whole


def test_resident_on_both_sides_of_the_budget():
    from camouflaged_vlm_amd import hip
    lib = hip.load()
    assert TO.lds_bytes(1024, 1024) == 139536 <= TO.LDS_BUDGET <= 160 * 1024
    assert lib.cvlm_mask_thin_resident(1024, 1024) == 1 and lib.cvlm_mask_thin_resident(1, 1) == 1
    h = TO.LDS_BUDGET // (4 * 34) - 2                                                    # the tallest plane of 1024 columns that fits
    assert TO.lds_bytes(h, 1024) <= TO.LDS_BUDGET < TO.lds_bytes(h + 1, 1024)
    assert lib.cvlm_mask_thin_resident(h, 1024) == 1 and lib.cvlm_mask_thin_resident(h + 1, 1024) == 0
    assert lib.cvlm_mask_thin_resident(h, 993) == 1 and lib.cvlm_mask_thin_resident(h, 1025) == 0
    assert lib.cvlm_mask_thin_resident(16384, 16384) == 0
    for bad in ((0, 5), (5, 0), (16385, 1), (1, 16385), (-1, -1)):
        assert lib.cvlm_mask_thin_resident(*bad) == 0, bad
    for hh, ww in ((1, 16384), (16384, 1), (480, 640), (1144, 1024), (1145, 1024)):
        assert hip.mask_thin_resident(hh, ww) == (TO.lds_bytes(hh, ww) <= TO.LDS_BUDGET), (hh, ww)


# ---- CVLM_E_BADARG, CVLM_E_WORKSPACE and the exports ------------------------------------------------------------------------------------------
def test_every_badarg_of_the_thin_entry():
    from camouflaged_vlm_amd import hip
    lib = hip.load()
    sizes = [(5, 40), (3, 7)]
    dims, off, nbytes, max_words = BO.tables(sizes, guard=0)
    steps = 3
    need = TO.ws_need(nbytes, 2, steps)
    assert lib.cvlm_mask_thin_workspace_bytes(nbytes, 2, steps) == need and lib.cvlm_mask_thin_workspace_bytes(4, 1, 0) == 16
    assert lib.cvlm_mask_thin_workspace_bytes(100, 3, 1024) == 112 + 12288
    for bad in ((3, 1, 1), (100, 0, 1), (100, 65536, 1), (100, 1, -1), (100, 1, 1025)):
        assert lib.cvlm_mask_thin_workspace_bytes(*bad) == -1, bad
    room = (nbytes + 15) // 16 * 16
    big = torch.zeros(2 * room + need + 64, dtype=torch.uint8)
    tab = lambda n: torch.zeros(n, dtype=torch.int32)
    keep = dict(big=big, offsets=torch.from_numpy(off), dims=torch.from_numpy(dims), max_iter=tab(3), area=tab(3), box=tab(9), iters=tab(3),
                done=tab(3), status=tab(2))
    base = big.data_ptr()
    assert base % 16 == 0
    good = dict(bits=base, n_bytes=nbytes, offsets=keep["offsets"].data_ptr(), dims=keep["dims"].data_ptr(), max_iter=keep["max_iter"].data_ptr(),
                P=2, max_words=max_words, mode=0, steps=steps, workspace=base + room, ws_bytes=need, out_bits=base + room + need,
                out_area=keep["area"].data_ptr(), out_box=keep["box"].data_ptr(), out_iters=keep["iters"].data_ptr(),
                out_done=keep["done"].data_ptr(), status=keep["status"].data_ptr())
    order = list(good)

    def call(dev: bool, **change):
        args = [dict(good, **change)[k] for k in order]
        return lib.cvlm_mask_thin_sized(*args, None) if dev else lib.cvlm_debug_mask_thin_sized_host(*args)

    assert call(False) == 0 and call(False, out_area=None, out_box=None) == 0 and call(False, mode=1) == 0
    bad = [{k: None} for k in ("bits", "offsets", "dims", "max_iter", "workspace", "out_bits", "out_iters", "out_done", "status")]
    bad += [dict(out_area=None), dict(out_box=None)]                  # both or neither
    bad += [{k: good[k] + 2} for k in ("bits", "dims", "max_iter", "out_bits", "out_area", "out_box", "out_iters", "out_done", "status")]
    bad += [dict(offsets=good["offsets"] + 4), dict(workspace=good["workspace"] + 8)]
    bad += [dict(P=0), dict(P=65536), dict(n_bytes=3), dict(max_words=0), dict(max_words=16384 * 512 + 1), dict(mode=-1), dict(mode=2),
            dict(steps=-1), dict(steps=1025), dict(mode=1, steps=0), dict(max_words=16384 * 512, steps=0)]
    bad += [dict(out_bits=base), dict(out_bits=base + nbytes - 4), dict(workspace=base), dict(out_bits=good["workspace"]),
            dict(out_bits=good["workspace"] + need - 4), dict(status=good["out_bits"]), dict(status=good["workspace"]),
            dict(out_bits=good["dims"]), dict(workspace=base + 16), dict(out_iters=good["out_done"]), dict(out_area=good["out_box"] + 4),
            dict(out_done=good["max_iter"]), dict(out_box=good["out_bits"]), dict(status=good["out_iters"] + 4)]
    for change in bad:
        for dev in (False, True):                                     # refused before the device is touched: no GPU is needed
            assert call(dev, **change) == -1, change
    for dev in (False, True):
        assert call(dev, ws_bytes=need - 16) == -3 and call(dev, ws_bytes=0) == -3      # CVLM_E_WORKSPACE
    assert call(False, steps=0, ws_bytes=room) == 0                   # a call of resident planes needs no flags


def test_exports_stay_at_abi_12():
    from camouflaged_vlm_amd import hip
    lib = hip.load()
    assert lib.cvlm_abi_version() == hip.ABI_VERSION == 12
    names = ("cvlm_mask_thin_sized", "cvlm_debug_mask_thin_sized_host", "cvlm_mask_thin_resident")
    for name in names:
        assert name in hip.EXPORTS and hasattr(lib, name) and hip.ABI[name][0] is ctypes.c_int32
    assert "cvlm_mask_thin_workspace_bytes" in hip.EXPORTS and hip.ABI["cvlm_mask_thin_workspace_bytes"][0] is ctypes.c_int64
    assert {n for n in names if n in hip._STREAMED} == {"cvlm_mask_thin_sized"}
    assert hip.THIN_MAX_ITER == TO.MAX_ITER and hip.THIN_MAX_STEPS == TO.MAX_STEPS


# ---- thin_request -------------------------------------------------------------------------------------------------------------------------------
SIZES = [(480, 640), (100, 75), (1, 1)]

BAD_THIN = {
    "no planes": dict(sizes=[]),
    "too many planes": dict(sizes=[(1, 1)] * 65536),
    "sizes a string": dict(sizes="480x640"),
    "a size of three": dict(sizes=[(480, 640, 3)]),
    "a side zero": dict(sizes=[(0, 640)]),
    "a side 16385": dict(sizes=[(480, 16385)]),
    "a side a bool": dict(sizes=[(True, 640)]),
    "a side a float": dict(sizes=[(480.0, 640)]),
    "max_iter zero": dict(max_iter=0),
    "max_iter negative": dict(max_iter=-1),
    "max_iter beyond 2^30": dict(max_iter=(1 << 30) + 1),
    "max_iter a bool": dict(max_iter=True),
    "max_iter a float": dict(max_iter=3.0),
    "max_iter a string": dict(max_iter="inf"),
    "max_iters too short": dict(max_iter=[1, 2]),
    "one max_iter a bool": dict(max_iter=[1, False, 3]),
    "one max_iter zero": dict(max_iter=[1, 0, 3]),
    "one max_iter None": dict(max_iter=[1, None, 3]),
    "path another string": dict(path="resident"),
    "path a bool": dict(path=True),
    "path None": dict(path=None),
    "steps zero": dict(steps=0),
    "steps 1025": dict(steps=1025),
    "steps a bool": dict(steps=True),
    "steps a float": dict(steps=64.0),
    "steps None": dict(steps=None),
}


@pytest.fixture
def launches(monkeypatch):
    """Every launcher the thinning calls could reach, replaced by a recorder."""
    from camouflaged_vlm_amd import hip
    seen = []
    for name in ("mask_thin_sized", "mask_thin_sized_host", "mask_inter_sized", "mask_inter_sized_host"):
        monkeypatch.setattr(hip, name, lambda *a, _n=name, **k: seen.append(_n))
    return seen


@pytest.mark.parametrize("name", list(BAD_THIN))
def test_bad_thin_requests_raise_and_launch_nothing(name, launches):
    from camouflaged_vlm_amd import engine
    for who in ("mask_thin_sized", "somebody"):
        kw = dict(dict(sizes=SIZES), **BAD_THIN[name])
        with pytest.raises(ValueError, match=who):
            engine.thin_request(kw.pop("sizes"), who=who, **kw)
    assert launches == []


def test_bad_arguments_of_the_cascade_calls_raise_and_launch_nothing(launches):
    from camouflaged_vlm_amd import engine
    util = object.__new__(engine.MaskUtilities)
    for bad in (None, torch.zeros(4, dtype=torch.uint8), SIZES):
        with pytest.raises(ValueError, match="mask_thin_sized"):
            engine.MaskUtilities.mask_thin_sized(util, bad)
        with pytest.raises(ValueError, match="mask_cldice"):
            engine.MaskUtilities.mask_cldice(util, bad, bad)
    assert launches == []


def test_request_tables(launches):
    from camouflaged_vlm_amd import engine
    sizes, limits, mode, steps = engine.thin_request(SIZES)
    assert sizes == SIZES and limits.dtype == np.int32 and limits.tolist() == [0, 0, 0] and (mode, steps) == (0, 64)
    sizes, limits, mode, steps = engine.thin_request([(np.int64(3), 4)] * 2, max_iter=np.int32(7))
    assert sizes == [(3, 4)] * 2 and limits.tolist() == [7, 7]
    _, limits, mode, steps = engine.thin_request(SIZES, max_iter=[1, 1 << 30, 5], path="steps", steps=1024)
    assert limits.tolist() == [1, 1 << 30, 5] and (mode, steps) == (1, 1024)
    assert engine.THIN_MAX_ITER == TO.MAX_ITER and engine.THIN_MAX_STEPS == TO.MAX_STEPS
    assert launches == []


# ---- clDice -------------------------------------------------------------------------------------------------------------------------------------
def test_surfeval_cldice_for_every_combination_of_empty_and_non_empty():
    from camouflaged_vlm_amd import surfeval
    limb, cut = TO.limb_planes()
    empty = np.zeros_like(limb)
    apart = np.zeros_like(limb)
    apart[45:47, 0:8] = True                                          # shares no pixel with either
    pairs = [(limb, limb), (limb, cut), (cut, limb), (empty, empty), (empty, limb), (limb, empty), (limb, apart)]
    counts = [TO.cldice_counts(a, b) for a, b in pairs]
    host = {k: np.asarray([c[k] for c in counts], dtype=np.int32) for k in counts[0]}
    got = surfeval.cldice(host)
    assert got["cldice"].dtype == np.float64
    want = [TO.cldice(c) for c in counts]
    assert got["cldice"].tolist() == want
    assert want[0] == 1.0 and want[3] == 1.0 and want[4] == want[5] == want[6] == 0.0 and 0.0 < want[1] == want[2] < 1.0
    assert got["tprec"][1] < 1.0 and got["tsens"][1] == 1.0          # the leg's centre line is missed, the rest lies inside
    dice = 2 * (limb & cut).sum() / (limb.sum() + cut.sum())
    assert want[1] < dice                                             # the missing limb costs clDice more than Dice
    refused = surfeval.cldice(dict(skel_a=[3, 3], skel_a_in_b=[-1, 2], skel_b=[4, 4], skel_b_in_a=[-1, 3]))
    assert np.isnan(refused["cldice"][0]) and np.isnan(refused["tprec"][0]) and refused["cldice"][1] == 2 * (2 / 3) * (3 / 4) / (2 / 3 + 3 / 4)
