"""CPU: mask NMS -- cvlm_debug_mask_nms_inter_host and cvlm_debug_mask_nms_host, the kernels' per-thread functions
(csrc/nms_logic.h) run sequentially, against the numpy oracle (tests/nms_oracle.py) on the one ragged scene; every CVLM_E_BADARG with
host pointers, each status refusal with its untouched rows, every ValueError of nms_request, select / rescored on host tensors."""
import ctypes

import numpy as np
import pytest
import torch

import nms_oracle as NO

COMBOS = [("iou", "greedy", False), ("iou", "greedy", True), ("min", "greedy", False), ("iou", "linear", False), ("min", "linear", True),
          ("iou", "gaussian", False), ("min", "gaussian", True)]


@pytest.fixture(scope="module")
def hip():
    from camouflaged_vlm_amd import hip
    hip.load()
    return hip


@pytest.fixture(scope="module")
def sc():
    return NO.scene()


@pytest.fixture(scope="module")
def host_inter(hip, sc):
    return NO.run_inter(hip, sc)


def test_abi_stays_12_and_the_entries_are_bound(hip):
    lib = hip.load()
    assert lib.cvlm_abi_version() == hip.ABI_VERSION == 12
    for name in ("cvlm_mask_nms_inter", "cvlm_debug_mask_nms_inter_host", "cvlm_mask_nms", "cvlm_debug_mask_nms_host"):
        assert name in hip.EXPORTS and hasattr(lib, name) and hip.ABI[name][0] is ctypes.c_int32
    assert hip._SIGNATURES["cvlm_mask_nms_inter"] == hip._SIGNATURES["cvlm_debug_mask_nms_inter_host"] + "s"
    assert hip._SIGNATURES["cvlm_mask_nms"] == hip._SIGNATURES["cvlm_debug_mask_nms_host"] + "s"


def test_inter_host_twin_equals_the_oracle(sc, host_inter):
    # the scene holds what DESIGN.md §30 lists
    sizes = set(sc["sizes"])
    assert {(1, 1), (1, 32), (5, 33), (7, 31), (3, 70), (40, 65), (16, 40), (8, 33)} <= sizes
    D = np.diff(sc["group_offsets"]).tolist()
    assert {1, 2, 3, 65, 257, 1024} <= set(D) and int(sc["pair_offsets"][-1]) >= 523776
    img = np.asarray(sc["image"])
    assert int((np.diff(img) != 0).sum()) > 100                       # the groups are interleaved in the planes' order
    assert bool(np.isnan(sc["scores"]).any()) and bool((sc["area"] == 0).any())
    assert host_inter["status"] == 0 and host_inter["bands"]
    assert np.array_equal(host_inter["inter"], sc["inter"])
    # the boxes meeting only in column 32, only in column 31 and only in row 3: one pixel column or row counted
    g2, g3 = sc["keys"].index(2), sc["keys"].index(3)
    tri = lambda g: sc["inter"][sc["pair_offsets"][g]:sc["pair_offsets"][g + 1]]
    rows2 = sc["member"][sc["group_offsets"][g2]:sc["group_offsets"][g2 + 1]].tolist()
    at = lambda rows, a, b: NO.pair_at(*sorted((rows.index(a), rows.index(b))), len(rows))
    r = [NO.row_of(sc, k) for k in (3, 4, 5)]
    assert tri(g2)[at(rows2, r[0], r[1])] == 3 and tri(g2)[at(rows2, r[1], r[2])] == 3 and tri(g2)[at(rows2, r[0], r[2])] == 0
    rows3 = sc["member"][sc["group_offsets"][g3]:sc["group_offsets"][g3 + 1]].tolist()
    assert tri(g3)[at(rows3, NO.row_of(sc, 8), NO.row_of(sc, 9))] == 11


@pytest.mark.parametrize("measure,method,class_aware", COMBOS)
def test_nms_host_twin_equals_the_oracle(hip, sc, measure, method, class_aware):
    want = NO.nms_oracle(sc, sc["inter"], measure=measure, method=method, class_aware=class_aware)
    got = NO.run_nms(hip, sc, sc["inter"], measure=measure, method=method, class_aware=class_aware)
    assert got["status"] == 0
    NO.same(got, want, method)
    if method == "greedy":
        assert 0 < int(got["keep"].sum()) < len(sc["area"]) and np.array_equal(got["decay"], got["keep"].astype(np.float32))
        assert bool((got["by"][got["keep"] == 1] == -1).all())
    else:
        assert np.array_equal(got["keep"], (sc["area"] >= 1).astype(np.uint8)) and bool((got["by"] == -1).all())
        assert bool(((got["decay"] >= 0) & (got["decay"] <= 1)).all()) and bool((got["decay"] < 1).any())


def test_the_greedy_cases(hip, sc):
    row = lambda k: NO.row_of(sc, k)
    run = lambda **kw: NO.run_nms(hip, sc, sc["inter"], **kw)
    at_half, below = run(thr=0.5), run(thr=NO.BELOW_HALF)
    # the exact tie: areas 1 and 2, inter 1: IoU == 0.5 survives thr 0.5 and falls at the next double below
    assert at_half["keep"][row(7)] == 1 and below["keep"][row(7)] == 0 and below["by"][row(7)] == row(6)
    # the chain: A suppresses B, and C survives only because B is gone
    a, b, c = row(10), row(11), row(12)
    assert at_half["keep"][[a, b, c]].tolist() == [1, 0, 1] and at_half["by"][b] == a and at_half["by"][c] == -1
    alone = dict(sc, area=sc["area"].copy())
    alone["area"][a] = 0                                              # without A, B is kept and does suppress C
    w = NO.run_nms(hip, alone, sc["inter"])
    assert w["keep"][[a, b, c]].tolist() == [0, 1, 0] and w["by"][c] == b
    # equal scores: the first in member order wins; an empty instance ranked first is not kept and suppresses nothing
    other_cat, nested, empty = (row(k) for k in (15, 16, 17))
    (big0, big1), (nan0, nan1) = sorted((row(13), row(14))), sorted((row(18), row(19)))       # the scene interleaves: member order is row order
    assert at_half["keep"][[big0, big1]].tolist() == [1, 0] and at_half["by"][big1] == big0
    assert at_half["keep"][empty] == 0 and at_half["by"][empty] == -1 and at_half["decay"][empty] == 0
    g5 = sc["keys"].index(5)
    order5 = at_half["order"][sc["group_offsets"][g5]:sc["group_offsets"][g5 + 1]].tolist()
    assert order5[0] == empty and order5[-2:] == [nan0, nan1]         # NaN behind every number, in member order
    assert at_half["keep"][[nan0, nan1]].tolist() == [1, 0] and at_half["by"][nan1] == nan0
    # identical masks of different categories: one falls class-agnostic, both stay class-aware
    assert at_half["keep"][other_cat] == 0 and run(class_aware=True)["keep"][other_cat] == 1
    # the nested blob: IoU keeps it, intersection over the smaller area does not
    assert at_half["keep"][nested] == 1
    m = run(measure="min")
    assert m["keep"][nested] == 0 and m["by"][nested] == big0
    # linear Matrix NMS with c = 1: the duplicate decays to 0, and what follows it is decayed by the original, never divided by 0
    lin = run(method="linear")
    assert lin["decay"][big0] == 1 and lin["decay"][big1] == 0 and np.isfinite(lin["decay"]).all()
    assert lin["decay"][nested] == np.float32(1.0 - 25.0 / 1500.0)


def test_the_boxes_restrict_the_count(hip):
    """A box smaller than the plane's pixels: only what lies inside both boxes is counted, and a pair of disjoint boxes is 0 whatever
    the planes hold."""
    planes = [np.ones((6, 70), bool)] * 3
    dims, off = NO.tables([p.shape for p in planes])
    sc = dict(bits=np.concatenate([NO.pack_rows(p, dirty=True) for p in planes]), offsets=off, dims=dims, area=np.full(3, 420, np.int32),
              box=np.asarray([[0, 0, 69, 5], [30, 2, 33, 3], [40, 0, 69, 5]], np.int32), group_offsets=np.asarray([0, 3], np.int32),
              member=np.arange(3, dtype=np.int32), pair_offsets=np.asarray([0, 3], np.int64))
    got = NO.run_inter(hip, sc)
    assert got["inter"].tolist() == [8, 180, 0] and got["status"] == 0 and got["bands"]
    assert NO.inter_oracle(sc).tolist() == [8, 180, 0]


def _small():
    planes = [NO.rect(5, 33, 0, 4, 0, 32), NO.rect(5, 33, 1, 3, 20, 32), NO.rect(5, 33, 0, 2, 0, 10), NO.rect(4, 40, 0, 3, 0, 39),
              NO.rect(4, 40, 1, 2, 5, 35)]
    dims, off = NO.tables([p.shape for p in planes])
    st = [NO.stats(p) for p in planes]
    keys, member, goff, poff = NO.groups_of([0, 0, 0, 1, 1])
    sc = dict(bits=np.concatenate([NO.pack_rows(p) for p in planes]), offsets=off, dims=dims, area=np.asarray([s[0] for s in st], np.int32),
              box=np.asarray([s[1] for s in st], np.int32), group_offsets=goff, member=member, pair_offsets=poff, keys=keys,
              scores=np.asarray([0.9, 0.8, 0.7, 0.6, 0.5], np.float32), category=np.zeros(5, np.int32))
    sc["inter"] = NO.inter_oracle(sc)
    return sc


def test_pair_refusals_leave_the_other_pairs(hip):
    sc = _small()
    assert sc["inter"].tolist() == [39, 33, 0, 62]
    cases = []
    for at in (0, 1, 2):                                              # the first, a middle and the last plane of the group
        box = sc["box"].copy(); box[at] = [5, 0, 4, 2]; cases.append(dict(box=box))                       # x0 > x1
        box = sc["box"].copy(); box[at, 2] = 33; cases.append(dict(box=box))                              # leaves [0, w)
        box = sc["box"].copy(); box[at] = [-1, -1, -1, 0]; cases.append(dict(box=box))                    # not the empty box
        dims = sc["dims"].copy(); dims[at] = (5, 34); cases.append(dict(dims=dims))                       # another size
        off = sc["offsets"].copy(); off[at] += 4 if at else -4; cases.append(dict(offsets=off))           # a slice that is not the plane's
    for over in cases:
        got = NO.run_inter(hip, sc, **over)
        assert got["status"] == 1 and got["bands"] and bool((got["inter"][:3] == -1).any())
        assert got["inter"][3] == 62 and all(v in (-1, w) for v, w in zip(got["inter"][:3], sc["inter"][:3]))
    nms = NO.run_nms(hip, sc, np.asarray([-1, 33, -1, 62], np.int32), thr=0.1)
    assert nms["status"] == 0 and nms["keep"].tolist() == [1, 1, 0, 1, 0] and nms["by"].tolist() == [-1, -1, 0, -1, 3]    # a refused pair suppresses nothing
    lin = NO.run_nms(hip, sc, np.asarray([-1, 33, -1, 62], np.int32), method="linear")
    assert lin["decay"][1] == 1                                       # Matrix NMS takes it as 0


def test_group_refusals_leave_their_rows_untouched(hip):
    sc = _small()
    want = NO.nms_oracle(sc, sc["inter"])
    i32, i64 = (lambda *v: np.asarray(v, np.int32)), (lambda *v: np.asarray(v, np.int64))
    cases = [(dict(group_offsets=i32(3, 0, 5)), {0, 1}),              # backwards; and five rows for a block of one pair
             (dict(group_offsets=i32(0, 3, 6)), {1}),                 # past the Q rows
             (dict(member=i32(0, 1, 2, 3, 5)), {1}), (dict(member=i32(0, 1, 2, -1, 4)), {1}),
             (dict(pair_offsets=i64(0, 3, 5)), {1}),                  # not the triangle
             (dict(pair_offsets=i64(0, 3, 2)), {1}),                  # backwards
             (dict(pair_offsets=i64(-3, 0, 1)), {0}),                 # before the table; image 1 takes the block at 0
             (dict(pair_offsets=i64(4, 7, 8)), {0, 1})]               # behind it
    for over, refused in cases:
        i = NO.run_inter(hip, sc, **over)
        n = NO.run_nms(hip, sc, sc["inter"], **over)
        assert i["status"] == 2 and n["status"] == 2 and i["bands"], over
        for g, rows in enumerate(([0, 1, 2], [3, 4])):
            if g not in refused:
                assert n["keep"][rows].tolist() == want["keep"][rows].tolist() and n["by"][rows].tolist() == want["by"][rows].tolist()
                assert n["n_keep"][g] == want["n_keep"][g]
            else:
                assert n["keep"][rows].tolist() == [0] * len(rows) and n["by"][rows].tolist() == [-1] * len(rows)
                assert n["decay"][rows].tolist() == [0.0] * len(rows) and n["n_keep"][g] == 0
        assert bool(np.isin(i["inter"], [-1] + sc["inter"].tolist()).all()) and bool((i["inter"] == -1).any())     # counts where a group was taken
    Q = 1100                                                          # the cap: D = 1024 is taken, 1025 is not
    dims, off = NO.tables([(1, 1)] * Q)
    cap = dict(bits=np.zeros(4 * Q, np.uint8), offsets=off, dims=dims, area=np.zeros(Q, np.int32), box=np.full((Q, 4), -1, np.int32),
               member=np.arange(Q, dtype=np.int32), scores=np.zeros(Q, np.float32), category=np.zeros(Q, np.int32))
    for D, status in ((1024, 0), (1025, 2)):
        t = dict(cap, group_offsets=np.asarray([0, D], np.int32), pair_offsets=np.asarray([0, D * (D - 1) // 2], np.int64))
        i = NO.run_inter(hip, t)
        assert i["status"] == status and bool((i["inter"] == (0 if status == 0 else -1)).all())
        n = NO.run_nms(hip, t, i["inter"])
        assert n["status"] == status and bool((n["order"][:D] == (np.arange(D) if status == 0 else -1)).all())


def test_every_badarg_with_host_pointers(hip):
    lib, BAD = hip.load(), -1
    sc = _small()
    Q, G, N = 5, 2, 4
    t = {k: np.ascontiguousarray(v) for k, v in sc.items() if isinstance(v, np.ndarray)}
    inter, status = np.zeros(N + 2, np.int32), np.zeros(3, np.int32)
    order, by, n_keep = np.zeros(Q + 1, np.int32), np.zeros(Q + 1, np.int32), np.zeros(G + 1, np.int32)
    keep, decay = np.zeros(Q + 4, np.uint8), np.zeros(Q + 1, np.float32)
    params = np.asarray([0.5, 2.0, 0.0])
    p = lambda a, shift=0: a.ctypes.data + shift

    def inter_call(**o):
        a = dict(bits=p(t["bits"]), n_bytes=t["bits"].size, offsets=p(t["offsets"]), dims=p(t["dims"]), area=p(t["area"]), box=p(t["box"]), Q=Q,
                 group_offsets=p(t["group_offsets"]), member=p(t["member"]), pair_offsets=p(t["pair_offsets"]), G=G, N=N, inter=p(inter),
                 status=p(status))
        a.update(o)
        return lib.cvlm_debug_mask_nms_inter_host(*a.values())

    def nms_call(**o):
        a = dict(group_offsets=p(t["group_offsets"]), member=p(t["member"]), pair_offsets=p(t["pair_offsets"]), G=G, inter=p(t["inter"]), N=N,
                 area=p(t["area"]), score=p(t["scores"]), category=p(t["category"]), Q=Q, measure=0, method=0, params=p(params), order=p(order),
                 keep=p(keep), by=p(by), decay=p(decay), n_keep=p(n_keep), status=p(status))
        a.update(o)
        return lib.cvlm_debug_mask_nms_host(*a.values())

    assert BAD == -1 and inter_call() == 0 and nms_call() == 0 and nms_call(category=None) == 0
    assert inter_call(N=0, inter=None, pair_offsets=p(np.zeros(3, np.int64)), group_offsets=p(np.asarray([0, 1, 2], np.int32))) == 0
    for name in ("bits", "offsets", "dims", "area", "box", "group_offsets", "member", "pair_offsets", "inter", "status"):
        assert inter_call(**{name: None}) != 0, name
    for name in ("dims", "area", "box", "group_offsets", "member", "inter", "status"):
        assert inter_call(**{name: p(np.zeros(64, np.int32), 2)}) != 0, name
    for name in ("offsets", "pair_offsets"):
        assert inter_call(**{name: p(np.zeros(64, np.int64), 4)}) != 0, name
    assert inter_call(bits=p(t["bits"], 1)) != 0
    for o in (dict(Q=0), dict(Q=(1 << 20) + 1), dict(G=0), dict(G=(1 << 20) + 1), dict(N=-1), dict(N=(1 << 22) + 1), dict(n_bytes=3),
              dict(inter=p(t["area"])), dict(status=p(t["box"], 8)), dict(inter=p(status)), dict(status=p(inter, 4)),
              dict(inter=p(t["bits"])), dict(status=p(t["pair_offsets"], 8))):
        assert inter_call(**o) != 0, o
    for name in ("group_offsets", "member", "pair_offsets", "inter", "area", "score", "params", "order", "keep", "by", "decay", "n_keep", "status"):
        assert nms_call(**{name: None}) != 0, name
    for name in ("group_offsets", "member", "inter", "area", "score", "category", "order", "by", "decay", "n_keep", "status"):
        assert nms_call(**{name: p(np.zeros(64, np.int32), 2)}) != 0, name
    for name in ("pair_offsets", "params"):
        assert nms_call(**{name: p(np.zeros(64, np.int64), 4)}) != 0, name
    nan, inf = float("nan"), float("inf")
    P = lambda *v: p(np.asarray(v, np.float64).copy())
    keepalive = [np.asarray(v, np.float64) for v in ((-1e-9, 2.0), (1.0000001, 2.0), (nan, 2.0), (0.5, 0.0), (0.5, -1.0), (0.5, nan), (0.5, inf))]
    for k, arr in enumerate(keepalive):
        assert nms_call(params=p(arr), method=2) != 0, arr
        assert (nms_call(params=p(arr), method=0) != 0) == (k < 3), arr       # sigma is the gaussian's alone
    for o in (dict(Q=0), dict(Q=(1 << 20) + 1), dict(G=0), dict(G=(1 << 20) + 1), dict(N=-1), dict(N=(1 << 22) + 1), dict(measure=2),
              dict(measure=-1), dict(method=3), dict(method=-1),
              dict(order=p(by)), dict(keep=p(decay).__add__(1)), dict(by=p(t["area"])), dict(decay=p(t["scores"])), dict(n_keep=p(t["inter"])),
              dict(status=p(order, 4)), dict(order=p(t["member"])), dict(keep=p(t["category"]))):
        assert nms_call(**o) != 0, o
    assert nms_call(params=P(0.0, 2.0)) == 0 and nms_call(params=P(1.0, 2.0)) == 0


def test_every_value_error_of_nms_request():
    from camouflaged_vlm_amd import maskpost
    ok = maskpost.nms_request([(4, 5)] * 3 + [(2, 2)], image=[7, 3, 7, 5], iou=0.3, measure="min", method="gaussian", sigma=1.5)
    assert ok.keys == [3, 5, 7] and ok.member.tolist() == [1, 3, 0, 2] and ok.group_offsets.tolist() == [0, 1, 2, 4]
    assert ok.pair_offsets.tolist() == [0, 0, 0, 1] and ok.n_pairs == 1 and (ok.thr, ok.measure, ok.method, ok.sigma) == (0.3, 1, 2, 1.5)
    assert ok.member.dtype == np.int32 and ok.group_offsets.dtype == np.int32 and ok.pair_offsets.dtype == np.int64
    S = [(4, 5)] * 3
    bad = [dict(sizes=[], image=[]), dict(sizes=S, image=[0, 0]), dict(sizes=S, image=[0, 0, 0.0]), dict(sizes=S, image=[0, 0, True]),
           dict(sizes=S, image="abc"), dict(sizes=S, image=5), dict(sizes=[(4, 5), (4, 6), (4, 5)], image=[0, 0, 1]),
           dict(sizes=[(4, 5), (0, 6), (4, 5)], image=[0, 1, 2]), dict(sizes=[(4, 5), (True, 6), (4, 5)], image=[0, 1, 2]),
           dict(sizes=[(4, 5)] * 1025, image=[0] * 1025), dict(sizes=[(4, 5)] * 9000, image=[k // 1000 for k in range(9000)]),
           dict(sizes=S, image=[0, 0, 0], iou=-0.1), dict(sizes=S, image=[0, 0, 0], iou=1.5), dict(sizes=S, image=[0, 0, 0], iou=float("nan")),
           dict(sizes=S, image=[0, 0, 0], iou=True), dict(sizes=S, image=[0, 0, 0], iou="0.5"), dict(sizes=S, image=[0, 0, 0], measure="dice"),
           dict(sizes=S, image=[0, 0, 0], measure=0), dict(sizes=S, image=[0, 0, 0], method="soft"), dict(sizes=S, image=[0, 0, 0], method=1),
           dict(sizes=S, image=[0, 0, 0], sigma=0), dict(sizes=S, image=[0, 0, 0], sigma=-1.0), dict(sizes=S, image=[0, 0, 0], sigma=float("inf")),
           dict(sizes=S, image=[0, 0, 0], sigma=True)]
    for kw in bad:
        sizes = kw.pop("sizes")
        with pytest.raises(ValueError):
            maskpost.nms_request(sizes, **kw)
    assert maskpost.nms_request([(1, 1)] * 1024, image=[0] * 1024).n_pairs == 523776
    assert maskpost.nms_request([(1, 1)] * 8192, image=[k // 1024 for k in range(8192)]).n_pairs == 8 * 523776 <= maskpost.NMS_MAX_PAIRS


def test_select_and_rescored_on_host_tensors():
    from camouflaged_vlm_amd import maskpost
    planes = [NO.rect(3, 40, 0, 1, 0, 9), NO.rect(5, 33, 1, 2, 3, 32), NO.rect(5, 33, 0, 4, 0, 0), NO.rect(3, 40, 2, 2, 35, 39), NO.rect(2, 2, 0, 0, 0, 0)]
    sizes = [p.shape for p in planes]
    _, off = NO.tables(sizes)
    st = [NO.stats(p) for p in planes]
    T = torch.from_numpy
    inst = maskpost.SizedMasks(bits=T(np.concatenate([NO.pack_rows(p) for p in planes])), offsets=T(off), area=T(np.asarray([s[0] for s in st], np.int32)),
                               box=T(np.asarray([s[1] for s in st], np.int32)), status=torch.zeros(1, dtype=torch.int32), sizes=sizes)
    res = maskpost.MaskNms(keep=T(np.asarray([0, 1, 1, 0, 1], np.uint8)), by=T(np.asarray([1, -1, -1, 2, -1], np.int32)),
                           decay=T(np.asarray([0, 1, 0.5, 0, 1], np.float32)), order=T(np.arange(5, dtype=np.int32)), n_keep=T(np.asarray([3], np.int32)),
                           inter=torch.zeros(0, dtype=torch.int32), status=torch.zeros(2, dtype=torch.int32))
    res.check()
    kept, idx = res.select(inst)
    assert idx.tolist() == [1, 2, 4] and idx.dtype == np.int64 and kept.sizes == [sizes[k] for k in idx]
    assert kept.offsets.tolist() == NO.tables(kept.sizes)[1].tolist() and kept.area.tolist() == [st[k][0] for k in idx]
    assert kept.box.tolist() == [list(st[k][1]) for k in idx]
    for n, k in enumerate(idx):
        assert np.array_equal(kept.to_numpy(n), planes[k])
    assert res.rescored([1.0, 0.5, 0.5, 2.0, 3.0]).tolist() == [0.0, 0.5, 0.25, 0.0, 3.0]
    assert res.rescored(torch.ones(5, dtype=torch.float64)).dtype == torch.float32
    none = maskpost.MaskNms(keep=torch.zeros(5, dtype=torch.uint8), by=res.by, decay=res.decay, order=res.order, n_keep=res.n_keep, inter=res.inter,
                            status=res.status)
    kept, idx = none.select(inst)
    assert idx.size == 0 and kept.sizes == [] and kept.bits.numel() == 0 and kept.offsets.tolist() == [0]
    for bad in (torch.tensor([1, 0], dtype=torch.int32), torch.tensor([0, 2], dtype=torch.int32)):
        refused = maskpost.MaskNms(keep=res.keep, by=res.by, decay=res.decay, order=res.order, n_keep=res.n_keep, inter=res.inter, status=bad)
        with pytest.raises(RuntimeError):
            refused.select(inst)
        with pytest.raises(RuntimeError):
            refused.check()
    with pytest.raises(ValueError):
        res.rescored([1.0, 2.0])
    with pytest.raises(ValueError):
        res.select(maskpost.SizedMasks(bits=inst.bits, offsets=inst.offsets, area=inst.area, box=inst.box, status=inst.status, sizes=sizes[:4]))
