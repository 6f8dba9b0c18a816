"""CPU: label maps -- the oracle (tests/labels_oracle.py: the published loops) on known answers; the host entries
cvlm_debug_label_*_host (the kernels' per-thread functions run sequentially on the CPU) against the oracle on exact and smooth inputs,
ragged images, every K, any cut into accumulate calls, every kind of weight, into sentinel-guarded outputs; the measured margin of the
one inexact comparison; the refusals of the entries (no GPU needed: they refuse before launching); the host checks
engine.labels_request, Cascade.label_maps and Cascade.label_iou with the launchers replaced by a recorder; segeval."""
import dataclasses

import numpy as np
import pytest
import torch

from camouflaged_vlm_amd import hip, segeval
from camouflaged_vlm_amd.engine import ClassHypotheses, LabelMaps, MaskUtilities, label_tables, labels_request
import labels_oracle as LO
import sized_oracle as SO


def plane(on: np.ndarray) -> np.ndarray:
    return np.where(on, np.float32(30), np.float32(-30)).astype(np.float32)


def columns(h: int, w: int, x0: int, x1: int) -> np.ndarray:
    on = np.zeros((h, w), bool)
    on[:, x0:x1] = True
    return plane(on)


# ---- known answers: the oracle and the host entry ----------------------------------------------------------------------------------------
def both(logits, sizes, weights=None, level=128, thr=0.8, cuts=None):
    """-> the host entries' outputs, which must be the oracle's on these exact inputs."""
    got = LO.run(logits, sizes, weights, level, thr, cuts=cuts)
    LO.compare(got, logits, sizes, weights, level, thr, exact=True)
    return got


def test_one_hypothesis_is_the_sized_mask():
    logits = LO.blocky(1, 1, 24, 40, 3)
    got = both(logits, [(33, 65)])
    bits, area = LO.sized_bits(logits, [(33, 65)])
    assert (got["winner"][0] == 0).all()
    assert np.array_equal(got["segment"][0] >= 0, bits[0][0]) and got["segment_id"].tolist() == [[1]] and got["n_segments"].tolist() == [1]
    assert got["won_area"][0, 0] == 33 * 65 and got["kept_area"][0, 0] == area[0, 0]
    # no set bit: the hypothesis still wins every pixel and is not kept
    empty = np.full((1, 1, 24, 40), -30, np.float32)
    got = both(empty, [(33, 65)])
    assert (got["winner"][0] == 0).all() and (got["segment"][0] == -1).all() and got["segment_id"].tolist() == [[0]]
    assert got["n_segments"].tolist() == [0] and got["orig_area"][0, 0] == 0 and got["won_area"][0, 0] == 33 * 65


def test_two_disjoint_masks_are_both_kept():
    logits = np.stack([columns(8, 16, 0, 8), columns(8, 16, 8, 16)])[None]
    got = both(logits, [(8, 16)])
    assert got["segment_id"].tolist() == [[1, 2]] and got["n_segments"].tolist() == [2]
    assert (got["segment"][0][:, :8] == 0).all() and (got["segment"][0][:, 8:] == 1).all()
    assert got["orig_area"].tolist() == got["won_area"].tolist() == got["kept_area"].tolist() == [[64, 64]]


def test_a_larger_mask_under_a_smaller_one_of_higher_weight():
    """8 x 16 at its own size.  Hypothesis 0: columns 0 .. 9 (80 pixels), weight 0.5; hypothesis 1: columns 6 .. 9 (32 pixels), weight 1.
    Columns 0 .. 5: s = (0.5, ~1e-13): 0 wins 48 pixels.  Columns 6 .. 9: s = (0.5, 1): 1 wins 32.  Columns 10 .. 15: both are off, s =
    (0.5 e, e) with e = sigmoid(-30): 1 wins 48 more, without its bit.  So 0 has won 48 of its original 80 -- 0.6: kept at 0.5, dropped
    at 0.8 --, and 1 has won 80, original 32, of which it holds 32: kept at both."""
    logits = np.stack([columns(8, 16, 0, 10), columns(8, 16, 6, 10)])[None]
    for thr, ids, n in ((0.5, [1, 2], 2), (0.8, [0, 1], 1), (0.6, [1, 2], 2)):          # 48 / 80 < 0.6 is false
        got = both(logits, [(8, 16)], [[0.5, 1.0]], thr=thr)
        assert got["orig_area"].tolist() == [[80, 32]] and got["won_area"].tolist() == [[48, 80]] and got["kept_area"].tolist() == [[48, 32]]
        assert got["segment_id"].tolist() == [ids] and got["n_segments"].tolist() == [n]
        seg = got["segment"][0]
        assert (seg[:, :6] == (0 if ids[0] else -1)).all() and (seg[:, 6:10] == 1).all() and (seg[:, 10:] == -1).all()
        assert (got["winner"][0][:, :6] == 0).all() and (got["winner"][0][:, 6:] == 1).all()


def test_equal_planes_of_equal_weight_go_to_the_smallest_k():
    one = SO.blocky(24, 40, 5)
    logits = np.stack([one, one, one])[None]
    for cuts in (None, [1], [2], [1, 2]):                             # also when the equal planes fall into different calls
        got = both(logits, [(33, 65)], [[0.5, 0.5, 0.5]], cuts=cuts)
        assert (got["winner"][0] == 0).all() and got["won_area"].tolist() == [[33 * 65, 0, 0]]
    got = both(logits, [(33, 65)], [[0.0, -0.0, 0.0]])               # +0 and -0 are equal
    assert (got["winner"][0] == 0).all()


def test_a_nan_plane_never_wins():
    nan = np.full((24, 40), np.nan, np.float32)
    logits = np.stack([nan, SO.blocky(24, 40, 6), nan])[None]
    got = both(logits, [(33, 65)], [[4.0, 0.25, 4.0]])
    assert (got["winner"][0] == 1).all() and got["orig_area"][0, 0] == 0 and got["segment_id"].tolist() == [[0, 1, 0]]
    # an image whose planes are all NaN: -1 everywhere, no segment; its neighbour is untouched by that
    logits = np.stack([np.stack([nan, nan]), LO.blocky(1, 2, 24, 40, 7)[0]])
    got = both(logits, [(5, 65), (33, 31)])
    assert (got["winner"][0] == -1).all() and (got["segment"][0] == -1).all() and got["n_segments"].tolist()[0] == 0
    assert got["won_area"][0].tolist() == [0, 0] and (got["winner"][1] >= 0).all()


# ---- the host entries against the oracle --------------------------------------------------------------------------------------------------
SOURCES = [(64, 64), (96, 128), (32, 64)]


def test_host_entry_is_exact_on_every_width_and_height():
    """Blocky +-30 planes with dyadic weights: widths around the unit of 64 pixels and its halves, heights 1, 2, 33, the three source
    sizes in turn, every pixel held."""
    i = 0
    for w in SO.GEOMETRY_WIDTHS:
        for h in SO.GEOMETRY_HEIGHTS:
            Hs, Ws = SOURCES[i % 3]
            logits = LO.blocky(1, 3, Hs, Ws, 100 * h + w)
            both(logits, [(h, w)], LO.dyadic(1, 3))
            i += 1


@pytest.mark.parametrize("src,dsts", [((64, 64), [(97, 131), (33, 31)]), ((96, 128), [(150, 201), (50, 70)]), ((32, 64), [(70, 133), (16, 20)])])
def test_host_entry_is_exact_enlarged_and_reduced(src, dsts):
    logits = LO.blocky(2, 4, *src, seed=src[0])
    both(logits, dsts, LO.dyadic(2, 4))
    both(logits, dsts, LO.dyadic(2, 4), level=1, thr=0.5)
    both(logits, dsts, None, level=255, thr=1.0)


@pytest.mark.parametrize("K", [1, 2, 5, 64, 65])
def test_ragged_images_in_one_call(K):
    logits = LO.blocky(7, K, 24, 40, 11 * K)
    both(logits, LO.RAGGED, LO.dyadic(7, K), thr=0.5)


def test_any_cut_into_calls_gives_the_same_outputs():
    """K = 3 over the seven ragged images, calls of 4 planes: a call crosses an image boundary, an image spans two or three calls."""
    logits = LO.blocky(7, 3, 24, 40, 77)
    wts = LO.dyadic(7, 3)
    whole = both(logits, LO.RAGGED, wts, thr=0.5)
    cut = both(logits, LO.RAGGED, wts, thr=0.5, cuts=list(range(4, 21, 4)))
    single = both(logits, LO.RAGGED, wts, thr=0.5, cuts=list(range(1, 21)))
    for other in (cut, single):
        for name, a in whole.items():
            b = other[name]
            same = all(np.array_equal(x, y) for x, y in zip(a, b)) if isinstance(a, list) else np.array_equal(a, b)
            assert same, name


@pytest.mark.parametrize("kind", ["null", "equal", "zero", "negative", "nan", "nan_all", "inf_planes"])
def test_weights_and_values(kind):
    logits = LO.blocky(2, 4, 24, 40, 21)
    sizes = [(33, 65), (70, 33)]
    wts = {"null": None, "equal": np.full((2, 4), 0.75), "zero": np.zeros((2, 4)), "negative": -LO.dyadic(2, 4),
           "nan": np.asarray([[1.0, np.nan, 0.5, np.nan], [np.nan, 2.0, 2.0, 0.25]]), "nan_all": np.full((2, 4), np.nan),
           "inf_planes": LO.dyadic(2, 4)}[kind]
    if kind == "inf_planes":
        logits = np.where(logits > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
    got = both(logits, sizes, wts, thr=0.5)
    if kind == "nan":
        assert not np.isin(got["winner"][0], (1, 3)).any() and not (got["winner"][1] == 0).any()
        assert got["won_area"][0, 1] == 0 and got["orig_area"][0, 1] > 0       # the bits of a hypothesis that takes no part still count
    if kind == "nan_all":
        assert all((wmap == -1).all() for wmap in got["winner"]) and got["n_segments"].tolist() == [0, 0]
    if kind == "negative":                                            # the largest s is the smallest |w| v: an off pixel of the largest weight
        assert got["status"] == 0 and all((wmap >= 0).all() for wmap in got["winner"])


def test_used_outputs_and_an_unaligned_base():
    """The whole sequence twice into the same outputs gives the same outputs; a logits base 4 bytes off a 16-byte boundary."""
    logits = LO.blocky(7, 2, 24, 40, 5)
    st = LO.State(LO.RAGGED, 2)
    first = LO.run(logits, LO.RAGGED, LO.dyadic(7, 2), state=st)
    other = LO.run(LO.blocky(7, 2, 24, 40, 6), LO.RAGGED, None, state=st)
    again = LO.run(logits, LO.RAGGED, LO.dyadic(7, 2), state=st)
    assert not np.array_equal(first["won_area"], other["won_area"])
    for name in ("winner", "segment", "score"):
        assert all(np.array_equal(a, b) for a, b in zip(first[name], again[name])), name
    for name in ("orig_area", "won_area", "kept_area", "segment_id", "n_segments"):
        assert np.array_equal(first[name], again[name]), name
    flat = torch.zeros(14 * 24 * 40 + 5, dtype=torch.float32)
    base = (-flat.data_ptr() // 4) % 4                               # element index of a 16-byte boundary
    off = flat[base + 1:base + 1 + 14 * 24 * 40].view(14, 24, 40)
    assert off.data_ptr() % 16 == 4
    off.copy_(torch.from_numpy(logits.reshape(14, 24, 40)))
    st.init()
    st.accumulate(off, 0, LO.dyadic(7, 2))
    st.finish()
    shifted = st.read()
    assert all(np.array_equal(a, b) for a, b in zip(first["winner"], shifted["winner"])) and np.array_equal(first["segment_id"], shifted["segment_id"])


def test_smooth_logits_within_the_measured_margin():
    """The margin of the one inexact comparison: LO.MEASURED bounds |s (float32 oracle) - s (fp64)| on these inputs, LO.MARGIN is five
    times that, and the host entry (the C library's expf) meets the oracle (numpy's) everywhere outside it."""
    worst = 0.0
    for logits, (h, w), wts in LO.smooth_cases():
        v = LO.values(logits[0], h, w)
        s32 = (wts[0][:, None, None] * v).astype(np.float32).astype(np.float64)
        worst = max(worst, float(np.abs(s32 - LO.scores_f64(logits[0], h, w, wts[0])).max()))
        got = LO.run(logits, [(h, w)], wts, overlap_threshold=0.5)
        LO.compare(got, logits, [(h, w)], wts, overlap_threshold=0.5)
    print(f"largest |fp32 - fp64| of s: {worst:.3e}; MEASURED {LO.MEASURED:.1e}, MARGIN {LO.MARGIN:.1e}")
    assert worst <= LO.MEASURED and LO.MARGIN == 5 * LO.MEASURED


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def refused(offsets=None, dims=None, n_pix=None):
    """The ragged call with image 2's table entry spoilt -> outputs; image 2 must stay at the fill, the others whole, status 1."""
    logits = LO.blocky(7, 2, 24, 40, 9)
    good = LO.run(logits, LO.RAGGED, LO.dyadic(7, 2), overlap_threshold=0.5)
    st = LO.State(LO.RAGGED, 2, n_pix=n_pix)
    d = st.dims if dims is None else torch.from_numpy(np.asarray(dims, np.int32))
    o = st.off if offsets is None else torch.from_numpy(np.asarray(offsets, np.int64))
    st.init()
    st.accumulate(torch.from_numpy(logits.reshape(14, 24, 40)), 0, LO.dyadic(7, 2), dims=d, off=o)
    st.finish(0.5, dims=d, off=o)
    return good, st


def test_a_refused_image_stays_at_the_fill_and_its_neighbours_whole():
    dims, off, _ = LO.tables(LO.RAGGED)
    cases = []
    bad = off.copy(); bad[3:] += 1                                   # image 2's slice one pixel longer than its size
    cases.append(dict(offsets=bad, skipped=(2,), n_pix=int(off[-1]) + 1))
    bad = off.copy(); bad[2] -= 1                                    # image 1 one short, image 2 one long
    cases.append(dict(offsets=bad, skipped=(1, 2)))
    for hw in ((0, 65), (5, 0), (-5, 65), (5, 16385), (2 ** 31 - 1, 2 ** 31 - 1)):
        d = dims.copy(); d[2] = hw
        cases.append(dict(dims=d, skipped=(2,)))
    cases.append(dict(n_pix=int(off[-1]) - 1, skipped=(6,)))        # the last image beyond the length of the maps
    bad = off.copy(); bad[0] = -1
    cases.append(dict(offsets=bad, skipped=(0,)))
    for case in cases:
        skipped = case.pop("skipped")
        good, st = refused(**case)
        used = np.asarray(case.get("offsets", off))                  # read the images where the call's own table puts them
        st.host_off = used
        got = st.read()
        assert got["status"] == 1, case
        for b in range(7):
            if b in skipped:
                lo, hi = max(int(used[b]), 0), min(int(used[b + 1]), st.n)
                assert (st.winner[lo:hi] == -1).all() and (st.segment[lo:hi] == -1).all() and (st.score[lo:hi] == 0).all(), (case, b)
                assert not got["orig_area"][b].any() and not got["won_area"][b].any() and not got["segment_id"][b].any()
                assert got["n_segments"][b] == 0
            else:
                assert np.array_equal(got["winner"][b], good["winner"][b]) and np.array_equal(got["segment"][b], good["segment"][b]), (case, b)
                assert np.array_equal(got["segment_id"][b], good["segment_id"][b]) and np.array_equal(got["orig_area"][b], good["orig_area"][b])
        # the lookup refuses the same image and writes nothing of it
        if "dims" in case:
            out = torch.full((st.n,), LO.FILL_I32, dtype=torch.int32)
            hip.label_lookup(st.winner, 7, 2, torch.from_numpy(case["dims"]), st.off, st.max_pixels, torch.arange(14, dtype=torch.int32), 255,
                             out, st.status, host=True)
            assert (out[int(off[2]):int(off[3])] == LO.FILL_I32).all() and (out[:int(off[2])] != LO.FILL_I32).all()


def test_label_entries_refuse_bad_arguments_without_gpu():
    import ctypes as C
    lib = hip.load()
    p = 1 << 20
    thr = C.c_double(0.8)
    tp = C.addressof(thr)
    ok = dict(logits=p, p0=0, p1=6, Hs=8, Ws=8, B=2, K=3, dims=p + 4096, off=p + 8192, wts=p + 12288, level=128, score=p + 16384,
              winner=p + 20480, segment=p + 24576, n_pix=100, max_pixels=64, areas=p + 28672, ids=p + 32768, nseg=p + 36864,
              status=p + 40960, thr=tp, table=p + 45056, out=p + 49152)
    common = [dict(dims=None), dict(off=None), dict(status=None), dict(dims=p + 4098), dict(off=p + 8196), dict(status=p + 40962),
              dict(B=0), dict(B=65536), dict(K=0), dict(K=16385), dict(n_pix=0), dict(max_pixels=0), dict(max_pixels=2 ** 28 + 1)]
    state = [dict(score=None), dict(winner=None), dict(segment=None), dict(areas=None), dict(score=p + 16386), dict(winner=p + 20481),
             dict(segment=p + 24577), dict(areas=p + 28674)]

    def call(name, k, host):
        fn = getattr(lib, ("cvlm_debug_" + name[5:] + "_host") if host else name)
        a = {"cvlm_label_init": ("score", "winner", "segment", "n_pix", "areas", "ids", "B", "K", "nseg", "status"),
             "cvlm_label_accumulate": ("logits", "p0", "p1", "Hs", "Ws", "B", "K", "dims", "off", "wts", "level", "score", "winner", "segment",
                                       "n_pix", "max_pixels", "areas", "status"),
             "cvlm_label_finish": ("B", "K", "dims", "off", "thr", "winner", "segment", "n_pix", "max_pixels", "areas", "ids", "nseg", "status"),
             "cvlm_label_lookup": ("winner", "B", "K", "dims", "off", "n_pix", "max_pixels", "table", "level", "out", "status")}[name]
        args = [k[n] for n in a]
        return fn(*args) if host else fn(*args, None)

    bad = {"cvlm_label_init": state + [dict(ids=None), dict(nseg=None), dict(status=None), dict(ids=p + 32770), dict(nseg=p + 36866),
                                       dict(B=0), dict(B=65536), dict(K=0), dict(K=16385), dict(n_pix=0)],
           "cvlm_label_accumulate": common + state + [dict(logits=None), dict(logits=p + 2), dict(wts=p + 12290), dict(Hs=0), dict(Ws=-1),
                                                      dict(Hs=2 ** 16, Ws=2 ** 15), dict(level=0), dict(level=256), dict(p0=-1),
                                                      dict(p0=6), dict(p0=3, p1=2), dict(p1=7)],
           "cvlm_label_finish": common + state[1:4] + state[5:] + [dict(ids=None), dict(nseg=None), dict(thr=None), dict(ids=p + 32770)],
           "cvlm_label_lookup": common + [dict(winner=None), dict(winner=p + 20481), dict(table=None), dict(out=None), dict(table=p + 45058),
                                          dict(out=p + 49154)]}
    for name, cases in bad.items():
        for kw in cases:
            for host in (False, True):
                assert call(name, dict(ok, **kw), host) == -1, (name, kw, host)
    for value in (float("nan"), 0.0, -0.5, 1.0000001, float("inf")):
        thr.value = value
        assert call("cvlm_label_finish", ok, False) == -1 and call("cvlm_label_finish", ok, True) == -1, value
    # weights may be NULL: the call passes the checks -- the host entry then runs, so it gets memory: one image of 2 x 3, one plane
    z = lambda n, dt: torch.zeros(n, dtype=dt)
    lg, dm, of = torch.full((4, 4), 30.0), torch.tensor([[2, 3]], dtype=torch.int32), torch.tensor([0, 6], dtype=torch.int64)
    sc, wi, sg, ar, st = z(6, torch.float32), torch.full((6,), -1, dtype=torch.int16), torch.full((6,), -1, dtype=torch.int16), z(3, torch.int32), z(1, torch.int32)
    assert lib.cvlm_debug_label_accumulate_host(lg.data_ptr(), 0, 1, 4, 4, 1, 1, dm.data_ptr(), of.data_ptr(), None, 128, sc.data_ptr(),
                                                wi.data_ptr(), sg.data_ptr(), 6, 6, ar.data_ptr(), st.data_ptr()) == 0
    assert wi.tolist() == [0] * 6 and sg.tolist() == [0] * 6 and sc.tolist() == [1.0] * 6 and ar.tolist() == [6, 0, 0] and st.item() == 0
    hk = dict(pred=p, gt=p + 4096, u8=0, n=10, C=3, ignore=255, reduce=0, zero=1, totals=p + 8192)
    for kw in (dict(pred=None), dict(gt=None), dict(totals=None), dict(pred=p + 2), dict(gt=p + 4098), dict(totals=p + 8196), dict(n=0),
               dict(C=0), dict(C=65537), dict(u8=2), dict(u8=-1)):
        k = dict(hk, **kw)
        args = [k[n] for n in ("pred", "gt", "u8", "n", "C", "ignore", "reduce", "zero", "totals")]
        assert lib.cvlm_label_iou_hist(*args, None) == -1 and lib.cvlm_debug_label_iou_hist_host(*args) == -1, kw


class Recorder:
    """Stands where the launchers stand and records what reaches them."""

    def __init__(self, monkeypatch):
        self.calls = []
        for name in ("label_init", "label_accumulate", "label_finish", "label_lookup", "label_iou_hist"):
            monkeypatch.setattr(hip, name, lambda *a, _n=name, **k: self.calls.append(_n))


def test_labels_request_raises_before_any_launch(monkeypatch):
    rec = Recorder(monkeypatch)
    ok = dict(label_maps=True, sizes=[(4, 5), (6, 7)], weights=None, level=128, overlap_threshold=0.8, n=2, K=3, masks="bits", who="caller")
    assert labels_request(**ok) == (None, 128, 0.8)
    w, _, _ = labels_request(**dict(ok, weights=[[1, 2, 3], [4, 5, 6]]))
    assert w.dtype == np.float32 and w.tolist() == [1, 2, 3, 4, 5, 6]
    assert labels_request(**dict(ok, label_maps=False)) is None
    bad = [dict(sizes=None), dict(masks="logits"), dict(K=16385), dict(K=0), dict(level=0), dict(level=256), dict(level=128.0), dict(level=True),
           dict(overlap_threshold=float("nan")), dict(overlap_threshold=0.0), dict(overlap_threshold=-1), dict(overlap_threshold=1.5),
           dict(overlap_threshold="0.8"), dict(overlap_threshold=None), dict(weights=[1.0, 2.0]), dict(weights=[[1, 2], [3, 4], [5, 6]]),
           dict(weights=[[1, 2, float("nan")], [4, 5, 6]]), dict(weights="abcdef"), dict(weights=torch.tensor([1.0, float("nan"), 1, 1, 1, 1])),
           dict(label_maps=1), dict(label_maps=False, weights=[1.0] * 6)]
    for kw in bad:
        with pytest.raises(ValueError, match="caller"):
            labels_request(**dict(ok, **kw))
    assert rec.calls == []


class Host(MaskUtilities):
    device = torch.device("cpu")


def test_label_maps_and_label_iou_raise_before_any_launch(monkeypatch):
    rec = Recorder(monkeypatch)
    eng = Host()
    logits = torch.zeros(6, 8, 8)
    sizes = [(4, 5), (6, 7)]
    bad = [dict(K=4), dict(K=0), dict(K=3.0), dict(sizes=[(4, 5)]), dict(sizes=None), dict(sizes=[(4, 5), (0, 7)]), dict(level=0),
           dict(overlap_threshold=0.0), dict(overlap_threshold=float("nan")), dict(weights=[1.0]), dict(weights=[float("nan")] * 6),
           dict(logits=torch.zeros(6, 8, 8, dtype=torch.float64)), dict(logits=torch.zeros(8, 8)), dict()]    # the last: not on the device
    for kw in bad:
        k = dict(dict(logits=logits, sizes=sizes, K=3), **kw)
        with pytest.raises(ValueError, match="label_maps"):
            eng.label_maps(k.pop("logits"), k.pop("sizes"), **k)
    pred, gt = np.zeros(10, np.int32), np.zeros(10, np.uint8)
    bad = [dict(num_classes=0), dict(num_classes=65537), dict(num_classes=3.0), dict(ignore_index=2 ** 31), dict(ignore_index=None),
           dict(reduce_zero_label=1), dict(pred=np.zeros(10, np.float32)), dict(pred=np.full(10, 2 ** 32 + 1, np.int64)),
           dict(gt=np.full(10, -2 ** 31 - 1, np.int64)), dict(gt=np.zeros(9, np.uint8)), dict(gt=[0] * 10),
           dict(pred=np.zeros(0, np.int32), gt=np.zeros(0, np.uint8)), dict(totals=torch.zeros(3, 4, dtype=torch.int64)),
           dict(totals=torch.zeros(3, 3, dtype=torch.int32)), dict(totals=np.zeros((3, 3), np.int64))]
    for kw in bad:
        k = dict(dict(pred=pred, gt=gt, num_classes=3), **kw)
        with pytest.raises(ValueError, match="label_iou"):
            eng.label_iou(k.pop("pred"), k.pop("gt"), **k)
    assert rec.calls == []
    assert eng.label_iou(pred, gt, num_classes=3).shape == (3, 3) and rec.calls == ["label_iou_hist"]


def test_containers():
    assert [f.name for f in dataclasses.fields(ClassHypotheses)] == ["classes", "pass1_logits", "masks", "edges", "logits", "pred"]
    h = ClassHypotheses(classes=None, pass1_logits=None, masks=None, edges=None, logits=None, pred=None)
    assert h.label_maps is None
    dims, off, most = label_tables([(4, 5), (6, 7)])
    assert dims.tolist() == [[4, 5], [6, 7]] and off.tolist() == [0, 20, 62] and most == 42
    z16 = torch.arange(62, dtype=torch.int16)
    m = LabelMaps(score=torch.zeros(62), winner=z16, segment=z16.clone(), areas=torch.zeros(3, 6, dtype=torch.int32),
                  segment_id=torch.tensor([0, 1, 2, 1, 0, 0], dtype=torch.int32), n_segments=torch.tensor([2, 1], dtype=torch.int32),
                  status=torch.zeros(1, dtype=torch.int32), dims=torch.from_numpy(dims), pix_offsets=torch.from_numpy(off),
                  sizes=[(4, 5), (6, 7)], K=3)
    assert m.B == 2 and m.winner_of(1).shape == (6, 7) and int(m.winner_of(1)[0, 0]) == 20 and m.segment_of(0).shape == (4, 5)
    assert m.kept.tolist() == [[False, True, True], [True, False, False]]
    m.check()
    host = m.to_host()
    assert host["winner"][1].shape == (6, 7) and host["kept"].tolist() == m.kept.tolist() and host["status"] == 0
    m.status[0] = 1
    with pytest.raises(RuntimeError, match="label_maps"):
        m.check()
    for kw in (dict(labels=[[1, 2, 3]]), dict(labels=[[1.0, 2, 3], [4, 5, 6]]), dict(labels=[[1, 2, 3], [4, 5, 6]], which="both"),
               dict(labels=[[1, 2, 3], [4, 5, 6]], void=2 ** 31)):
        with pytest.raises(ValueError, match="LabelMaps"):
            m.categories(**kw)


# ---- the histogram and the metrics -------------------------------------------------------------------------------------------------------
def host_hist(pred, gt, C, ignore_index=255, reduce_zero_label=False, totals=None):
    fresh = totals is None
    if fresh:
        totals = torch.full((3, C), -5, dtype=torch.int64)
    hip.label_iou_hist(torch.from_numpy(np.ascontiguousarray(pred, dtype=np.int32)), torch.from_numpy(np.ascontiguousarray(gt)), C, ignore_index,
                       reduce_zero_label, fresh, totals, host=True)
    return totals


def test_eval_metrics_on_a_hand_example():
    """Three classes, ten pixels.  gt 255 is ignored (pixel 9); the prediction 3 = C at pixel 8 is counted nowhere -- np.histogram would
    put it into class 2 --, while its gt 2 still counts as label."""
    gt = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2, 255], np.uint8)
    pred = np.array([0, 0, 1, 1, 1, 2, 2, 0, 3, 1], np.int32)
    want = np.array([[2, 2, 1], [3, 3, 2], [3, 3, 3]], np.int64)    # intersect; pred counts; label counts
    assert np.array_equal(LO.intersect_and_union(pred, gt, 3), want)
    assert np.array_equal(host_hist(pred, gt, 3).numpy(), want)
    assert np.array_equal(host_hist(pred, gt.astype(np.int32), 3).numpy(), want)
    all_acc, acc, iou = segeval.eval_metrics(want)
    assert all_acc == 5 / 9 and acc.tolist() == [2 / 3, 2 / 3, 1 / 3] and iou.tolist() == [2 / 4, 2 / 4, 1 / 4]
    _, _, iou, dice = segeval.eval_metrics(torch.from_numpy(want), metrics=("mIoU", "mDice"))
    assert dice.tolist() == [4 / 6, 4 / 6, 2 / 5] and segeval.mean_iou(want) == np.mean([0.5, 0.5, 0.25])
    assert segeval.mean_dice(want) == np.mean([4 / 6, 4 / 6, 2 / 5])
    # reduce_zero_label: gt 0 -> ignored, 1 -> 0, 2 -> 1, 255 stays ignored
    want_r = LO.intersect_and_union(pred, gt, 3, reduce_zero_label=True)
    assert want_r.tolist() == [[0, 0, 0], [1, 2, 2], [3, 3, 0]]       # pixels 3 .. 8: pred 1 1 2 2 0 3 against gt 0 0 0 1 1 1
    assert np.array_equal(host_hist(pred, gt, 3, reduce_zero_label=True).numpy(), want_r)
    assert np.array_equal(host_hist(pred, gt.astype(np.int32), 3, reduce_zero_label=True).numpy(), want_r)
    # a class that occurs nowhere is NaN, nan_to_num replaces it, the means skip it
    absent = np.array([[2, 0], [3, 0], [3, 0]], np.int64)
    _, acc, iou = segeval.eval_metrics(absent)
    assert np.isnan(iou[1]) and np.isnan(acc[1]) and segeval.mean_iou(absent) == 2 / 4
    assert segeval.eval_metrics(absent, nan_to_num=0)[2].tolist() == [0.5, 0.0] and segeval.mean_iou(absent, nan_to_num=0) == 0.25
    with pytest.raises(KeyError):
        segeval.eval_metrics(want, metrics=("mFscore",))
    with pytest.raises(ValueError):
        segeval.eval_metrics(np.zeros((2, 3), np.int64))


@pytest.mark.parametrize("C", [3, 150, 4097])
@pytest.mark.parametrize("gt_dtype", [np.uint8, np.int32])
def test_host_histogram_equals_the_definition(C, gt_dtype):
    rng = np.random.default_rng(C)
    for n in (1, 63, 1000, 4133):
        top = min(C, 255) if gt_dtype is np.uint8 else C
        gt = rng.integers(0, top + 1, n).astype(gt_dtype)            # the value C itself occurs
        if gt_dtype is np.int32:
            gt[rng.random(n) < 0.05] = -3
        gt[rng.random(n) < 0.1] = 255
        pred = np.where(rng.random(n) < 0.6, gt.astype(np.int64), rng.integers(-1, C + 2, n)).astype(np.int32)
        for reduce in (False, True):
            for ignore in (255, 0):
                want = LO.intersect_and_union(pred, gt, C, ignore, reduce)
                assert np.array_equal(host_hist(pred, gt, C, ignore, reduce).numpy(), want), (n, reduce, ignore)
        # two calls accumulate to one call over the concatenation
        if n > 1:
            t = host_hist(pred[:n // 3], gt[:n // 3], C)
            t = host_hist(pred[n // 3:], gt[n // 3:], C, totals=t)
            assert np.array_equal(t.numpy(), LO.intersect_and_union(pred, gt, C))
