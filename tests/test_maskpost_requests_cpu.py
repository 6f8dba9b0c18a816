"""The host checks of the packed-mask family (camouflaged_vlm_amd/maskpost.py), argument by argument: for every `*_request` one valid
call whose result is held to literals, and a table that spoils one argument per row -- a bool, a float or a string where an int is
wanted, None where it is not allowed, the ways an (h, w) list goes wrong, the ways "one or one per plane" goes wrong -- each refused
with ValueError under the caller's name; then every MaskUtilities method that takes a SizedMasks, on a bare MaskUtilities(): the
checks come before the device is touched.  STRICTER lists the inputs a tree may refuse on the host although the commit that
introduced this file did not: there each ended in another exception, or in a plane the kernel refused.  n, K, side and the counts of
pixels are the engine's own values, not the caller's, and are not spoiled."""
import numpy as np
import pytest
import torch

from camouflaged_vlm_amd import hip, maskpost
from camouflaged_vlm_amd.maskpost import MaskUtilities, RenderLayer, SizedImages
from test_gt_cpu import fake_gt

W = "Caller.method"
I64 = np.int64
S3 = [(3, 4), (5, 33), (3, 4)]                       # three planes, the first and the last of one size
NOT_INT = {"a bool": True, "a float": 2.0, "a string": "2", "None": None}
# what is wrong with a list of (h, w): the value, and whether a function without a count check (sized_request) refuses it too
BAD_SIZES = {"a string": "ab", "no sequence": 7, "a triple": [(3, 4, 5)], "h = 0": [(0, 5)], "h = 16385": [(16385, 5)], "w = 0": [(5, 0)],
             "w = 16385": [(5, 16385)], "a bool": [(True, 5)], "a float": [(5.0, 5)], "a pair that is a string": ["ab"], "a pair that is an int": [7]}
BAD_COUNTS = {"an empty list": [], "65536 pairs": [(1, 1)] * 65536}


def per_plane(lo: int, hi: int, P: int = 3) -> dict:
    """The ways "one int in [lo, hi] or one per plane" goes wrong, for P planes."""
    ok = [lo] * P
    out = {"a bool": True, "a float": float(lo), "a string": str(lo), "too few": ok[:-1], "too many": ok + [lo], "below": lo - 1, "above": hi + 1,
           "a bool inside": ok[:1] + [True] + ok[2:], "a float inside": ok[:-1] + [float(lo)], "a string of P": "1" * P}
    for at, where in ((0, "first"), (P // 2, "middle"), (P - 1, "last")):
        out[f"below at the {where}"] = ok[:at] + [lo - 1] + ok[at + 1:]
        out[f"above at the {where}"] = ok[:at] + [hi + 1] + ok[at + 1:]
    return out


def spoil(fn, args: tuple, kw: dict, name, values: dict, what: str = "") -> list:
    """One row per value: the valid call (args, kw) with the keyword `name` -- or the positional argument of that index -- replaced."""
    rows = []
    for label, v in values.items():
        a, k = list(args), dict(kw)
        if isinstance(name, int):
            a[name] = v
        else:
            k[name] = v
        rows.append(pytest.param(fn, tuple(a), k, id=f"{fn.__name__} {what or name}: {label}"))
    return rows


ROWS, STRICTER, VALID = [], [], []


def table(fn, args, kw, want, spoiled: dict, stricter: dict = ()):
    """Registers a request function: its valid call with the expected result, the rows that spoil it, and the STRICTER rows."""
    VALID.append(pytest.param(fn, args, kw, want, id=fn.__name__))
    for name, values in spoiled.items():
        ROWS.extend(spoil(fn, args, kw, name, values))
    for name, values in dict(stricter).items():
        STRICTER.extend(spoil(fn, args, kw, name, values))


def same(a, b) -> bool:
    """Equal, to the type and dtype of every numpy array; tuples, lists and dataclasses field by field."""
    if isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and bool((a == b).all())
    if isinstance(b, (tuple, list)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(b, dict):
        return all(same(getattr(a, k), v) for k, v in b.items())     # a dataclass against its fields
    return type(a) is type(b) and a == b


def arr(v, dt):
    return np.asarray(v, dtype=dt)


CONNECTIVITY = dict(NOT_INT, **{"6": 6, "0": 0, "[8]": [8]})

table(maskpost.compact_request, (), dict(masks="both", overlaps=True, n=2, K=3), (True, True, True),
      dict(masks={"a bool": True, "an int": 1, "None": None, "another string": "bit"}, overlaps={"an int": 1, "a string": "yes", "None": None},
           K={"1025 with overlaps": 1025}, n={"too many in all": 30000}))
table(maskpost.components_request, (), dict(components=I64(2), min_area=I64(16), connectivity=I64(4), masks="bits", side=64), (True, 2, 16, 4),
      dict(components={"a bool": True, "a float": 2.0, "a string": "2", "-1": -1, "65": 65}, min_area=dict(NOT_INT, **{"-1": -1}),
           connectivity=CONNECTIVITY, masks={"logits": "logits"}, side={"48": 48}))
table(maskpost.holes_request, (), dict(holes=I64(2), fill_holes=I64(16), connectivity=I64(4), masks="bits", side=64), (True, 2, 16, 4),
      dict(holes={"a bool": True, "a float": 2.0, "a string": "2", "-1": -1, "65": 65}, fill_holes=dict(NOT_INT, **{"-1": -1, "2^31": 2 ** 31}),
           connectivity=CONNECTIVITY, masks={"logits": "logits"}, side={"48": 48}))
table(maskpost.morph_request, (), dict(band=I64(2), masks="both", overlaps=True, side=64), (True, 2, True),
      dict(band={"a bool": True, "a float": 2.0, "a string": "2", "0": 0, "17": 17}, masks={"logits": "logits"}, side={"48": 48}))
table(maskpost.edge_request, (), dict(edge_threshold=0.5, masks="both", overlaps=True, band=2, side=64), (True, 0.5, True, True),
      dict(edge_threshold={"a bool": True, "a string": "0.5", "0": 0, "1": 1, "NaN": float("nan"), "a list": [0.5], "below float32": 1e-60},
           masks={"logits": "logits"}, side={"48": 48}))
table(maskpost.rle_request, (), dict(rle="kept", masks="bits", min_area=I64(1), fill_holes=0, side=64), "kept_bits",
      dict(rle={"a bool": True, "an int": 1, "another string": "bits", "filled without fill_holes": "filled"}, masks={"logits": "logits"},
           min_area={"0": 0, "a bool": True, "a float": 1.0}, side={"48": 48}))
table(maskpost.sized_request, (), dict(sizes=[(I64(3), 4), [5, 33]], sized_level=I64(1), n=2, masks="bits"), ([(3, 4), (5, 33)], 1),
      dict(sizes={"three for two images": S3}, sized_level=dict(NOT_INT, **{"0": 0, "256": 256}), masks={"logits": "logits"}, n={"another count": 3}))
for label, v in BAD_SIZES.items():                   # with the count they hold, so that the entry is what is refused
    ROWS.append(pytest.param(maskpost.sized_request, (), dict(sizes=v, n=len(v) if hasattr(v, "__len__") else 1), id=f"sized_request sizes: {label}"))
ROWS.append(pytest.param(maskpost.sized_request, (), dict(sizes=None, n=2, rle="sized"), id="sized_request rle='sized' without sizes"))
table(maskpost.labels_request, (), dict(label_maps=True, sizes=S3, weights=[1, 0.5] * 3, level=I64(64), overlap_threshold=0.5, n=3, K=2),
      (arr([1, 0.5] * 3, np.float32), 64, 0.5),
      dict(label_maps={"an int": 1, "a string": "yes", "None": None}, sizes={"None": None}, masks={"logits": "logits"},
           level=dict(NOT_INT, **{"0": 0, "256": 256}), K={"0": 0, "16385": 16385},
           overlap_threshold={"a bool": True, "a string": "0.5", "None": None, "0": 0, "1.5": 1.5, "NaN": float("nan")},
           weights={"a string": "abcdef", "five": [1.0] * 5, "a NaN": [1.0] * 5 + [float("nan")], "a None inside": [1.0] * 5 + [None]}))
ROWS.append(pytest.param(maskpost.labels_request, (), dict(label_maps=False, weights=[1.0], n=1, K=1), id="labels_request weights without label maps"))

PQ = dict(num_classes=I64(5), n_pred=12 + 165, n_gt=12 + 165)
PQ_ARGS = ([[-1, 1, 2], [-1, 3, 4]], [[-1, 0], [-1, 4]], [[0, 1], [0, 0]], [(3, 4), (5, 33)])
table(maskpost.pq_request, PQ_ARGS, PQ,
      ([(3, 4), (5, 33)], arr(PQ_ARGS[0], np.int32), arr(PQ_ARGS[1], np.int32), arr(PQ_ARGS[2], np.uint8), 2, 3),
      {"num_classes": dict(NOT_INT, **{"0": 0, "65537": 65537, "4: a category beyond": 4}), 3: dict(BAD_SIZES, **BAD_COUNTS, **{"None": None}),
       "n_pred": {"another count": 5}, "n_gt": {"another count": 5},
       0: {"floats": [[-1.0, 1.0]] * 2, "one image": [[-1, 1]], "slot 0 is no void": [[0, 1], [-1, 1]], "bools": [[True, False]] * 2, "a string": "ab",
           "-2": [[-1, -2], [-1, 1]], "flat": [-1, 1]},
       1: {"floats": [[-1.0, 1.0]] * 2, "one image": [[-1, 1]], "slot 0 is no void": [[0, 1], [-1, 1]], "5": [[-1, 5], [-1, 1]]},
       2: {"a 2": [[0, 2], [0, 0]], "another shape": [[0, 1, 0], [0, 0, 0]], "floats": [[0.0, 1.0]] * 2}})
SEG = [[(1, 1, 0), (I64(2), I64(2), True)], [(7, 3, 0)]]
table(maskpost.pq_segments_request, (SEG, 2), dict(num_classes=5),
      (arr([1, 2, 7], np.int32), arr([1, 2, 1], np.int32), arr([0, 2, 3], np.int64), arr([[-1, 1, 2], [-1, 3, -1]], np.int32),
       arr([[0, 0, 1], [0, 0, 0]], np.uint8)),
      {0: {"a string": "ab", "one image": SEG[:1], "a pair": [[(1, 1)], []], "a segment that is a string": [["abc"], []], "id 0": [[(0, 1, 0)], []],
           "id 2^24": [[(2 ** 24, 1, 0)], []], "a bool id": [[(True, 1, 0)], []], "a float id": [[(1.0, 1, 0)], []], "category -1": [[(1, -1, 0)], []],
           "a bool category": [[(1, True, 0)], []], "category 5": [[(1, 5, 0)], []], "iscrowd 2": [[(1, 1, 2)], []], "an id twice": [[(1, 1, 0), (1, 2, 0)], []],
           "no sequence": 7, "None": None}},
      {0: {"an image that is an int": [7, 7]}})          # before: TypeError from len() of the image's segments

RLE = [{"size": [I64(2), 3], "counts": [1, 2, 3]}, {"size": (1, 1), "counts": np.asarray([0, 1])}]
rle_size = lambda v: [{"size": v, "counts": [1]}]
BAD_ENTRY_SIZE = {"a string": "ab", "no sequence": 7, "a triple": (3, 4, 5), "h = 0": (0, 5), "h = 16385": (16385, 5), "a bool": (True, 5),
                  "a float": (5.0, 5), "None": None}
table(maskpost.rle_decode_request, (RLE,), {}, (arr([1, 2, 3, 0, 1], np.int32), arr([0, 3, 5], np.int64), [(2, 3), (1, 1)]),
      {0: dict({"a string": "ab", "no sequence": 7, "None": None, "a dict": RLE[0], "an empty list": [], "65536 entries": [RLE[1]] * 65536,
                "an entry that is no dict": [7], "no counts": [{"size": [2, 3]}], "counts that sum to 5": [{"size": [2, 3], "counts": [5]}],
                "a negative count": [{"size": [2, 3], "counts": [7, -1]}], "a float count": [{"size": [2, 3], "counts": [3.0, 3]}],
                "a bool count": [{"size": [2, 3], "counts": [True, 5]}], "counts that are an int": [{"size": [2, 3], "counts": 6}]},
               **{f"size: {k}": rle_size(v) for k, v in BAD_ENTRY_SIZE.items()})})
POLY = [{"size": [I64(5), 33], "polygons": [[1, 1, 20, 1, 20, 4.5]]}, {"size": (3, 4), "polygons": [np.asarray([0, 0, 2, 0, 2, 2, 0, 2]), [0, 0, 1, 0, 1, 1]]}]
poly_size = lambda v: [{"size": v, "polygons": POLY[0]["polygons"]}]
poly = lambda v: [{"size": [5, 33], "polygons": v}]
table(maskpost.polygons_request, (POLY,), {},
      (arr([1, 1, 20, 1, 20, 4.5, 0, 0, 2, 0, 2, 2, 0, 2, 0, 0, 1, 0, 1, 1], np.float64), arr([0, 6, 14, 20], np.int64), arr([0, 1, 3], np.int32),
       [(5, 33), (3, 4)]),
      {0: dict({"a string": "ab", "no sequence": 7, "None": None, "a dict": POLY[0], "an empty list": [], "65536 entries": [POLY[0]] * 65536,
                "an entry that is no dict": [7], "no polygons": [{"size": [5, 33]}], "polygons: none": poly([]), "polygons: a string": poly("ab"),
                "polygons: 4097": poly([[0, 0, 1, 0, 1, 1]] * 4097), "a polygon that is a string": poly(["abcdef"]), "two vertices": poly([[0, 0, 1, 1]]),
                "an odd count": poly([[0, 0, 1, 0, 1, 1, 2]]), "a bool": poly([[0, 0, 1, 0, 1, True]]), "inf": poly([[0, 0, 1, 0, 1, float("inf")]]),
                "beyond 65536": poly([[0, 0, 1, 0, 1, 65537]]), "nested": poly([[[0, 0], [1, 0], [1, 1]]])},
               **{f"size: {k}": poly_size(v) for k, v in BAD_ENTRY_SIZE.items()})})

table(maskpost.pairs_request, (S3, S3[:2]), dict(pairs=[(I64(2), 1), (0, 0)]), arr([[2, 1], [0, 0]], np.int32),
      dict(pairs={"none of the three": None, "empty": [], "triples": [(0, 0, 0)], "flat": [0, 0], "floats": [(0.0, 0.0)], "negative": [(-1, 0)],
                  "a beyond": [(3, 0)], "b beyond": [(0, 2)], "a string": "ab", "bools": [(True, False)]},
           a_image={"with pairs": [0, 0, 0]}, b_image={"with pairs": [0, 0]}))
ids_ok = dict(a_image=[I64(0), 1, 0], b_image=[0, 5])
VALID.append(pytest.param(maskpost.pairs_request, (S3, S3[:2]), ids_ok, arr([[0, 0], [2, 0]], np.int32), id="pairs_request image ids"))
for side, P in (("a_image", 3), ("b_image", 2)):
    ROWS.extend(spoil(maskpost.pairs_request, (S3, S3[:2]), ids_ok, side,
                      {"None": None, "a string": "0" * P, "no sequence": 7, "too few": [0] * (P - 1), "too many": [0] * (P + 1), "a bool inside": [0] * (P - 1) + [True],
                       "a float inside": [0.0] + [0] * (P - 1), "no pair": [9] * P}))

RADII = per_plane(1, 16384)
table(maskpost.boundary_request, (S3,), dict(radius=[I64(1), 2, 16384]), arr([1, 2, 16384], np.int32),
      dict(radius=RADII, dilation_ratio={"given with a radius": 0.05}))
VALID.append(pytest.param(maskpost.boundary_request, ([(480, 640), (100, 75), (1, 1)],), dict(dilation_ratio=0.02), arr([16, 2, 1], np.int32),
                          id="boundary_request ratio"))
VALID.append(pytest.param(maskpost.boundary_request, (S3,), dict(radius=I64(3)), arr([3, 3, 3], np.int32), id="boundary_request one radius"))
ROWS.extend(spoil(maskpost.boundary_request, (S3,), {}, "dilation_ratio",
                  {"a bool": True, "a string": "0.02", "None": None, "0": 0, "negative": -0.02, "inf": float("inf"), "NaN": float("nan"), "too large": 1e4}))

ALL_SIZES = dict(BAD_SIZES, **BAD_COUNTS)
table(maskpost.contour_request, (S3,), dict(connectivity=I64(4)), ([(3, 4), (5, 33), (3, 4)], 4), {0: ALL_SIZES, "connectivity": CONNECTIVITY})
REACH = {k: v for k, v in per_plane(0, 23170).items()}
table(maskpost.distance_request, ([(I64(3), 4), [5, 33], (3, 4)],), dict(reach=[0, I64(7), 23170]), ([(3, 4), (5, 33), (3, 4)], arr([0, 7, 23170], np.int32)),
      {0: ALL_SIZES, "reach": REACH})
VALID.append(pytest.param(maskpost.distance_request, (S3,), dict(reach=None), (S3, arr([0, 0, 0], np.int32)), id="distance_request no reach"))
VALID.append(pytest.param(maskpost.distance_request, (S3,), dict(reach=I64(9)), (S3, arr([9, 9, 9], np.int32)), id="distance_request one reach"))
table(maskpost.surface_request, (S3, S3), dict(pairs=[(0, 2), (1, 1)], tolerance=[I64(2), 0.5], reach="tolerance"),
      dict(a_sizes=S3, b_sizes=S3, pairs=arr([[0, 2], [1, 1]], np.int32), radii=arr([[2, 3], [2, 17]], np.int32), reach_a=arr([3, 17, 1], np.int32),
           reach_b=arr([1, 17, 3], np.int32)),
      {0: ALL_SIZES, 1: ALL_SIZES,
       "pairs": {"a string": "ab", "empty": [], "triples": [(0, 0, 0)], "flat": [0, 0], "floats": [(0.0, 0.0)], "negative": [(-1, 0)], "a beyond": [(3, 0)],
                 "b beyond": [(0, 3)], "two sizes": [(0, 1)], "bools": [(True, False)]},
       "tolerance": {"a bool": True, "a string": "ab", "None": None, "none": [], "nine": [1] * 9, "-1": -1, "23171": 23171, "1.5": 1.5, "0.0": 0.0,
                     "a bool inside": [1, True], "a string inside": [1, "1"]},
       "reach": {"a bool": True, "a float": 2.0, "another string": "far", "-1": -1, "23171": 23171, "one per plane": [1, 1, 1]}})
VALID.append(pytest.param(maskpost.surface_request, (S3, S3), dict(tolerance=I64(0), reach=I64(5)),
                          dict(pairs=arr([[0, 0], [1, 1], [2, 2]], np.int32), radii=arr([[0], [0], [0]], np.int32), reach_a=arr([5, 5, 5], np.int32),
                               reach_b=arr([5, 5, 5], np.int32)), id="surface_request plane p against plane p"))
ROWS.append(pytest.param(maskpost.surface_request, (S3, S3[:2]), {}, id="surface_request no pairs, 3 planes against 2"))
ITERS = {k: v for k, v in per_plane(1, 2 ** 30).items()}
table(maskpost.thin_request, (S3,), dict(max_iter=[I64(1), 2, 2 ** 30], path="steps", steps=I64(7)), (S3, arr([1, 2, 2 ** 30], np.int32), 1, 7),
      {0: ALL_SIZES, "max_iter": ITERS, "path": {"an int": 1, "another string": "fast", "None": None, "a bool": True},
       "steps": dict(NOT_INT, **{"0": 0, "1025": 1025})})
VALID.append(pytest.param(maskpost.thin_request, (S3,), {}, (S3, arr([0, 0, 0], np.int32), 0, 64), id="thin_request defaults"))
VALID.append(pytest.param(maskpost.thin_request, (S3,), dict(max_iter=I64(4)), (S3, arr([4, 4, 4], np.int32), 0, 64), id="thin_request one max_iter"))
table(maskpost.regions_request, (S3,), dict(regions=I64(2), min_area=I64(9), connectivity=I64(4)), (S3, 2, 9, 4),
      {0: ALL_SIZES, "regions": dict(NOT_INT, **{"0": 0, "65": 65}), "min_area": dict(NOT_INT, **{"-1": -1, "2^31": 2 ** 31}), "connectivity": CONNECTIVITY})

MATCH = dict(det_image=[0, I64(1), 0], gt_image=[1, 0], det_category=[7, 7, 7], gt_category=[7, 7], iscrowd=[0, 1], gt_area=[4.0, 5], scores=[0.5, 0.25, 1],
             iou_thrs=[0.5, 1], area_rngs=[(0, 1e10)], max_det=I64(2))
MATCH_SIZES = ([(3, 4), (5, 33), (3, 4)], [(5, 33), (3, 4)])
table(maskpost.match_request, MATCH_SIZES, MATCH,
      dict(keys=[(7, 0), (7, 1)], det_perm=arr([0, 2, 1], np.int64), gt_perm=arr([1, 0], np.int64), det_offsets=arr([0, 2, 3], np.int32),
           gt_offsets=arr([0, 1, 2], np.int32), pair_offsets=arr([0, 2, 3], np.int64), pairs=arr([[0, 1], [2, 1], [1, 0]], np.int32),
           crowd=arr([1, 0], np.uint8), range_area=arr([5, 4], np.float64), scores=arr([0.5, 1, 0.25], np.float32), iou_thrs=arr([0.5, 1], np.float64),
           area_rngs=arr([[0, 1e10]], np.float64), max_det=2),
      dict(det_image={"None": None, "no sequence": 7, "a string": "010", "too few": [0, 1], "a bool inside": [0, True, 0], "a float inside": [0, 1.0, 0], "another size in the group": [1, 1, 0]},
           gt_image={"None": None, "a string": "10", "too many": [1, 0, 0], "a bool inside": [True, 0]}, det_category={"None": None, "too few": [7, 7], "a float inside": [7, 7.0, 7]},
           gt_category={"None": None, "a string": "77"}, iscrowd={"too few": [0], "strings": ["a", "b"]},
           gt_area={"negative": [4.0, -1], "inf": [4.0, float("inf")], "too few": [4.0], "strings": ["a", "b"]},
           scores={"a NaN": [0.5, float("nan"), 1], "too few": [0.5, 1], "strings": ["a", "b", "c"]},
           iou_thrs={"none": [], "0": [0], "1.5": [1.5], "seventeen": [0.5] * 17, "a string": "ab", "nested": [[0.5]]},
           area_rngs={"hi below lo": [(2, 1)], "nine": [(0, 1)] * 9, "flat": [0, 1], "none": []}, max_det=dict(NOT_INT, **{"0": 0, "2^31": 2 ** 31})),
      {0: {"no sequence": 7, "None": None}, 1: {"no sequence": 7}})                      # before: TypeError from len() of the sizes
ROWS.append(pytest.param(maskpost.match_request, ([], []), dict(det_image=[], gt_image=[]), id="match_request nothing on either side"))

NMS = dict(image=[I64(4), 9, 4], iou=I64(1), measure="min", method="gaussian", sigma=I64(3))
table(maskpost.nms_request, (S3,), NMS,
      dict(keys=[4, 9], member=arr([0, 2, 1], np.int32), group_offsets=arr([0, 2, 3], np.int32), pair_offsets=arr([0, 1, 1], np.int64), thr=1.0,
           measure=hip.NMS_MEASURES["min"], method=hip.NMS_METHODS["gaussian"], sigma=3.0),
      {0: ALL_SIZES, "image": {"a string": "494", "no sequence": 7, "None": None, "too few": [4, 9], "a bool inside": [4, True, 4], "a float inside": [4.0, 9, 4],
                               "another size in the group": [4, 4, 4]},
       "iou": {"a bool": True, "a string": "0.5", "None": None, "-0.1": -0.1, "1.1": 1.1, "NaN": float("nan")},
       "measure": {"an int": 1, "another string": "dice", "None": None}, "method": {"an int": 1, "another string": "soft", "None": None},
       "sigma": {"a bool": True, "a string": "2", "None": None, "0": 0, "inf": float("inf"), "NaN": float("nan")}})

BITS = torch.zeros(64, dtype=torch.uint8)
layer = lambda **kw: RenderLayer(**dict(dict(kind=0, flags=0, source=BITS, src=0, size=(3, 4), rgb=arr([[1, 2, 3]], np.uint8), alpha=arr([0.5], np.float32)), **kw))
table(maskpost.render_request, ([(I64(3), 4), (5, 33)], [[layer(), layer(src=I64(12), flags=hip.RENDER_INVERT)], []]), dict(device="cpu"),
      dict(layer_offsets=arr([0, 2, 2], np.int32), layers=arr([[0, 0, 0, 1], [hip.RENDER_INVERT << 8, 12, 1, 1]], np.int64),
           rgb=arr([[1, 2, 3], [1, 2, 3]], np.uint8), alpha=arr([0.5, 0.5], np.float32)),
      {0: ALL_SIZES,
       1: {"no sequence": 7, "None": None, "a string": "ab", "a layer": layer(), "one image": [[layer()]], "layers that are no lists": [layer(), layer()], "no layer": [[7], []],
           "another size": [[layer(size=(4, 3))], []], "a slice past the end": [[layer(src=60)], []], "a slice off a word": [[layer(src=2)], []],
           "an edges flag on bits": [[layer(flags=hip.RENDER_EDGES)], []], "int32 bits": [[layer(source=BITS.view(torch.int32))], []],
           "float colours": [[layer(rgb=np.ones((1, 3)))], []], "two colours": [[layer(rgb=np.ones((2, 3), np.uint8))], []],
           "an alpha of 2": [[layer(alpha=arr([2], np.float32))], []], "a bool src": [[layer(src="0")], []]},
       "device": {"another device": "meta"}})

SREQ = ([(3, 4), (5, 33)], 128)
GT = fake_gt(S3)
table(maskpost.ground_truth_request, ((GT, [0, I64(1), 0]), SREQ, 2), {}, (GT, [0, 1, 0]),
      {0: {"ids None": (GT, None), "a triple": (GT, [0, 1, 0], 3), "no pair": GT, "too few ids": (GT, [0, 1]), "too many ids": (GT, [0, 1, 0, 0]),
           "another size": (GT, [1, 1, 0]), "image 2 of 2": (GT, [0, 1, 2]), "image -1": (GT, [0, 1, -1]), "a float id": (GT, [0, 1.0, 0]),
           "a bool id": (GT, [0, True, 0]), "ids that are a string": (GT, "010"), "no SizedMasks": ("gt", [0, 1, 0]), "a tensor": (BITS, [0, 1, 0]),
           "no areas": (fake_gt(S3, area=False), [0, 1, 0]), "on the host": (fake_gt(S3, cuda=False), [0, 1, 0]), "a string": "ab", "an int": 7},
       1: {"no sizes": None}})


@pytest.mark.parametrize("fn, args, kw, want", VALID)
def test_a_valid_request_returns_exactly_this(fn, args, kw, want):
    got = fn(*args, **kw, who=W)
    assert same(got, want), (got, want)


@pytest.mark.parametrize("fn, args, kw", ROWS)
def test_a_spoiled_argument_is_refused_under_the_callers_name(fn, args, kw):
    with pytest.raises(ValueError, match="^" + W + ": "):
        fn(*args, **kw, who=W)


@pytest.mark.parametrize("fn, args, kw", STRICTER)
def test_what_may_be_refused_on_the_host_never_returns(fn, args, kw):
    """A STRICTER row ends in an exception of some kind, before or after this file's commit; where it is a ValueError, it is under the
    caller's name."""
    with pytest.raises(Exception) as e:
        fn(*args, **kw, who=W)
    assert not isinstance(e.value, ValueError) or str(e.value).startswith(W + ": ")


def test_an_integer_of_numpy_is_an_int_everywhere():
    """np.int64 where an int is wanted is accepted: the VALID calls above pass one for every int and every per-plane entry."""
    assert sum("int64" in repr(p.values[1:3]) for p in VALID) >= 15


# ---- the SizedMasks arguments of MaskUtilities ---------------------------------------------------------------------------------------
def sized(area=True, box=True, cuda=True, sizes=S3):
    s = fake_gt(sizes, area=area, cuda=cuda)
    s.box = torch.zeros(len(sizes), 4) if box else None
    return s


IMAGES = SizedImages(data=torch.zeros(12, dtype=torch.uint8), offsets=None, dims=None, sizes=[(1, 4)])
NMS_KW = dict(scores=[1.0] * 3, image=[0, 1, 2])
MATCH_KW = dict(scores=[1.0] * 3, det_image=[0, 1, 2], gt_image=[0, 1, 2])
# method -> (how it is called with the spoiled argument(s), which of areas / boxes the argument needs)
METHODS = {
    "mask_rle_sized": (lambda m, s: m.mask_rle_sized(s), ()),
    "mask_boundary_sized": (lambda m, s: m.mask_boundary_sized(s), ()),
    "mask_contours_sized": (lambda m, s: m.mask_contours_sized(s), ()),
    "mask_distance_sized": (lambda m, s: m.mask_distance_sized(s), ()),
    "mask_thin_sized": (lambda m, s: m.mask_thin_sized(s), ()),
    "mask_regions_sized": (lambda m, s: m.mask_regions_sized(s), ()),
    "mask_nms_sized": (lambda m, s: m.mask_nms_sized(s, **NMS_KW), ("area", "box")),
    "mask_inter_sized a": (lambda m, s: m.mask_inter_sized(s, sized(), pairs=[(0, 0)]), ("area",)),
    "mask_inter_sized b": (lambda m, s: m.mask_inter_sized(sized(), s, pairs=[(0, 0)]), ("area",)),
    "mask_surface_distances a": (lambda m, s: m.mask_surface_distances(s, sized()), ()),
    "mask_surface_distances b": (lambda m, s: m.mask_surface_distances(sized(), s), ()),
    "mask_cldice a": (lambda m, s: m.mask_cldice(s, sized()), ("area",)),
    "mask_cldice b": (lambda m, s: m.mask_cldice(sized(), s), ("area",)),
    "coco_match dets": (lambda m, s: m.coco_match(s, sized(), **MATCH_KW), ("area",)),
    "coco_match gts": (lambda m, s: m.coco_match(sized(), s, **MATCH_KW), ("area",)),
}
SPOILED = {"a string": lambda: "sized", "a tensor": lambda: BITS, "None": lambda: None, "on the host": lambda: sized(cuda=False),
           "without areas": lambda: sized(area=False), "without boxes": lambda: sized(box=False)}
SIZED_ROWS = [pytest.param(name, how, id=f"{name}: {how}") for name, (_, needs) in METHODS.items() for how in SPOILED
              if not (how == "None" and name.startswith("coco_match")) and not (how == "without areas" and "area" not in needs)
              and not (how == "without boxes" and "box" not in needs)]
SIZED_ROWS += [pytest.param("render_overlay", how, id=f"render_overlay: {how}") for how in ("a string", "a tensor", "None")]
METHODS["render_overlay"] = (lambda m, s: m.render_overlay(IMAGES, s, image_of=[0, 0, 0]), ())


@pytest.mark.parametrize("name, how", SIZED_ROWS)
def test_a_utility_refuses_what_is_no_sized_masks_under_its_own_name(name, how):
    with pytest.raises(ValueError, match="^" + name.split()[0] + ": "):
        METHODS[name][0](MaskUtilities(), SPOILED[how]())


def test_coco_match_takes_none_for_a_side_without_planes_but_not_for_both():
    with pytest.raises(ValueError, match="^coco_match: no detection and no annotation"):
        MaskUtilities().coco_match(None, None, scores=[], det_image=[], gt_image=[])
