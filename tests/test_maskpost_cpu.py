"""The packed-mask family's host side after its move into camouflaged_vlm_amd/maskpost.py: every public name is the same object under
`engine`; the plan of a call (MaskPost) refuses what the request functions refuse, under the caller's name, before anything exists
to allocate or launch with; the utilities on packed planes refuse bad (bits, H, W) under their own names.  No GPU."""
import numpy as np
import pytest
import torch

from camouflaged_vlm_amd import engine, maskpost
from camouflaged_vlm_amd.maskpost import MaskPost, MaskUtilities
from test_gt_cpu import fake_gt

NAMES = ("MASK_MODES", "OVERLAP_MAXK", "OVERLAP_MAXP", "COMPONENTS_MAXM", "COMPONENTS_WS_CAP", "HOLES_MAXM", "HOLE_FIELDS", "MORPH_MAXR",
         "BAND_FIELDS", "EDGE_FIELDS", "RLE_WS_CAP", "RLE_SOURCES", "RLE_SIZED", "SIZED_MAX_SIDE",
         "compact_request", "components_request", "holes_request", "morph_request", "_edge_threshold", "edge_request", "rle_request",
         "sized_tables", "sized_request", "rle_decode_request", "pairs_request", "ground_truth_request",
         "MaskComponents", "MaskHoles", "MaskMorph", "EdgeBits", "MaskRle", "SizedMasks", "SizedOverlaps")
UTILITIES = ("pack_masks", "mask_components", "mask_holes", "mask_morph", "pack_edges", "mask_rle", "pack_masks_sized", "mask_rle_sized",
             "rle_decode", "mask_inter_sized")


def test_every_public_name_is_one_object_under_both_modules():
    for name in NAMES:
        assert getattr(engine, name) is getattr(maskpost, name), name
    star = {}
    exec("from camouflaged_vlm_amd.engine import *", star)
    assert all(name in star for name in NAMES if not name.startswith("_"))
    for name in UTILITIES:
        assert getattr(engine.Cascade, name) is getattr(MaskUtilities, name), name
    assert "ClassHypotheses" not in vars(maskpost) and engine.ClassHypotheses.__module__ == engine.__name__


SIZES = [(213, 320), (480, 641)]
# the keyword sets the request tests refuse (test_compact_cpu.py .. test_gt_cpu.py), on the base each of them stands on
BAD = [(dict(), [dict(masks="bit"), dict(masks=None), dict(masks=1), dict(masks="BITS"), dict(masks=["bits"]), dict(overlaps=True),
                 dict(masks="logits", overlaps=True), dict(masks="bits", overlaps=True, K=1025), dict(masks="both", overlaps=True, K=1025),
                 dict(masks="bits", overlaps=True, n=64, K=1024), dict(masks="bits", overlaps=1), dict(masks="bits", overlaps="yes")]),
       (dict(masks="bits"),
        [dict(components=-1), dict(components=65), dict(components=1.0), dict(components="1"), dict(components=True), dict(min_area=-1),
         dict(min_area=1.5), dict(min_area=None), dict(min_area=True), dict(components=1, masks="logits"), dict(min_area=1, masks="logits"),
         dict(components=0, masks="logits"), dict(components=1, connectivity=6), dict(connectivity=6), dict(connectivity="8"),
         dict(connectivity=True), dict(connectivity=None), dict(components=1, side=48),
         dict(holes=-1), dict(holes=65), dict(holes=1.0), dict(holes="1"), dict(holes=True), dict(fill_holes=-1), dict(fill_holes=1.5),
         dict(fill_holes=None), dict(fill_holes=True), dict(fill_holes=2 ** 31), dict(holes=1, masks="logits"),
         dict(fill_holes=1, masks="logits"), dict(holes=0, masks="logits"), dict(holes=1, side=48), dict(fill_holes=4, side=1000),
         dict(band=0), dict(band=17), dict(band=-2), dict(band=2.0), dict(band="2"), dict(band=True), dict(band=np.bool_(True)),
         dict(band=2, masks="logits"), dict(band=2, side=48), dict(band=2, side=1000),
         dict(edge_threshold=0), dict(edge_threshold=1), dict(edge_threshold=0.0), dict(edge_threshold=1.0), dict(edge_threshold=-0.5),
         dict(edge_threshold=1.5), dict(edge_threshold=float("nan")), dict(edge_threshold=float("inf")), dict(edge_threshold=True),
         dict(edge_threshold=np.bool_(True)), dict(edge_threshold="0.5"), dict(edge_threshold=[0.5]), dict(edge_threshold=0.5 + 0j),
         dict(edge_threshold=1 - 1e-12), dict(edge_threshold=1e-60), dict(edge_threshold=0.5, masks="logits"),
         dict(edge_threshold=0.5, side=48), dict(edge_threshold=0.5, side=1000),
         dict(rle="bits"), dict(rle=""), dict(rle=True), dict(rle=1), dict(rle=b"mask"), dict(rle="mask", masks="logits"), dict(rle="kept"),
         dict(rle="kept", min_area=0), dict(rle="kept", fill_holes=5), dict(rle="filled"), dict(rle="filled", fill_holes=0),
         dict(rle="filled", min_area=5), dict(rle="mask", side=48), dict(rle="mask", side=1000),
         dict(sizes=[(3, 4)]), dict(sizes=[(3, 4)] * 3), dict(sizes=[(3, 4), (5,)]), dict(sizes=[(3, 4), (5, 6, 7)]), dict(sizes=[(3, 4), 5]),
         dict(sizes=[(3, 4), (5.0, 6)]), dict(sizes=[(3, 4), (True, 6)]), dict(sizes=[(3, 4), (0, 6)]), dict(sizes=[(3, 4), (5, 16385)]),
         dict(sizes=[(3, 4), (-1, 6)]), dict(sizes=[(3, 4), "56"]), dict(sizes="3456"), dict(sizes=7),
         dict(sizes=[(3, 4), (5, 6)], sized_level=0), dict(sizes=[(3, 4), (5, 6)], sized_level=256), dict(sized_level=0),
         dict(sizes=[(3, 4), (5, 6)], sized_level=128.0), dict(sizes=[(3, 4), (5, 6)], sized_level=True),
         dict(sizes=[(3, 4), (5, 6)], masks="logits"), dict(rle="sized"), dict(rle="sized", masks="both")])]


def ground_truth_sets():
    gt = fake_gt([SIZES[0], SIZES[0], SIZES[1]])
    bad = [(gt, None), (gt, [0, 0, 1], 3), gt, (gt, [0, 0]), (gt, [0, 0, 1, 1]), (gt, [0, 1, 1]), (gt, [1, 0, 1]), (gt, [0, 0, 2]), (gt, [0, 0, -1]),
           (gt, [0, 0, 1.0]), (gt, [0, 0, True]), (gt, "001"), ("gt", [0, 0, 1]), (gt.bits, [0, 0, 1]),
           (fake_gt(gt.sizes, area=False), [0, 0, 1]), (fake_gt(gt.sizes, cuda=False), [0, 0, 1])]
    return gt, [dict(sizes=SIZES, ground_truth=g) for g in bad] + [dict(ground_truth=(gt, [0, 0, 1])), dict(sizes=SIZES[::-1], ground_truth=(gt, [0, 0, 1]))]


@pytest.mark.parametrize("who", ["infer_classes", "decode"])
def test_the_plan_refuses_what_the_requests_refuse_under_the_callers_name(who):
    gt, gt_bad = ground_truth_sets()
    for base, sets in BAD + [(dict(masks="bits"), gt_bad)]:
        for kw in sets:
            with pytest.raises(ValueError, match="^" + who + ": "):
                MaskPost(**{**dict(who=who, n=2, K=3, side=320), **base, **kw})
    # what it accepts: attributes by name, nothing allocated
    p = MaskPost(who=who, n=2, K=3, side=320)
    assert (p.want_logits, p.want_bits, p.want_inter, p.want_comps, p.want_holes, p.want_band, p.want_edges) == (True,) + (False,) * 6
    assert p.rle_source is None and p.sizes is None and p.gt is None and all(v is None for v in p.fields().values())
    assert p.outputs() == () and p.inputs() == ()
    p = MaskPost(who=who, n=2, K=3, side=320, masks="both", overlaps=True, components=2, min_area=16, holes=3, fill_holes=8, connectivity=4,
                 band=2, edge_threshold=0.5, rle="sized", sizes=SIZES, sized_level=1, ground_truth=(gt, [0, 0, 1]))
    assert (p.want_logits, p.want_bits, p.want_inter) == (True, True, True)
    assert (p.want_comps, p.comps_m, p.min_area, p.connectivity) == (True, 2, 16, 4) and (p.want_holes, p.holes_m, p.fill_below) == (True, 3, 8)
    assert (p.want_band, p.band_radius, p.want_band_inter) == (True, 2, True)
    assert (p.want_edges, p.edge_t, p.want_edge_band, p.want_edge_inter) == (True, 0.5, True, True)
    assert p.rle_source == "sized" and p.sizes == SIZES and p.sized_level == 1 and p.gt is gt and p.gt_image == [0, 0, 1]
    assert MaskPost(who=who, n=2, K=3, side=320, masks="bits", min_area=4, rle="kept").rle_source == "kept_bits"
    assert tuple(p.fields()) == MaskPost.FIELDS and all(v is None for v in p.fields().values())
    assert set(MaskPost.FIELDS) <= set(engine.ClassHypotheses.__dataclass_fields__)


S = 64
PLANES = {"a host tensor": (torch.zeros(2, S * S // 8, dtype=torch.uint8), S, S),
          "int32": (torch.zeros(2, S * S // 8, dtype=torch.int32), S, S),
          "one dimension": (torch.zeros(2 * S * S // 8, dtype=torch.uint8), S, S),
          "W = S + 32": (torch.zeros(2, S * S // 8, dtype=torch.uint8), S, S + 32),
          "W no multiple of 32": (torch.zeros(2, S * 48 // 8, dtype=torch.uint8), S, 48),
          "H = True": (torch.zeros(2, S // 8, dtype=torch.uint8), True, S)}


@pytest.mark.parametrize("utility", ["mask_components", "mask_holes", "mask_morph", "mask_rle"])
@pytest.mark.parametrize("case", list(PLANES))
def test_utilities_on_packed_planes_refuse_bad_planes_under_their_own_name(utility, case):
    """The checks come before the engine's workspace or device is touched: an object with neither raises the ValueError."""
    bits, H, W = PLANES[case]
    with pytest.raises(ValueError, match="^" + utility + ": "):
        getattr(MaskUtilities(), utility)(bits, H, W)
