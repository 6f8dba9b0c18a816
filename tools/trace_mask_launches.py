"""The launches of Cascade.infer_classes / decode, option by option, as a record: tiny geometry, batch 2, K = 3, chunks of 4 prompts (a
chunk crosses the image boundary).  Every public function of the `hip` module but the `*_bytes` size queries and `load` (the library
handle, fetched by every launch) is wrapped by a recorder that still calls through; six calls run -- the default, masks="bits",
everything on with rle="sized" and with rle="kept", and on an encoded batch `decode` with everything on and with stage2=False,
rle="filled".  Of every recorded call the name is kept, in order; of the packed-mask family (`mask_*`, `edge_pack*`) also the shape and
dtype of each tensor argument and the value of each int / float argument, by parameter name -- but not the length of `counts`, which
the masks' bits decide, not the call.  tests/test_maskpost_trace_gpu.py holds the tree under test to the record in
tests/golden/mask_post_launches.json: a refactor of the host code leaves it as it is; a change of the launch schedule re-records it.
`record_utilities` is the same for the stand-alone utilities (maskpost.MaskUtilities), every call in the detailed form, held by
tests/test_maskutil_trace_gpu.py to tests/golden/mask_util_launches.json.
Usage: python tools/trace_mask_launches.py OUT.json [utilities]"""
import inspect
import json
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from camouflaged_vlm_amd import hip, spec, synth  # noqa: E402
from camouflaged_vlm_amd.engine import Cascade, Precision  # noqa: E402

SIZES = [(213, 320), (480, 641)]
CLASSES = [[0, 1, 2], [2, 1, 0]]
IMAGES = [1, 0, 1]
EVERYTHING = dict(masks="both", overlaps=True, quality=True, components=2, min_area=16, holes=2, fill_holes=16, band=2, edge_threshold=0.5)


def disc(h: int, w: int, cy: float, cx: float, r: float) -> np.ndarray:
    yy, xx = np.mgrid[0:h, 0:w]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def run_counts(plane: np.ndarray) -> np.ndarray:
    """bool (H, W) -> COCO run counts: column-major, alternating, starting with the 0s."""
    f = np.ascontiguousarray(plane.astype(np.int8).T).reshape(-1)
    t = np.flatnonzero(np.diff(f, prepend=np.int8(0)))
    return np.diff(np.concatenate([t, [f.size]]), prepend=0).astype(np.int64)


def annotations(sizes, ids) -> list:
    """tests/test_gt_gpu.py's: two discs and a rectangle, one per entry of ids, each at the size of its image, as COCO dicts."""
    coco = []
    for n, b in enumerate(ids):
        h, w = sizes[b]
        if n == 1:
            m = np.zeros((h, w), dtype=bool)
            m[h // 5:h // 2, w // 4:w - 7] = True
        else:
            m = disc(h, w, h * (0.4 + 0.1 * n), w * 0.5, min(h, w) * (0.45 - 0.1 * n))
        coco.append({"size": [h, w], "counts": run_counts(m).tolist()})
    return coco


def build_tiny(dev):
    """The engine and the inputs of the GPU tests (tests/test_classes_gpu.py: build_tiny), class_chunk() = 4."""
    g, c = spec.TINY_SAM, spec.TINY_CLIP
    with np.load(os.path.join(REPO, "tests", "golden", "tiny_classes.npz")) as z:
        eot, bank = z["eot_test"].tolist(), torch.from_numpy(z["bank_test"])
    cas = Cascade({k: torch.from_numpy(v) for k, v in synth.make_full_state_dict(g, c).items()}, g, c, dev, Precision.named("exact"))
    cas.clip.set_text_bank(cas.clip.text_features(eot, "test"), bank, "test")
    cas.class_chunk = lambda: 4
    return cas, tuple(torch.from_numpy(t).to(dev) for t in synth.make_inputs(g, c, batch=2))


def describe(v, name: str = ""):
    if isinstance(v, torch.Tensor):                                  # the run counts' length is a function of the masks' bits, not of the call
        return [str(v.dtype).replace("torch.", ""), None if name == "counts" else list(v.shape)]
    if isinstance(v, (bool, int, float)) or v is None:
        return v
    return type(v).__name__


class Recorder:
    """`with Recorder() as log:` -- log is the list of calls made through the `hip` module meanwhile: a name, or for the packed-mask
    family [name, {parameter: description}].  Recorder(everything=True) keeps every call in the detailed form."""

    def __init__(self, everything: bool = False):
        self.everything = everything

    def __enter__(self):
        self.log, self.saved = [], {}
        for name, fn in list(vars(hip).items()):
            if name == "load" or name.startswith("_") or name.endswith("_bytes"):   # the library handle, helpers, size queries: no launches
                continue
            if isinstance(fn, types.FunctionType) and fn.__module__ == hip.__name__:
                self.saved[name] = fn
                setattr(hip, name, self.wrap(name, fn))
        return self.log

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(hip, name, fn)

    def wrap(self, name, fn):
        detailed = self.everything or name.startswith("mask_") or name.startswith("edge_pack")
        sig = inspect.signature(fn)

        def recorded(*a, **k):
            if detailed:
                bound = sig.bind(*a, **k)
                bound.apply_defaults()
                self.log.append([name, {p: describe(v, p) for p, v in bound.arguments.items()}])
            else:
                self.log.append(name)
            return fn(*a, **k)
        return recorded


def record(dev) -> dict:
    """{"names": the names met, "calls": {label: the launches of that call}}; a launch is an index into names, or for the packed-mask
    family [index, {parameter: description}]."""
    cas, (inp, ci, cm) = build_tiny(dev)
    classes = torch.tensor(CLASSES)
    gt = cas.rle_decode(annotations(SIZES, [0, 0, 1]))
    dec_sizes = [SIZES[i] for i in IMAGES]
    dec_gt = cas.rle_decode(annotations(dec_sizes, [0, 0, 1]))
    enc = cas.encode(inp, ci, cm)
    torch.cuda.synchronize()
    runs = {
        "infer_classes": lambda: cas.infer_classes(inp, ci, cm, classes=classes),
        "infer_classes bits": lambda: cas.infer_classes(inp, ci, cm, classes=classes, masks="bits"),
        "infer_classes everything, rle sized": lambda: cas.infer_classes(inp, ci, cm, classes=classes, sizes=SIZES, rle="sized",
                                                                         ground_truth=(gt, [0, 0, 1]), **EVERYTHING),
        "infer_classes everything, rle kept": lambda: cas.infer_classes(inp, ci, cm, classes=classes, sizes=SIZES, rle="kept",
                                                                        ground_truth=(gt, [0, 0, 1]), **EVERYTHING),
        "decode everything": lambda: cas.decode(enc, images=IMAGES, topk=3, sizes=dec_sizes, rle="sized", ground_truth=(dec_gt, [0, 0, 1]),
                                                **EVERYTHING),
        "decode bits without stage 2": lambda: cas.decode(enc, images=IMAGES, topk=3, stage2=False, masks="bits", rle="filled", fill_holes=16),
    }
    return run_recorded(runs)


def run_recorded(runs: dict, everything: bool = False) -> dict:
    """Each of `runs` under a Recorder -> {"names": the names met, "calls": {label: its launches}}."""
    names, calls = [], {}
    for label, run in runs.items():
        with Recorder(everything) as log:
            run()
            torch.cuda.synchronize()
        out = []
        for entry in log:
            name = entry if isinstance(entry, str) else entry[0]
            if name not in names:
                names.append(name)
            out.append(names.index(name) if isinstance(entry, str) else [names.index(name), entry[1]])
        calls[label] = out
    return {"names": names, "calls": calls}


UTILITY_SIZES = [(1, 1), (5, 33), (7, 31), (3, 70), (40, 65), (1, 32)]      # a width below, at and above a word; a single pixel
UTILITY_SEED = 20261021


def record_utilities(dev) -> dict:
    """The launches of the stand-alone utilities (maskpost.MaskUtilities), every public method once per host path, as `record` has
    those of infer_classes / decode, every call in the detailed form: six ragged planes on two sides a and b (detections and
    annotations: one random fill each, one plane of b all clear), three packed planes of 64 x 64, label maps of two images with two
    hypotheses each.  The contours and the surface distances also run with maskpost.RLE_WS_CAP at 512 bytes, so that the host cuts
    several rounds.  The planes are seeded: the lengths that the bits decide (`xy`, `ring_start`, `inter`) are part of the record."""
    from camouflaged_vlm_amd import maskpost
    from camouflaged_vlm_amd.engine import Workspace
    from camouflaged_vlm_amd.maskpost import SizedMasks

    class Engine(maskpost.MaskUtilities):
        """The two attributes the utilities use of an engine."""

        def __init__(self):
            self.device, self.ws = dev, Workspace(dev)

    eng = Engine()
    rng = np.random.default_rng(UTILITY_SEED)
    P = len(UTILITY_SIZES)
    fills = [[rng.random(s) < 0.6 for s in UTILITY_SIZES] for _ in range(2)]
    fills[1][2][:] = False
    coco = [[{"size": list(m.shape), "counts": run_counts(m).tolist()} for m in side] for side in fills]
    a, b = eng.rle_decode(coco[0]), eng.rle_decode(coco[1])
    both = SizedMasks.concat([a, b])
    ids, same = list(range(P)), [(p, p) for p in range(P)]
    logits = torch.from_numpy(rng.standard_normal((3, 64, 64)).astype(np.float32)).to(dev)
    prob = torch.sigmoid(logits)
    bits, _, _ = eng.pack_masks(logits)
    band = eng.mask_morph(bits, 64, 64).band_bits
    small = torch.from_numpy(rng.standard_normal((P, 16, 16)).astype(np.float32)).to(dev)
    map_sizes, K = [(5, 33), (7, 31)], 2
    labels = [[1, 2], [3, 4]]
    maps = eng.label_maps(small[:4], map_sizes, K=K)
    cats = maps.categories(labels)
    n_pix = sum(h * w for h, w in map_sizes)
    truth = rng.integers(0, 5, n_pix).astype(np.int32)
    raw = [rng.choice([0, 1, 2], size=map_sizes[0]).astype(np.int32), rng.choice([0, 7, 9, 5], size=map_sizes[1]).astype(np.int32)]
    rgb = [np.stack([r & 255, (r >> 8) & 255, (r >> 16) & 255], axis=-1).astype(np.uint8) for r in raw]
    segments = [[(1, 1, 0), (2, 2, 0)], [(7, 3, 0), (9, 4, 1)]]
    pan = eng.panoptic_remap(raw, map_sizes, segments)
    pred, pred_cat = maps.pq_inputs(labels)
    pq = lambda **kw: eng.panoptic_quality(pred, pred_cat, pan.gt, pan.gt_cat, pan.gt_crowd, map_sizes, num_classes=5, **kw)
    polys = [{"size": [5, 33], "polygons": [[1, 1, 20, 1, 20, 4, 1, 4]]},
             {"size": [40, 65], "polygons": [[2, 2, 60, 3, 30, 38], [5.5, 20, 12.25, 20, 12.25, 30.5, 5.5, 30.5]]}]
    scores = np.linspace(0.9, 0.1, 2 * P).astype(np.float32).tolist()
    category = [0, 1] * P
    none = SizedMasks(bits=torch.empty(0, dtype=torch.uint8, device=dev), offsets=torch.zeros(1, dtype=torch.int64, device=dev),
                      area=torch.empty(0, dtype=torch.int32, device=dev), box=torch.empty(0, 4, dtype=torch.int32, device=dev),
                      status=torch.zeros(1, dtype=torch.int32, device=dev), sizes=[], level=0)
    images = maskpost.sized_images([rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in UTILITY_SIZES], dev)
    levels = torch.from_numpy(rng.integers(0, 256, (1, 5, 33)).astype(np.uint8)).to(dev)
    layers = [[maskpost.fill(a, p, color=(255, 0, 0))] for p in range(P)]
    layers[1].append(maskpost.heat(levels, 0, lut=maskpost.palette(256), alpha=0.5))
    match = dict(scores=scores[:P], det_image=ids, gt_image=ids)
    torch.cuda.synchronize()

    rounds = {}                                                       # label -> (the launch each round makes, how many at least)

    def capped(label: str, run, launch: str, at_least: int):
        """`run` with RLE_WS_CAP at 512 bytes, so that the host cuts it into rounds: `launch` must be met at_least times."""
        def go():
            keep, maskpost.RLE_WS_CAP = maskpost.RLE_WS_CAP, 512
            try:
                run()
            finally:
                maskpost.RLE_WS_CAP = keep
        rounds[label] = (launch, at_least)
        return go

    runs = {
        "pack_masks": lambda: eng.pack_masks(logits),
        "mask_components": lambda: eng.mask_components(bits, 64, 64, components=2, min_area=4),
        "mask_holes": lambda: eng.mask_holes(bits, 64, 64, holes=2, fill_holes=4, connectivity=4),
        "mask_morph": lambda: eng.mask_morph(bits, 64, 64, radius=2, dilate=True, erode=True),
        "mask_rle": lambda: eng.mask_rle(bits, 64, 64),
        "pack_edges": lambda: eng.pack_edges(prob, threshold=0.5),
        "pack_edges resized, with_bits": lambda: eng.pack_edges(prob[:, ::2, ::2].contiguous(), (64, 64), threshold=0.25, with_bits=band),
        "rle_decode list": lambda: eng.rle_decode(coco[0]),
        "rle_decode list, stats=False": lambda: eng.rle_decode(coco[1], stats=False),
        "rle_decode MaskRle": lambda: eng.rle_decode(eng.mask_rle_sized(a)),
        "polygons_decode": lambda: eng.polygons_decode(polys),
        "mask_rle_sized": lambda: eng.mask_rle_sized(b),
        "concat": lambda: SizedMasks.concat([a, b]),
        "pack_masks_sized": lambda: eng.pack_masks_sized(small, UTILITY_SIZES, level=1),
        "mask_inter_sized pairs": lambda: eng.mask_inter_sized(a, b, pairs=same),
        "mask_inter_sized image ids": lambda: eng.mask_inter_sized(a, b, a_image=ids, b_image=ids),
        "mask_inter_sized b is a": lambda: eng.mask_inter_sized(a, a, pairs=same),
        "mask_boundary_sized ratio": lambda: eng.mask_boundary_sized(a),
        "mask_boundary_sized radius": lambda: eng.mask_boundary_sized(a, radius=1),
        "mask_boundary_sized radius per plane": lambda: eng.mask_boundary_sized(b, radius=[1, 2, 1, 1, 3, 1]),
        "mask_contours_sized": lambda: eng.mask_contours_sized(a),
        "mask_contours_sized capped": capped("mask_contours_sized capped", lambda: eng.mask_contours_sized(a, connectivity=4), "mask_contour_emit", 2),
        "mask_distance_sized": lambda: eng.mask_distance_sized(a),
        "mask_distance_sized reach per plane": lambda: eng.mask_distance_sized(b, reach=[0, 1, 2, 3, 4, 5]),
        "mask_surface_distances": lambda: eng.mask_surface_distances(a, b),
        "mask_surface_distances surface=None": lambda: eng.mask_surface_distances(a, b, surface=None, tolerance=[1, 0.1]),
        "mask_surface_distances reach=tolerance": lambda: eng.mask_surface_distances(a, b, pairs=[(4, 4), (1, 1)], reach="tolerance"),
        "mask_surface_distances capped": capped("mask_surface_distances capped", lambda: eng.mask_surface_distances(a, b), "mask_surface_totals", 4),
        "mask_surface_distances surface=None capped": capped("mask_surface_distances surface=None capped", lambda: eng.mask_surface_distances(a, a, surface=None), "mask_surface_totals", 4),
        "mask_thin_sized": lambda: eng.mask_thin_sized(a),
        "mask_thin_sized max_iter per plane": lambda: eng.mask_thin_sized(a, max_iter=[1, 2, 3, 1, 2, 1]),
        "mask_thin_sized steps": lambda: eng.mask_thin_sized(a, path="steps", steps=1),
        "mask_cldice": lambda: eng.mask_cldice(a, b),
        "mask_cldice image ids": lambda: eng.mask_cldice(a, a, a_image=ids, b_image=ids),
        "mask_regions_sized, compact": lambda: eng.mask_regions_sized(a, regions=2, min_area=1, connectivity=4).compact(),
        "mask_nms_sized greedy": lambda: eng.mask_nms_sized(both, scores=scores, image=ids + ids),
        "mask_nms_sized gaussian, category on the device": lambda: eng.mask_nms_sized(
            both, scores=torch.tensor(scores, device=dev), image=ids + ids, category=torch.tensor(category, device=dev), method="gaussian"),
        "mask_nms_sized category on the host": lambda: eng.mask_nms_sized(both, scores=scores, image=ids + ids, category=category, measure="min"),
        "mask_nms_sized no instance": lambda: eng.mask_nms_sized(none, scores=[], image=[]),
        "label_maps": lambda: eng.label_maps(small[:4], map_sizes, K=K),
        "label_maps weights": lambda: eng.label_maps(small[:4], map_sizes, K=K, weights=[1.0, 0.5, 0.25, 2.0], level=64, overlap_threshold=0.5),
        "LabelMaps.categories": lambda: maps.categories(labels, which="segment"),
        "LabelMaps.panoptic": lambda: maps.panoptic(),
        "LabelMaps.pq_inputs": lambda: maps.pq_inputs(labels),
        "label_iou": lambda: eng.label_iou(cats, truth, num_classes=5),
        "label_iou totals": lambda: eng.label_iou(cats, truth, num_classes=5, totals=eng.label_iou(cats, truth, num_classes=5)),
        "panoptic_remap": lambda: eng.panoptic_remap(raw, map_sizes, segments),
        "panoptic_remap rgb": lambda: eng.panoptic_remap(rgb, map_sizes, segments, rgb=True),
        "panoptic_quality": lambda: pq(),
        "panoptic_quality totals": lambda: pq(totals=pq()),
        "render": lambda: eng.render(images, layers),
        "render_overlay": lambda: eng.render_overlay(images, a, image_of=ids, outline=1),
        "coco_match": lambda: eng.coco_match(a, b, **match),
        "coco_match boundary": lambda: eng.coco_match(a, b, boundary=0.02, iscrowd=[0, 1, 0, 0, 0, 0], **match),
        "coco_match no annotation": lambda: eng.coco_match(a, None, scores=scores[:P], det_image=ids, gt_image=[]),
    }
    trace = run_recorded(runs, everything=True)
    for label, (launch, at_least) in rounds.items():
        met = sum(trace["names"][e[0]] == launch for e in trace["calls"][label])
        assert met >= at_least, f"{label}: {met} {launch} launches under a cap of 512 bytes, {at_least} at least were expected"
    return trace


def readable(trace: dict, label: str) -> list:
    """The launches of one call with the names written out, one string each."""
    names = trace["names"]
    return [names[e] if isinstance(e, int) else f"{names[e[0]]} {json.dumps(e[1], sort_keys=True)}" for e in trace["calls"][label]]


if __name__ == "__main__":
    trace = (record_utilities if sys.argv[2:] == ["utilities"] else record)(torch.device("cuda:0"))
    with open(sys.argv[1], "w") as f:
        f.write("{\"names\": " + json.dumps(trace["names"]) + ",\n \"calls\": {\n" +
                ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in trace["calls"].items()) + "\n }}\n")
    print({k: len(v) for k, v in trace["calls"].items()}, os.path.getsize(sys.argv[1]), "bytes")
