"""The launches of Cascade.infer_classes / decode, option by option, as a record: tiny geometry, batch 2, K = 3, chunks of 4 prompts (a
chunk crosses the image boundary).  Every public function of the `hip` module but the `*_bytes` size queries and `load` (the library
handle, fetched by every launch) is wrapped by a recorder that still calls through; six calls run -- the default, masks="bits",
everything on with rle="sized" and with rle="kept", and on an encoded batch `decode` with everything on and with stage2=False,
rle="filled".  Of every recorded call the name is kept, in order; of the packed-mask family (`mask_*`, `edge_pack*`) also the shape and
dtype of each tensor argument and the value of each int / float argument, by parameter name -- but not the length of `counts`, which
the masks' bits decide, not the call.  tests/test_maskpost_trace_gpu.py holds the tree under test to the record in
tests/golden/mask_post_launches.json: a refactor of the host code leaves it as it is; a change of the launch schedule re-records it.
Usage: python tools/trace_mask_launches.py OUT.json"""
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
    family [name, {parameter: description}]."""

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
        detailed = name.startswith("mask_") or name.startswith("edge_pack")
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
    names, calls = [], {}
    for label, run in runs.items():
        with Recorder() as log:
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


def readable(trace: dict, label: str) -> list:
    """The launches of one call with the names written out, one string each."""
    names = trace["names"]
    return [names[e] if isinstance(e, int) else f"{names[e[0]]} {json.dumps(e[1], sort_keys=True)}" for e in trace["calls"][label]]


if __name__ == "__main__":
    trace = record(torch.device("cuda:0"))
    with open(sys.argv[1], "w") as f:
        f.write("{\"names\": " + json.dumps(trace["names"]) + ",\n \"calls\": {\n" +
                ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in trace["calls"].items()) + "\n }}\n")
    print({k: len(v) for k, v in trace["calls"].items()}, os.path.getsize(sys.argv[1]), "bytes")
