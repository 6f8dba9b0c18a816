"""The plan of the packed outputs of Cascade.infer_classes / decode (camouflaged_vlm_amd/maskpost.py: MaskPost), held from outside:
the launches of six calls -- every `hip` call by name and order, the packed-mask family's with its argument shapes and values --
against the record of the commit before the plan existed (tests/golden/mask_post_launches.json, tools/trace_mask_launches.py),
never against a second run of the code under test; and the independence the options promise: the call with everything on returns,
in every field it shares with a call that asks for one option alone, the same bytes, floats included.  Tiny geometry, chunks of 4
prompts at K = 3, so that a chunk crosses the image boundary."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from test_classes_gpu import build_tiny
from test_gt_gpu import CLASSES, OTHER, SIZES, annotations

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def tracer():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "trace_mask_launches.py")
    spec = importlib.util.spec_from_file_location("trace_mask_launches", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_launches_equal_the_recorded_ones(tracer, golden_dir):
    with open(os.path.join(golden_dir, "mask_post_launches.json")) as f:
        want = json.load(f)
    got = json.loads(json.dumps(tracer.record(torch.device(DEV))))           # tuples and lists alike, as the file has them
    assert list(got["calls"]) == list(want["calls"]) and len(want["calls"]) == 6
    for label in want["calls"]:
        a, b = tracer.readable(got, label), tracer.readable(want, label)
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        assert a == b, f"{label}: {len(a)} launches against {len(b)} recorded; the first difference at {first}: {a[first:first + 2]} against {b[first:first + 2]}"
        assert sum(" " in line for line in b) >= 2, label                    # the packed-mask family is in every record: one mask_head_* per chunk at least
    assert got["names"] == want["names"]


# ---- everything at once equals each alone --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(golden_dir):
    with np.load(os.path.join(golden_dir, "tiny_classes.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def tiny():
    from camouflaged_vlm_amd import spec, synth
    g, c = spec.TINY_SAM, spec.TINY_CLIP
    inp, ci, cm = synth.make_inputs(g, c, batch=2)
    dev = torch.device(DEV)
    return g, c, synth.make_full_state_dict(g, c), tuple(torch.from_numpy(t).to(dev) for t in (inp, ci, cm)), dev


@pytest.fixture(scope="module")
def cas(tiny, gold):
    return build_tiny(tiny, gold)


EVERYTHING = dict(masks="both", overlaps=True, quality=True, components=2, min_area=16, holes=2, fill_holes=16, band=2, edge_threshold=0.5)
NESTED = {"sized": ("bits", "offsets", "area", "box", "status"), "rle": ("counts", "offsets", "n_runs", "status"),
          "gt_overlaps": ("pairs", "inter", "area_a", "area_b", "status")}


def tensors_of(h) -> dict:
    """Every tensor of a ClassHypotheses by its dotted name."""
    out = {f: getattr(h, f) for f in OTHER if getattr(h, f) is not None}
    for obj, fields in NESTED.items():
        if getattr(h, obj) is not None:
            out.update({f"{obj}.{f}": getattr(getattr(h, obj), f) for f in fields})
    return out


def alone(gt):
    """One option, or one option with what it needs, per call."""
    return {"both": dict(masks="both"), "overlaps": dict(masks="bits", overlaps=True), "quality": dict(masks="bits", quality=True),
            "components": dict(masks="bits", components=2, min_area=16), "holes": dict(masks="bits", holes=2, fill_holes=16),
            "band": dict(masks="bits", band=2), "band overlaps": dict(masks="bits", band=2, overlaps=True),
            "edges": dict(masks="bits", edge_threshold=0.5), "edges on the band": dict(masks="bits", edge_threshold=0.5, band=2),
            "edges overlaps": dict(masks="bits", edge_threshold=0.5, overlaps=True),
            "sized": dict(masks="bits", sizes=gt["sizes"]), "rle sized": dict(masks="bits", sizes=gt["sizes"], rle="sized"),
            "ground truth": dict(masks="bits", sizes=gt["sizes"], ground_truth=gt["ground_truth"])}


def check_everything_equals_each_alone(cas, call, sizes, ids):
    gt = cas.rle_decode(annotations(sizes, ids)[1])
    gt.check()
    gt = dict(sizes=sizes, ground_truth=(gt, ids))
    full = call(rle="sized", **gt, **EVERYTHING)
    torch.cuda.synchronize()
    want = {k: v.clone() for k, v in tensors_of(full).items()}
    assert set(want) == set(OTHER) | {f"{o}.{f}" for o, fs in NESTED.items() for f in fs}      # everything on: every field is there
    assert int(full.area.max()) > 0 and int(full.gt_overlaps.inter.max()) > 0 and int(full.sized.area.max()) > 0
    full.rle.check(), full.sized.check(), full.gt_overlaps.check()
    seen = set()
    for name, kw in alone(gt).items():
        one = tensors_of(call(**kw))
        torch.cuda.synchronize()
        for f, t in one.items():
            assert t.dtype == want[f].dtype and t.shape == want[f].shape and \
                torch.equal(t.contiguous().view(torch.uint8), want[f].contiguous().view(torch.uint8)), (name, f)
        seen |= set(one)
    assert seen == set(want), set(want) - seen
    # the other source of rle=: everything on with the despeckled planes encoded against that option alone
    kept = tensors_of(call(rle="kept", **gt, **EVERYTHING))
    one = tensors_of(call(masks="bits", min_area=16, rle="kept"))
    torch.cuda.synchronize()
    assert {"rle.counts", "kept_bits"} <= set(one)
    for f, t in one.items():
        assert torch.equal(t.contiguous().view(torch.uint8), kept[f].contiguous().view(torch.uint8)), ("rle kept", f)
    for f in set(kept) - {f for f in kept if f.startswith("rle.")}:
        assert torch.equal(kept[f].contiguous().view(torch.uint8), want[f].contiguous().view(torch.uint8)), ("everything, rle kept", f)


def test_infer_classes_everything_equals_each_alone(tiny, cas, monkeypatch):
    _, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    classes = torch.tensor(CLASSES)
    check_everything_equals_each_alone(cas, lambda **kw: cas.infer_classes(inp, ci, cm, classes=classes, **kw), SIZES, [0, 0, 1])


def test_decode_everything_equals_each_alone(tiny, cas, monkeypatch):
    _, _, _, (inp, ci, cm), _ = tiny
    monkeypatch.setattr(cas, "class_chunk", lambda: 4)
    enc = cas.encode(inp, ci, cm)
    sizes = [SIZES[1], SIZES[0], SIZES[1]]                                        # one per decoded row
    check_everything_equals_each_alone(cas, lambda **kw: cas.decode(enc, topk=3, images=[1, 0, 1], **kw), sizes, [1, 1, 2])
