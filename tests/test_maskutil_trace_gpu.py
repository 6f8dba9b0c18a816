"""The stand-alone utilities of the packed-mask family (camouflaged_vlm_amd/maskpost.py: MaskUtilities), held from outside: every `hip`
call each of them makes -- name, order, the dtype and shape of each tensor argument, the value of each scalar, by parameter name --
against the record of the commit before their host code was restated (tests/golden/mask_util_launches.json,
tools/trace_mask_launches.py: record_utilities), never against a second run of the code under test.  Six ragged planes of at most
40 x 65, three packed planes of 64 x 64; the test never writes the record."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def tracer():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "trace_mask_launches.py")
    spec = importlib.util.spec_from_file_location("trace_mask_launches", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_utilities_launch_what_the_record_holds(tracer, golden_dir):
    with open(os.path.join(golden_dir, "mask_util_launches.json")) as f:
        want = json.load(f)
    got = json.loads(json.dumps(tracer.record_utilities(torch.device(DEV))))  # tuples and lists alike, as the file has them
    assert list(got["calls"]) == list(want["calls"]) and len(want["calls"]) >= 50
    for label in want["calls"]:
        a, b = tracer.readable(got, label), tracer.readable(want, label)
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        assert a == b, f"{label}: {len(a)} launches against {len(b)} recorded; the first difference at {first}: {a[first:first + 2]} against {b[first:first + 2]}"
    assert got["names"] == want["names"]
    launched = [label for label in want["calls"] if want["calls"][label]]
    assert set(want["calls"]) - set(launched) == {"concat", "mask_nms_sized no instance"}      # the two that launch nothing
