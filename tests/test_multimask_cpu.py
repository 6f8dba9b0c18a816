"""CPU: the multimask oracle (tests/multimask_oracle.py) against the reference's own `predict_masks` call
(tests/golden/tiny_multimask.npz, tools/make_multimask_golden.py), and the argument checks of cvlm_mask_head_multi (no GPU needed:
it refuses before launching)."""
import os

import numpy as np
import pytest
import torch

from camouflaged_vlm_amd import hip, spec, synth
from oracle import cvlm_oracle as O
import multimask_oracle as MO


def d(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


@pytest.fixture(scope="module")
def gold(golden_dir):
    with np.load(os.path.join(golden_dir, "tiny_multimask.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def oracle_run(gold):
    g, c = spec.TINY_SAM, spec.TINY_CLIP
    sd = O.to_torch_sd(synth.make_full_state_dict(g, c))
    inp, ci, cm = (torch.from_numpy(t) for t in synth.make_inputs(g, c, 2))
    with torch.no_grad():
        tf = O.clip_text_features(sd, c, gold["eot_test"].tolist())
        return MO.infer_test_multimask(inp, ci, cm, sd, g, c, tf, torch.from_numpy(gold["bank_test"])), (inp, ci, cm, sd, g, c, tf)


def test_golden_holds_four_distinct_masks_and_scores(gold):
    G = spec.TINY_SAM.grid
    assert gold["low_masks"].shape == (2, 4, 4 * G, 4 * G) and gold["low_edges"].shape == (2, 4 * G, 4 * G)
    assert gold["iou"].shape == (2, 4) and gold["masks_at_pos"].shape == (2, 4, gold["pos"].size)
    # the reference's predict_masks call reproduced the decoder call of its own infer_test in slice 0
    assert float(gold["slice0_vs_infer_test"].max()) <= 1e-4
    # four masks that say different things, none of them empty or full, and scores that tell them apart
    for b in range(2):
        frac = [(gold["low_masks"][b, m] > 0).mean() for m in range(4)]
        assert all(0.1 < f < 0.9 for f in frac), frac
        s = np.sort(gold["iou"][b])
        assert float(np.diff(s).min()) > 2e-3 * float(np.abs(gold["iou"]).max())


def test_oracle_reproduces_reference_multimask(oracle_run, gold):
    r, _ = oracle_run
    pos = gold["pos"]
    rows = (("low masks", r["low_masks"], gold["low_masks"]), ("low edges", r["low_edges"], gold["low_edges"]),
            ("iou_pred", r["iou"], gold["iou"]), ("full-res masks", r["masks"].reshape(2, 4, -1)[:, :, pos], gold["masks_at_pos"]),
            ("pass-1 logits", r["pass1_logits"], gold["pass1_logits"]))
    print("oracle vs reference: " + ", ".join(f"{n} {d(a, b):.2e}" for n, a, b in rows))
    # 1e-5 of each array's scale, the rule of tests/test_classes_cpu.py
    for n, a, ref in rows:
        assert d(a, ref) <= 1e-5 * max(1.0, float(np.abs(ref).max())), n


def test_oracle_slice_zero_is_the_one_mask_oracle(oracle_run, gold):
    """The restated tail returns in slice 0 what oracle.cvlm_oracle.infer_test computes."""
    r, (inp, ci, cm, sd, g, c, tf) = oracle_run
    with torch.no_grad():
        one = O.infer_test(inp, ci, cm, sd, g, c, tf, torch.from_numpy(gold["bank_test"]))
    assert torch.equal(one[:, 0], r["masks"][:, 0])


def test_mask_head_multi_refuses_bad_arguments_without_gpu():
    lib = hip.load()
    p = 4096
    ok = dict(up=p, edge=p, hyper=p, P=2, HW=64, Cc=32, n=4, low=p, ep=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cvlm_mask_head_multi(a["up"], a["edge"], a["hyper"], a["P"], a["HW"], a["Cc"],
                                        a["n"], a["low"], a["ep"], None)
    for kw in (dict(up=None), dict(hyper=None), dict(low=None), dict(edge=None), dict(n=0), dict(n=5), dict(n=-1), dict(P=0),
               dict(P=65536), dict(HW=0), dict(Cc=0), dict(Cc=30), dict(Cc=-4)):
        assert call(**kw) == -1, kw                          # edge=None with an edge_prob pointer: nothing to write it from
    assert call(Cc=64) == -2                                 # rows of more than 60 floats: CVLM_E_UNSUPPORTED, nothing launched
    assert "cvlm_mask_head_multi" in hip.EXPORTS and hip.ABI_VERSION == 12
