"""CPU: the K-hypotheses oracle (tests/classes_oracle.py) against the reference's own K-prompt decoder call
(tests/golden/tiny_classes.npz, tools/make_classes_golden.py), and the argument checks of the two C-ABI entries behind
Cascade.infer_classes (no GPU needed: they refuse before launching)."""
import os

import numpy as np
import pytest
import torch

from camouflaged_vlm_amd import hip, spec, synth
from oracle import cvlm_oracle as O
import classes_oracle as CO


def d(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


@pytest.fixture(scope="module")
def gold(golden_dir):
    with np.load(os.path.join(golden_dir, "tiny_classes.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def oracle_run(gold):
    g, c = spec.TINY_SAM, spec.TINY_CLIP
    sd = O.to_torch_sd(synth.make_full_state_dict(g, c))
    inp, ci, cm = (torch.from_numpy(t) for t in synth.make_inputs(g, c, 2))
    with torch.no_grad():
        tf = O.clip_text_features(sd, c, gold["eot_test"].tolist())
        return CO.infer_classes(inp, ci, cm, sd, g, c, tf, torch.from_numpy(gold["bank_test"]),
                                classes=torch.from_numpy(gold["classes"]))


def test_golden_holds_every_class_of_the_tiny_bank(gold):
    B, K = gold["classes"].shape
    assert (B, K) == (2, spec.TINY_CLIP.n_cls_test)
    assert all(sorted(row) == list(range(K)) for row in gold["classes"].tolist())
    # hypothesis 0 is pass 1's argmax; the reference's K-prompt call reproduced its own one-prompt infer_test
    assert (gold["classes"][:, 0] == gold["pass1_logits"].argmax(1)).all()
    assert float(gold["hyp0_vs_infer_test"].max()) <= 1e-4


def test_oracle_reproduces_reference_hypotheses(oracle_run, gold):
    r = oracle_run
    dm = d(r["low_masks"], gold["low_masks"])
    de = d(r["low_edges"], gold["low_edges"])
    pos = gold["pos"]
    B, K = gold["classes"].shape
    df = d(r["masks"].reshape(B, K, -1)[:, :, pos], gold["masks_at_pos"])
    d1 = d(r["pass1_logits"], gold["pass1_logits"])
    dl = d(r["logits"], gold["class_logits"])
    print(f"oracle vs reference: low masks {dm:.2e}, low edges {de:.2e}, full-res masks {df:.2e}, pass-1 logits {d1:.2e}, "
          f"stage-2 logits {dl:.2e}")
    # 1e-5 of each array's scale (|low-res mask logits| reach 16 here): the reference's own K-prompt and one-prompt decoder calls
    # already differ by 1.4e-5 (tiny_classes.npz: hyp0_vs_infer_test)
    for v, ref in ((dm, gold["low_masks"]), (de, gold["low_edges"]), (df, gold["masks_at_pos"]), (d1, gold["pass1_logits"]),
                   (dl, gold["class_logits"])):
        assert v <= 1e-5 * max(1.0, float(np.abs(ref).max()))
    assert np.array_equal(r["pred"].numpy(), gold["pred"])
    # topk through the oracle gives the golden's order (its pass-1 logits are well separated)
    assert np.array_equal(torch.topk(r["pass1_logits"], K, dim=1).indices.numpy(), gold["classes"])


def _lib():
    return hip.load()


def test_mask_head_edge_refuses_bad_arguments_without_gpu():
    lib = _lib()
    p = 4096
    ok = dict(up=p, edge=p, hyper=p, P=2, HW=64, Cc=32, low=p, ep=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cvlm_mask_head_edge(a["up"], a["edge"], a["hyper"], a["P"], a["HW"], a["Cc"],
                                       a["low"], a["ep"], None)
    for kw in (dict(up=None), dict(edge=None), dict(hyper=None), dict(low=None), dict(ep=None), dict(P=0), dict(P=65536),
               dict(HW=0), dict(Cc=0), dict(Cc=30)):
        assert call(**kw) == -1, kw


def test_topk_select_refuses_bad_arguments_without_gpu():
    lib = _lib()
    p = 4096
    ok = dict(logits=p, B=2, Cc=5, K=3, txt=p, D=8, idx_in=None, idx_out=p, sel=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cvlm_topk_select(a["logits"], a["B"], a["Cc"], a["K"], a["txt"], a["D"],
                                    a["idx_in"], a["idx_out"], a["sel"], None)
    for kw in (dict(logits=None), dict(txt=None), dict(idx_out=None), dict(sel=None), dict(B=0), dict(Cc=0), dict(K=0),
               dict(K=6), dict(D=0), dict(D=6), dict(Cc=1025, K=3)):
        assert call(**kw) == -1, kw
    # gather only: logits may be NULL and K may exceed C (repeated classes); still a bad D is refused
    assert call(logits=None, idx_in=p, K=6, D=6) == -1
