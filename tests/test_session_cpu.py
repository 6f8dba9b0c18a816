"""CPU: what Cascade.encode / Cascade.decode rest on that needs no GPU -- the export and the argument checks of
cvlm_expand_blocks (the launcher refuses before it touches a device), the pure request check of `decode`, and the text-row
oracle (tests/session_oracle.py) against the class oracle it generalises (tests/classes_oracle.py)."""
import os

import numpy as np
import pytest
import torch

from camouflaged_vlm_amd import hip, spec, synth
from camouflaged_vlm_amd.engine import decode_request
from oracle import cvlm_oracle as O
import classes_oracle as CO
import session_oracle as SO


def test_expand_blocks_is_exported_and_the_abi_stays():
    assert "cvlm_expand_blocks" in hip.EXPORTS and hip.ABI_VERSION == 12
    lib = hip.load()
    assert hasattr(lib, "cvlm_expand_blocks") and lib.cvlm_abi_version() == 12


def test_expand_blocks_refuses_bad_arguments_without_gpu():
    lib = hip.load()
    p = 4096
    ok = dict(image_of=p, P=7, B=3, n=4096, sf=p, df=p, shi=p, slo=p, dhi=p, dlo=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cvlm_expand_blocks(a["image_of"], a["P"], a["B"], a["n"], a["sf"], a["df"],
                                      a["shi"], a["slo"], a["dhi"], a["dlo"], None)
    none_h2 = dict(shi=None, slo=None, dhi=None, dlo=None)
    bad = [dict(image_of=None),
           # non-positive sizes
           dict(P=0), dict(P=-1), dict(B=0), dict(B=-2), dict(n=0), dict(n=-8), dict(P=65536),
           # no output set
           dict(none_h2, sf=None, df=None), dict(none_h2, df=None), dict(sf=None, df=None, dhi=None, dlo=None),
           # a source without its destination and the reverse
           dict(df=None), dict(sf=None),
           # one h2 plane without the other
           dict(dlo=None), dict(dhi=None), dict(slo=None), dict(shi=None), dict(sf=None, df=None, dlo=None),
           dict(sf=None, df=None, shi=None), dict(none_h2, dhi=p),
           # an output of 2^31 bytes or more: P * block_elems * 4
           dict(P=8, n=1 << 26), dict(P=1, n=1 << 29), dict(P=1, n=1 << 31), dict(P=1, n=1 << 62), dict(P=127, n=1 << 23, **none_h2),
           dict(P=64, n=1 << 23, sf=None, df=None)]
    for kw in bad:
        assert call(**kw) == -1, kw


def test_decode_request_accepts_and_rejects():
    B, n_cls, D = 2, 5, 8
    base = dict(same_engine=True, B=B, n_cls=n_cls, D=D)
    C2 = torch.tensor([[4, 0, 2], [3, 1, 0]], dtype=torch.int64)
    # accepted
    images, K, host = decode_request(**base, classes=C2)
    assert images == [0, 1] and K == 3 and torch.equal(host, C2) and host.device.type == "cpu"
    assert decode_request(**base, topk=1) == ([0, 1], 1, None)
    assert decode_request(**base, topk=np.int64(n_cls)) == ([0, 1], n_cls, None)
    assert decode_request(**base, text=torch.zeros(2, 4, D)) == ([0, 1], 4, None)
    images, K, host = decode_request(**base, classes=C2[[1, 1, 0]], images=[1, 1, 0])
    assert images == [1, 1, 0] and K == 3 and host.shape == (3, 3)
    assert decode_request(**base, topk=2, images=(1,)) == ([1], 2, None)
    assert decode_request(**base, topk=2, images=[np.int32(0), np.int64(1)]) == ([0, 1], 2, None)
    assert decode_request(**base, text=torch.zeros(1, 1, D), images=[0]) == ([0], 1, None)
    # rejected
    bad = [dict(base, same_engine=False, topk=1),
           # none or more than one of classes / topk / text
           dict(base), dict(base, topk=2, classes=C2), dict(base, topk=2, text=torch.zeros(2, 2, D)),
           dict(base, classes=C2, text=torch.zeros(2, 3, D)), dict(base, classes=C2, topk=3, text=torch.zeros(2, 3, D)),
           # topk
           dict(base, topk=0), dict(base, topk=n_cls + 1), dict(base, topk=1.0), dict(base, topk=True), dict(base, topk="2"),
           dict(base, n_cls=1025, topk=1),
           # classes: type, dtype, shape, range
           dict(base, classes=[[0, 1], [1, 0]]), dict(base, classes=C2.int()), dict(base, classes=C2.float()),
           dict(base, classes=torch.zeros(3, 2, dtype=torch.int64)), dict(base, classes=torch.zeros(2, dtype=torch.int64)),
           dict(base, classes=torch.zeros(2, 0, dtype=torch.int64)), dict(base, classes=torch.tensor([[0, n_cls], [0, 0]])),
           dict(base, classes=torch.tensor([[0, -1], [1, 1]])), dict(base, classes=C2, images=[0]),
           # text: type, dtype, shape
           dict(base, text=np.zeros((2, 2, D), np.float32)), dict(base, text=torch.zeros(2, 2, D, dtype=torch.float64)),
           dict(base, text=torch.zeros(2, 2, D, dtype=torch.float16)), dict(base, text=torch.zeros(2, D)),
           dict(base, text=torch.zeros(3, 2, D)), dict(base, text=torch.zeros(2, 2, D + 1)), dict(base, text=torch.zeros(2, 0, D)),
           dict(base, text=torch.zeros(2, 2, D), images=[0, 1, 1]),
           # images: a host sequence of ints in [0, B), non-empty
           dict(base, topk=1, images=[]), dict(base, topk=1, images=[2]), dict(base, topk=1, images=[0, -1]),
           dict(base, topk=1, images=torch.tensor([0, 1])), dict(base, topk=1, images=np.array([0, 1])), dict(base, topk=1, images=1),
           dict(base, topk=1, images=[0.0]), dict(base, topk=1, images=[True]), dict(base, topk=1, images="01"),
           dict(base, topk=1, images={0, 1})]
    for kw in bad:
        with pytest.raises(ValueError):
            decode_request(**kw)


@pytest.fixture(scope="module")
def gold(golden_dir):
    with np.load(os.path.join(golden_dir, "tiny_classes.npz")) as z:
        return {k: z[k] for k in z.files}


def test_text_oracle_with_bank_rows_is_the_class_oracle(gold):
    g, c = spec.TINY_SAM, spec.TINY_CLIP
    sd = O.to_torch_sd(synth.make_full_state_dict(g, c))
    inp, ci, cm = (torch.from_numpy(t) for t in synth.make_inputs(g, c, 2))
    classes = torch.tensor([[4, 0, 2], [3, 1, 1]], dtype=torch.int64)
    bank = torch.from_numpy(gold["bank_test"])
    with torch.no_grad():
        tf = O.clip_text_features(sd, c, gold["eot_test"].tolist())
        want = CO.infer_classes(inp, ci, cm, sd, g, c, tf, bank, classes=classes)
        got = SO.decode_text(inp, ci, cm, sd, g, c, tf, bank, CO.text_rows(tf, bank)[classes])
        sub = SO.decode_text(inp, ci, cm, sd, g, c, tf, bank, CO.text_rows(tf, bank)[classes[[1]]], images=[1])
    for k in ("pass1_logits", "low_masks", "low_edges", "masks", "edges", "logits", "pred"):
        assert torch.equal(got[k], want[k]), k
    # a subset of the images: the same arithmetic per prompt (the batch size changes the CPU GEMM blocking, not the mathematics)
    for k in ("low_masks", "low_edges", "logits"):
        assert float((sub[k] - want[k][1:2]).abs().max()) <= 1e-5 * max(1.0, float(want[k].abs().max())), k
    assert torch.equal(sub["pred"], want["pred"][1:2])
