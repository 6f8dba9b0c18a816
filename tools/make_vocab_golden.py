#!/usr/bin/env python3
"""Golden vectors of a class vocabulary larger than the kernels' former 1024-class cap, made by running the REFERENCE's own modules
on CPU (build container only; tools/make_golden.py's loader).

The reference fixes its vocabulary at construction: CustomCLIP tokenises the class names, embeds them and keeps prefix / suffix
buffers (cocotrainers/mapleAlphaCLIP.py:132-168).  Here it is constructed over N = 1100 names -- pairs "a b" of the packaged OVCamo
test names, through the reference's own tokenizer --, its token_prefix_test / token_suffix_test are set to table[ids] for the
synthetic embedding table synth.make_tensor("openai.token_embedding.weight", ...), and its bank to synth.make_text_bank(N, 768,
"test"); everything else is the tiny synthetic model of tools/make_golden.py.  Per image (0-1 of synth.make_inputs): pass 1 over all
N classes, the top 8 classes, and for the K = 2 leading hypotheses the K-prompt decoder call and stage 2 of
tools/make_classes_golden.py.

Asserted, so that tests compare every stored rank and prediction without exception: the top 9 pass-1 logits of each image are
pairwise >= 1e-3 apart, and the top 2 of every stage-2 row are >= 1e-3 apart.  If one fails, change N or the names, not a tolerance.

Output (data only): tests/golden/tiny_vocab.npz.   Usage:  python tools/make_vocab_golden.py [--out tests/golden] [--n 1100]
"""
from __future__ import annotations

import argparse
import dataclasses
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from make_golden import build_reference, install_reference  # noqa: E402
from make_classes_golden import hypotheses, text_rows  # noqa: E402
from camouflaged_vlm_amd import spec, synth  # noqa: E402

N_CLASSES = 1100
K_HYP, K_TOP = 2, 8
N_ROWS = 64                  # text rows kept
GAP = 1e-3


def compose_names(base, n):
    """n distinct names "a b": a = base[i % m], b = base[(a + 1 + i // m) % m] -- a != b and no pair twice while n <= m (m - 1)."""
    m = len(base)
    assert n <= m * (m - 1)
    return [base[i % m] + " " + base[(i % m + 1 + i // m) % m] for i in range(n)]


def main(out_dir, n_cls):
    mm, ml, cm, train_names, test_names = install_reference()
    g = spec.TINY_SAM
    c = dataclasses.replace(spec.TINY_CLIP, n_cls_test=n_cls)
    names = compose_names(list(test_names), n_cls)
    assert len(set(names)) == n_cls
    model, sd, _, eot = build_reference(mm, ml, cm, g, c, train_names, names)
    clipm = model.clip_model
    ids = clipm.tokenized_prompts_test.numpy().astype(np.int32)                    # (N, 77) from the reference's tokenizer
    assert ids.shape == (n_cls, c.context_length) and np.array_equal(ids.argmax(-1), eot)
    width = int(eot.max()) + 1
    assert not ids[:, width:].any()
    table = torch.from_numpy(synth.make_tensor("openai.token_embedding.weight", (49408, c.text_width), "embed", 0))
    emb = table[torch.from_numpy(ids).long()]                                      # (N, 77, W)
    pl = clipm.prompt_learner
    with torch.no_grad():
        pl.token_prefix_test.copy_(emb[:, :1])
        pl.token_suffix_test.copy_(emb[:, 1 + c.n_ctx:])
    bank = torch.from_numpy(synth.make_text_bank(n_cls, c.embed_dim, "test"))
    clipm.test_text_features = bank
    model.test_text_features = bank
    inp, clip_image, clip_mask = synth.make_inputs(g, c, batch=2)
    with np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "tiny_classes.npz")) as z:
        pos = z["pos"]
    with torch.no_grad():
        rows = text_rows(model).numpy().astype(np.float32)
    row_idx = np.sort(np.random.default_rng(7).choice(n_cls, N_ROWS, replace=False)).astype(np.int64)
    outs, top8 = [], []
    for b in range(2):
        print("image %d" % b, flush=True)
        o = hypotheses(model, g, c, *(torch.from_numpy(t[b:b + 1]) for t in (inp, clip_image, clip_mask)), K_HYP)
        p1 = o["pass1_logits"]
        order = np.argsort(-p1, kind="stable")
        top9 = p1[order[:K_TOP + 1]]
        gap1 = float(np.min(top9[:-1] - top9[1:]))
        print("  pass 1: top-9 gap %.3g, classes %s" % (gap1, order[:K_TOP].tolist()))
        assert gap1 >= GAP, gap1
        assert order[:K_HYP].tolist() == o["classes"].tolist()
        for k in range(K_HYP):
            s = np.sort(o["class_logits"][k])[::-1]
            print("  stage 2 of hypothesis %d: top-2 gap %.3g, pred %d" % (k, s[0] - s[1], int(o["pred"][k])))
            assert s[0] - s[1] >= GAP
        outs.append(o)
        top8.append(order[:K_TOP].astype(np.int64))
    st = lambda k: np.stack([o[k] for o in outs])
    path = os.path.join(out_dir, "tiny_vocab.npz")
    np.savez_compressed(
        path, n_cls=np.int64(n_cls), tokens=ids[:, :width], eot=eot.astype(np.int32), row_idx=row_idx, rows=rows[row_idx],
        pass1_logits=st("pass1_logits"), top8=np.stack(top8), classes=st("classes"), low_masks=st("low_masks"), low_edges=st("low_edges"),
        pos=pos, masks_at_pos=np.stack([o["masks"].reshape(K_HYP, -1)[:, pos] for o in outs]).astype(np.float32),
        class_logits=st("class_logits"), pred=st("pred"), hyp0_vs_infer_test=st("hyp0_vs_infer_test"))
    print("%s: %d bytes" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    ap.add_argument("--n", type=int, default=N_CLASSES)
    args = ap.parse_args()
    main(args.out, args.n)
