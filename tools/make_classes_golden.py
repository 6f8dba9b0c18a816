#!/usr/bin/env python3
"""Golden vectors of K class hypotheses per image, made by running the REFERENCE's own modules on CPU (build container only).

The reference segments for ONE class per image: CLIP pass 1's argmax picks the text row that conditions the mask decoder
(models/sam_maskdecoder_edge.py:341-344, cocotrainers/mapleAlphaCLIP.py:285-294).  Its decoder already serves several prompts
per image -- `predict_masks` expands the output tokens to sparse_prompt_embeddings.size(0) and repeat_interleaves the image
embedding (models/mmseg/models/sam/mask_decoder_edge.py:150-158,170) -- so "one image, K class prompts -> K masks" is pinned
here with ONE `mask_decoder(...)` call per image on sparse prompts (K, 2, 256):

    image_encoder(inp, interm=True)                              features of the image
    clip_model(clip_image, clip_mask, False)                     pass 1 (logits, image feature)
    prompt_learner.forward_test -> text_encoder -> normalise + bank      the test-branch text rows of every class (:285-291)
    torch.topk(pass-1 logits, K)                                 the hypotheses
    sam_visual_proj(image feature), sam_text_proj(text rows)     sparse prompts (K, 2, 256)
    mask_decoder(...) once; postprocess_masks of masks AND edges
    stage 2 per hypothesis: clip_model(clip_image, resize(sigmoid(mask_k)), False)      (demo.py:116-122)

Hypothesis 0 is asserted to reproduce the reference's own `infer_test` for that image to HYP0_TOL (measured and stored: the CPU
reference's K-prompt call and its one-prompt call differ by ~1e-5, the blocking of its GEMMs).  Inputs and weights come from
camouflaged_vlm_amd.synth (the same as tools/make_golden.py, whose reference loader this reuses).  Output (data only):
  tests/golden/tiny_classes.npz          spec.TINY_SAM / TINY_CLIP, images 0-1, K = n_cls = 5
  tests/golden/demo_classes_digest.npz   demo geometry, images 0-1 of synth.make_inputs, K = 3 (digests)

Usage:  python tools/make_classes_golden.py [--out tests/golden] [--only-tiny | --only-demo]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from make_golden import build_reference, install_reference  # noqa: E402
from camouflaged_vlm_amd import spec, synth  # noqa: E402

N_TINY_POS = 8192            # full-resolution positions kept of the tiny masks / edges
N_DENSE_DEMO = 16384         # the first N of demo_digest.npz's dense_idx
N_NEAR = 4096                # each hypothesis's own smallest-|logit| positions
HYP0_TOL = 1e-4              # hypothesis 0 vs the reference's infer_test (the same image, one decoder prompt)


def text_rows(model):
    """The test-branch text rows of every class: mapleAlphaCLIP.py:285-291 (what pass 1 indexes with its argmax)."""
    cm = model.clip_model
    prompts, _, deep_text, _ = cm.prompt_learner.forward_test()
    tf = cm.text_encoder(prompts, cm.tokenized_prompts_test, deep_text)
    tf = tf / tf.norm(dim=-1, keepdim=True)
    return tf + cm.test_text_features


def hypotheses(model, g, c, inp, clip_image, clip_mask, K):
    """One image (B = 1 tensors) -> dict of the K hypotheses' reference outputs."""
    S, R = g.inp_size, c.image_resolution
    with torch.no_grad():
        features, interm = model.image_encoder(inp, interm=True)
        image_pe = model.get_dense_pe()
        dense = model.no_mask_embed.weight.reshape(1, -1, 1, 1).expand(1, -1, model.image_embedding_size, model.image_embedding_size)
        img_f, txt_f, pred1, s1 = model.clip_model(clip_image, clip_mask, False)
        txt = text_rows(model)
        top = torch.topk(s1[0], K)
        classes = top.indices
        assert int(classes[0]) == int(pred1[0]), (classes, pred1)
        sel = txt[classes].unsqueeze(1)                                    # (K, 1, D)
        assert torch.equal(sel[0], txt_f[0]), "text row of hypothesis 0 != pass 1's text_features[pred_label_id]"
        vis = model.sam_visual_proj(img_f)                                 # (1, 1, 256)
        sparse = torch.cat((vis.expand(K, -1, -1), model.sam_text_proj(sel)), dim=1)      # (K, 2, 256)
        low_m, low_e, _ = model.mask_decoder(image_embeddings=features, interm_embeddings=interm, image_pe=image_pe,
                                             sparse_prompt_embeddings=sparse, dense_prompt_embeddings=dense,
                                             multimask_output=False)
        masks = model.postprocess_masks(low_m, S, S)
        edges = model.postprocess_masks(low_e, S, S)
        logits, preds = [], []
        for k in range(K):
            alpha = F.interpolate(torch.sigmoid(masks[k:k + 1]), (R, R), mode="bilinear", align_corners=False)
            _, _, p, s = model.clip_model(clip_image, alpha, False)
            logits.append(s[0]); preds.append(p[0])
        ref = model.infer_test(inp, clip_image, clip_mask)
    d = float((masks[:1] - ref).abs().max())
    print("  hypothesis 0 vs the reference's infer_test: max |diff| %g (%s)" % (d, "IDENTICAL" if torch.equal(masks[:1], ref) else "DIFFERENT"),
          flush=True)
    # the CPU reference's own K-prompt decoder call is not bit-identical to its one-prompt call (its GEMMs block the rows of a
    # K-image batch differently: ~1e-5 here): the assertion holds hypothesis 0 to the rounding of that arithmetic
    assert d <= HYP0_TOL, d
    return dict(hyp0_vs_infer_test=np.float64(d), classes=classes.numpy().astype(np.int64), pass1_logits=s1[0].numpy().astype(np.float32),
                low_masks=low_m[:, 0].numpy().astype(np.float32), low_edges=low_e[:, 0].numpy().astype(np.float32),
                masks=masks[:, 0].numpy(), edges=edges[:, 0].numpy(), class_logits=torch.stack(logits).numpy().astype(np.float32),
                pred=torch.stack(preds).numpy().astype(np.int64))


def tiny(out_dir, mods):
    mm, ml, cm, train_names, test_names = mods
    g, c = spec.TINY_SAM, spec.TINY_CLIP
    model, sd, eot_train, eot_test = build_reference(mm, ml, cm, g, c, train_names, test_names)
    K = c.n_cls_test
    inp, clip_image, clip_mask = synth.make_inputs(g, c, batch=2)
    pos = np.random.default_rng(11).integers(0, g.inp_size * g.inp_size, size=N_TINY_POS).astype(np.int64)
    outs = []
    for b in range(2):
        print("tiny: image %d" % b, flush=True)
        outs.append(hypotheses(model, g, c, *(torch.from_numpy(t[b:b + 1]) for t in (inp, clip_image, clip_mask)), K))
    st = lambda k: np.stack([o[k] for o in outs])
    np.savez_compressed(
        os.path.join(out_dir, "tiny_classes.npz"), classes=st("classes"), pass1_logits=st("pass1_logits"),
        low_masks=st("low_masks"), low_edges=st("low_edges"), pos=pos,
        masks_at_pos=np.stack([o["masks"].reshape(K, -1)[:, pos] for o in outs]).astype(np.float32),
        class_logits=st("class_logits"), pred=st("pred"), hyp0_vs_infer_test=st("hyp0_vs_infer_test"), eot_test=eot_test,
        bank_test=model.test_text_features.numpy())
    print("tiny: classes %s | stage-2 pred %s" % (st("classes").tolist(), st("pred").tolist()))


def demo(out_dir, mods, n_images=2, K=3):
    mm, ml, cm, train_names, test_names = mods
    g, c = spec.DEMO_SAM, spec.DEMO_CLIP
    model, sd, eot_train, eot_test = build_reference(mm, ml, cm, g, c, train_names, test_names)
    inp, clip_image, clip_mask = synth.make_inputs(g, c, batch=n_images)
    with np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "demo_digest.npz")) as z:
        sample_idx, dense_idx = z["sample_idx"], z["dense_idx"][:N_DENSE_DEMO]
    keys = ("mask_bits", "mask_samples", "dense_samples", "near_idx", "near_samples", "edge_samples", "class_logits", "pred",
            "pass1_logits", "classes", "hyp0_vs_infer_test")
    out = {k: [] for k in keys}
    for b in range(n_images):
        t0 = time.time()
        o = hypotheses(model, g, c, *(torch.from_numpy(t[b:b + 1]) for t in (inp, clip_image, clip_mask)), K)
        m = o["masks"].reshape(K, -1)
        e = o["edges"].reshape(K, -1)
        near = np.stack([np.sort(np.argpartition(np.abs(m[k]), N_NEAR)[:N_NEAR]) for k in range(K)]).astype(np.int32)
        out["mask_bits"].append(np.stack([np.packbits(m[k] > 0) for k in range(K)]))
        out["mask_samples"].append(m[:, sample_idx]); out["dense_samples"].append(m[:, dense_idx])
        out["near_idx"].append(near); out["near_samples"].append(np.take_along_axis(m, near.astype(np.int64), axis=1))
        out["edge_samples"].append(e[:, sample_idx])
        for k in ("class_logits", "pred", "pass1_logits", "classes", "hyp0_vs_infer_test"):
            out[k].append(o[k])
        print("demo: image %d in %.1f s; classes %s; stage-2 pred %s" % (b, time.time() - t0, o["classes"].tolist(), o["pred"].tolist()),
              flush=True)
    arr = {k: np.stack(v) for k, v in out.items()}
    for k in ("mask_samples", "dense_samples", "near_samples", "edge_samples"):
        arr[k] = arr[k].astype(np.float32)
    np.savez_compressed(os.path.join(out_dir, "demo_classes_digest.npz"), sample_idx=sample_idx, dense_idx=dense_idx,
                        eot_test=eot_test, **arr)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    ap.add_argument("--only-tiny", action="store_true")
    ap.add_argument("--only-demo", action="store_true")
    ap.add_argument("--threads", type=int, default=0)
    args = ap.parse_args()
    if args.threads:
        torch.set_num_threads(args.threads)
    mods = install_reference()
    if not args.only_demo:
        tiny(args.out, mods)
    if not args.only_tiny:
        demo(args.out, mods)
