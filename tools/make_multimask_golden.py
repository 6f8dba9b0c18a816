#!/usr/bin/env python3
"""Golden vectors of the edge decoder's four masks and predicted mask qualities, made by running the REFERENCE's own modules on
CPU (build container only).

The reference's `infer_test` keeps mask 0 (models/sam_maskdecoder_edge.py:347-354, multimask_output=False), but its decoder
computes four masks, the edge map and `iou_pred (P, 4)` for every prompt (models/mmseg/models/sam/mask_decoder_edge.py:163-190)
and hands out masks 1..3 with their qualities under multimask_output=True (:130-135).  Pinned here per image with the steps of
`infer_test` and the decoder's own two calls in place of its `forward`:

    image_encoder(inp, interm=True), get_dense_pe(), no_mask_embed           as infer_test (:334-338)
    maple_alpha_clip_process -> sam_visual_proj | sam_text_proj              the sparse prompt (1, 2, 256) (:341-344)
    mask_decoder.embedding_encoder(features)                                 mask_decoder_edge.py:120
    mask_decoder.predict_masks(...)                                          four masks, edge, iou_pred (1, 4) (:140-190)
    postprocess_masks of the four masks and of the edge map

Mask 0, the edge map and iou_pred[:, 0] are asserted to agree with the reference's own decoder call of `infer_test`
(`mask_decoder(..., multimask_output=False)`) to SLICE0_TOL; the measured difference is stored.  Inputs and weights come from
camouflaged_vlm_amd.synth (the same as tools/make_golden.py, whose reference loader this reuses).  Output (data only):
  tests/golden/tiny_multimask.npz          spec.TINY_SAM / TINY_CLIP, images 0-1, everything low-res in full
  tests/golden/demo_multimask_digest.npz   demo geometry, images 0-1 of synth.make_inputs (digests: sampled logits, iou_pred)
  tests/golden/demo_multimask_bits.npz     the same run: every mask's packed sign bits (eight masks' bits and their sampled
                                           logits together pass the size limit of a committed file, so the bits have a file of their own)

Usage:  python tools/make_multimask_golden.py [--out tests/golden] [--only-tiny | --only-demo]
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

from make_golden import build_reference, install_reference  # noqa: E402
from camouflaged_vlm_amd import spec, synth  # noqa: E402

N_TINY_POS = 8192            # full-resolution positions kept of the tiny masks: tiny_classes.npz's
N_DENSE_DEMO = 16384         # the first N of demo_digest.npz's dense_idx
N_NEAR = 4096                # each mask's own smallest-|logit| positions
SLICE0_TOL = 1e-4            # mask 0 / edge / iou_pred[:, 0] vs the reference's infer_test decoder call


def four_masks(model, g, inp, clip_image, clip_mask):
    """One image (B = 1 tensors) -> dict of the reference's four masks, edge map and predicted qualities."""
    S = g.inp_size
    with torch.no_grad():
        features, interm = model.image_encoder(inp, interm=True)
        image_pe = model.get_dense_pe()
        dense = model.no_mask_embed.weight.reshape(1, -1, 1, 1).expand(1, -1, model.image_embedding_size, model.image_embedding_size)
        img_f, txt_f, _, s1 = model.maple_alpha_clip_process(clip_image, clip_mask)
        sparse = torch.cat((model.sam_visual_proj(img_f), model.sam_text_proj(txt_f)), dim=1)          # (1, 2, 256)
        dec = model.mask_decoder
        low_m, low_e, iou = dec.predict_masks(image_embeddings=features, edge_embeddings=dec.embedding_encoder(features),
                                              image_pe=image_pe, sparse_prompt_embeddings=sparse, dense_prompt_embeddings=dense)
        masks = model.postprocess_masks(low_m, S, S)
        edges = model.postprocess_masks(low_e, S, S)
        ref_m, ref_e, ref_i = dec(image_embeddings=features, interm_embeddings=interm, image_pe=image_pe,
                                  sparse_prompt_embeddings=sparse, dense_prompt_embeddings=dense, multimask_output=False)
    assert low_m.shape[:2] == (1, 4) and low_e.shape[:2] == (1, 1) and iou.shape == (1, 4), (low_m.shape, low_e.shape, iou.shape)
    d = [float((low_m[:, :1] - ref_m).abs().max()), float((low_e - ref_e).abs().max()), float((iou[:, :1] - ref_i).abs().max())]
    print("  mask 0 / edge / iou_pred[:, 0] vs the reference's infer_test decoder call: max |diff| %g / %g / %g" % tuple(d), flush=True)
    assert max(d) <= SLICE0_TOL, d
    return dict(slice0_vs_infer_test=np.asarray(d, dtype=np.float64), pass1_logits=s1[0].numpy().astype(np.float32),
                low_masks=low_m[0].numpy().astype(np.float32), low_edges=low_e[0, 0].numpy().astype(np.float32),
                iou=iou[0].numpy().astype(np.float32), masks=masks[0].numpy(), edges=edges[0, 0].numpy())


def tiny(out_dir, mods):
    mm, ml, cm, train_names, test_names = mods
    g, c = spec.TINY_SAM, spec.TINY_CLIP
    model, sd, eot_train, eot_test = build_reference(mm, ml, cm, g, c, train_names, test_names)
    inp, clip_image, clip_mask = synth.make_inputs(g, c, batch=2)
    pos = np.random.default_rng(11).integers(0, g.inp_size * g.inp_size, size=N_TINY_POS).astype(np.int64)
    outs = []
    for b in range(2):
        print("tiny: image %d" % b, flush=True)
        outs.append(four_masks(model, g, *(torch.from_numpy(t[b:b + 1]) for t in (inp, clip_image, clip_mask))))
    st = lambda k: np.stack([o[k] for o in outs])
    np.savez_compressed(
        os.path.join(out_dir, "tiny_multimask.npz"), low_masks=st("low_masks"), low_edges=st("low_edges"), iou=st("iou"), pos=pos,
        masks_at_pos=np.stack([o["masks"].reshape(4, -1)[:, pos] for o in outs]).astype(np.float32),
        pass1_logits=st("pass1_logits"), slice0_vs_infer_test=st("slice0_vs_infer_test"), eot_test=eot_test,
        bank_test=model.test_text_features.numpy())
    print("tiny: iou_pred %s" % st("iou").tolist())


def demo(out_dir, mods, n_images=2):
    mm, ml, cm, train_names, test_names = mods
    g, c = spec.DEMO_SAM, spec.DEMO_CLIP
    model, sd, eot_train, eot_test = build_reference(mm, ml, cm, g, c, train_names, test_names)
    inp, clip_image, clip_mask = synth.make_inputs(g, c, batch=n_images)
    with np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "demo_digest.npz")) as z:
        sample_idx, dense_idx = z["sample_idx"], z["dense_idx"][:N_DENSE_DEMO]
    keys = ("mask_bits", "mask_samples", "dense_samples", "near_idx", "near_samples", "edge_samples", "iou", "pass1_logits",
            "slice0_vs_infer_test")
    out = {k: [] for k in keys}
    for b in range(n_images):
        t0 = time.time()
        o = four_masks(model, g, *(torch.from_numpy(t[b:b + 1]) for t in (inp, clip_image, clip_mask)))
        m = o["masks"].reshape(4, -1)
        e = o["edges"].reshape(-1)
        near = np.stack([np.sort(np.argpartition(np.abs(m[k]), N_NEAR)[:N_NEAR]) for k in range(4)]).astype(np.int32)
        out["mask_bits"].append(np.stack([np.packbits(m[k] > 0) for k in range(4)]))
        out["mask_samples"].append(m[:, sample_idx]); out["dense_samples"].append(m[:, dense_idx])
        out["near_idx"].append(near); out["near_samples"].append(np.take_along_axis(m, near.astype(np.int64), axis=1))
        out["edge_samples"].append(e[sample_idx])
        for k in ("iou", "pass1_logits", "slice0_vs_infer_test"):
            out[k].append(o[k])
        print("demo: image %d in %.1f s; iou_pred %s" % (b, time.time() - t0, o["iou"].tolist()), flush=True)
    arr = {k: np.stack(v) for k, v in out.items()}
    for k in ("mask_samples", "dense_samples", "near_samples", "edge_samples"):
        arr[k] = arr[k].astype(np.float32)
    bits = arr.pop("mask_bits")
    np.savez_compressed(os.path.join(out_dir, "demo_multimask_digest.npz"), sample_idx=sample_idx, dense_idx=dense_idx,
                        eot_test=eot_test, **arr)
    np.savez_compressed(os.path.join(out_dir, "demo_multimask_bits.npz"), mask_bits=bits)


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
