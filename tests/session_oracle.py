"""CPU oracle of Cascade.decode(text=): the K-prompt oracle of tests/classes_oracle.py with the text rows passed in.

Per image, K sparse prompts -- the image feature's sam_visual_proj row with the sam_text_proj rows of K caller-supplied text rows
(models/sam_maskdecoder_edge.py:342-344 takes any row of the bank's width) -- go through the edge mask decoder together with K
copies of the image's features, in the prompt order p = i * K + k (models/mmseg/models/sam/mask_decoder_edge.py:150-158); masks
and edges are upsampled by postprocess_masks, and stage 2 (demo.py:117-122) runs on each hypothesis's mask.  Given the bank rows
`classes_oracle.text_rows(text_feat, bank)[classes]` it returns exactly what `classes_oracle.infer_classes(classes=)` returns."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import cvlm_oracle as O


def decode_text(inp, clip_image, clip_mask, sd, g, c, text_feat, bank, text, images=None):
    """text f32 (n, K, D); images: indices into the batch (default all, n = B) -> dict pass1_logits (n, n_cls), low_masks /
    low_edges (n, K, 4G, 4G), masks / edges (n, K, S, S), logits (n, K, n_cls), pred (n, K)."""
    G, S, R = g.grid, g.inp_size, c.image_resolution
    feats = O.sam_encoder(inp, sd, g)
    pe = O.dense_pe(sd, G).unsqueeze(0)
    img_f, _, _, score = O.clip_forward(clip_image, clip_mask, sd, c, text_feat, bank)
    if images is not None:
        sel_i = torch.as_tensor(list(images), dtype=torch.int64)
        feats, img_f, score, clip_image = feats[sel_i], img_f[sel_i], score[sel_i], clip_image[sel_i]
    text = torch.as_tensor(text, dtype=torch.float32)
    n, K, D = text.shape
    assert n == feats.shape[0]
    P = n * K
    sel = text.reshape(P, D).unsqueeze(1)                                                # (P, 1, D)
    v = O.layer_norm(img_f, sd, "sam_visual_proj.0", 1e-5)
    v = O.layer_norm(O.linear(v, sd, "sam_visual_proj.1"), sd, "sam_visual_proj.2", 1e-5)
    t = O.linear(O.layer_norm(sel, sd, "sam_text_proj.0", 1e-5), sd, "sam_text_proj.1")
    sparse = torch.cat((v.repeat_interleave(K, 0), t), dim=1)                           # (P, 2, 256)
    dense = sd["no_mask_embed.weight"].reshape(1, -1, 1, 1).expand(P, -1, G, G)
    low_m, low_e, _ = O.mask_decoder(feats.repeat_interleave(K, 0), pe, sparse, dense, sd, g)
    masks, edges = O.postprocess_masks(low_m, S), O.postprocess_masks(low_e, S)
    alpha = F.interpolate(torch.sigmoid(masks), (R, R), mode="bilinear", align_corners=False)
    _, _, pred, logits = O.clip_forward(clip_image.repeat_interleave(K, 0), alpha, sd, c, text_feat, bank)
    n_cls = logits.shape[-1]
    return dict(pass1_logits=score, low_masks=low_m.reshape(n, K, 4 * G, 4 * G), low_edges=low_e.reshape(n, K, 4 * G, 4 * G),
                masks=masks.reshape(n, K, S, S), edges=edges.reshape(n, K, S, S), logits=logits.reshape(n, K, n_cls),
                pred=pred.reshape(n, K))
