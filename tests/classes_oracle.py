"""CPU oracle of K class hypotheses per image (Cascade.infer_classes), composed from oracle/cvlm_oracle.py's own functions.

Per image, K sparse prompts (K, 2, 256) -- the image feature's sam_visual_proj row with the sam_text_proj rows of the K chosen
text rows -- go through the edge mask decoder together with K copies of the image's features, in the prompt order p = b * K + k
of the reference's repeat_interleave (models/mmseg/models/sam/mask_decoder_edge.py:150-158); masks and edges are upsampled by
postprocess_masks, and stage 2 (demo.py:117-122) runs on each hypothesis's mask."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import cvlm_oracle as O


def text_rows(text_feat, bank):
    """cocotrainers/mapleAlphaCLIP.py:289-291: the rows pass 1 indexes with its argmax."""
    return text_feat / text_feat.norm(dim=-1, keepdim=True) + bank


def infer_classes(inp, clip_image, clip_mask, sd, g, c, text_feat, bank, classes=None, topk=None):
    """-> dict classes (B, K), pass1_logits (B, n), low_masks / low_edges (B, K, 4G, 4G), masks / edges (B, K, S, S),
    logits (B, K, n), pred (B, K)."""
    B, G, S, R = inp.shape[0], g.grid, g.inp_size, c.image_resolution
    feats = O.sam_encoder(inp, sd, g)
    pe = O.dense_pe(sd, G).unsqueeze(0)
    img_f, _, _, score = O.clip_forward(clip_image, clip_mask, sd, c, text_feat, bank)
    if classes is None:
        classes = torch.topk(score, topk, dim=1).indices
    classes = torch.as_tensor(classes, dtype=torch.int64)
    K = classes.shape[1]
    P = B * K
    sel = text_rows(text_feat, bank)[classes.reshape(-1)].unsqueeze(1)                  # (P, 1, D)
    v = O.layer_norm(img_f, sd, "sam_visual_proj.0", 1e-5)
    v = O.layer_norm(O.linear(v, sd, "sam_visual_proj.1"), sd, "sam_visual_proj.2", 1e-5)
    t = O.linear(O.layer_norm(sel, sd, "sam_text_proj.0", 1e-5), sd, "sam_text_proj.1")
    sparse = torch.cat((v.repeat_interleave(K, 0), t), dim=1)                           # (P, 2, 256)
    dense = sd["no_mask_embed.weight"].reshape(1, -1, 1, 1).expand(P, -1, G, G)
    low_m, low_e, _ = O.mask_decoder(feats.repeat_interleave(K, 0), pe, sparse, dense, sd, g)
    masks, edges = O.postprocess_masks(low_m, S), O.postprocess_masks(low_e, S)
    alpha = F.interpolate(torch.sigmoid(masks), (R, R), mode="bilinear", align_corners=False)
    _, _, pred, logits = O.clip_forward(clip_image.repeat_interleave(K, 0), alpha, sd, c, text_feat, bank)
    n = logits.shape[-1]
    return dict(classes=classes, pass1_logits=score, low_masks=low_m.reshape(B, K, 4 * G, 4 * G),
                low_edges=low_e.reshape(B, K, 4 * G, 4 * G), masks=masks.reshape(B, K, S, S), edges=edges.reshape(B, K, S, S),
                logits=logits.reshape(B, K, n), pred=pred.reshape(B, K))
