"""CPU oracle of the edge decoder's multimask output (Cascade.infer_test_multimask), composed from oracle/cvlm_oracle.py's own
functions.

oracle.cvlm_oracle.mask_decoder computes the four masks and iou_pred (1, 4) and keeps slice 0 (its last ten lines); here the same
steps return all of them (models/mmseg/models/sam/mask_decoder_edge.py:163-190), per image as the reference runs them, and
`infer_test_multimask` puts `infer_test`'s steps (models/sam_maskdecoder_edge.py:331-357) around it."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import cvlm_oracle as O


def predict_masks(image_emb, image_pe, sparse, dense, sd, g, prefix: str = "mask_decoder."):
    """-> masks (B, 4, 4h, 4w), edge (B, 1, 4h, 4w), iou_pred (B, 4)."""
    outs = []
    for b in range(image_emb.shape[0]):
        emb, sp, de = image_emb[b:b + 1], sparse[b:b + 1], dense[b:b + 1]
        edge_features = O._upscaler(emb, sd, prefix + "embedding_encoder", final_gelu=False)          # :120
        tokens = torch.cat([sd[prefix + "iou_token.weight"], sd[prefix + "mask_tokens.weight"],
                            sd[prefix + "edge_token.weight"]], dim=0).unsqueeze(0)                     # :150-153
        src = emb + de
        hs, src2 = O.two_way_transformer(src, image_pe, tokens, sp, sd, prefix + "transformer", g.dec_depth, g.dec_heads)
        _, c, h, w = src.shape
        up = O._upscaler(src2.transpose(1, 2).reshape(1, c, h, w), sd, prefix + "output_upscaling", final_gelu=True)   # :168
        mf = prefix + "embedding_maskfeature"
        e = F.conv_transpose2d(up, sd[mf + ".0.weight"], sd[mf + ".0.bias"], stride=1, padding=1)
        e = F.gelu(O.layer_norm_2d(e, sd, mf + ".1"))
        e = F.conv_transpose2d(e, sd[mf + ".3.weight"], sd[mf + ".3.bias"], stride=1, padding=1)
        edge_emb = e + edge_features                                                                   # :170
        mt = hs[:, 1:6, :]                                                                             # :164
        hyper = [O._mlp3(mt[:, i, :], sd, f"{prefix}output_hypernetworks_mlps.{i}") for i in range(4)]
        hyper.append(O._mlp3(mt[:, 4, :], sd, prefix + "edge_mlp"))
        hyper = torch.stack(hyper, dim=1)                                                              # (1, 5, C / 8)
        _, c8, H, W = up.shape
        masks = (hyper[:, :4] @ up.view(1, c8, H * W)).view(1, 4, H, W)                                # :181
        edge = torch.sigmoid((hyper[:, 4:] @ edge_emb.view(1, c8, H * W)).view(1, 1, H, W))            # :182-184
        masks = masks * edge + masks                                                                   # :186
        iou = O._mlp3(hs[:, 0, :], sd, prefix + "iou_prediction_head")                                 # :188
        outs.append((masks, edge, iou))
    return tuple(torch.cat([o[i] for o in outs], dim=0) for i in range(3))


def infer_test_multimask(inp, clip_image, clip_mask, sd, g, c, text_feat, bank):
    """-> dict low_masks (B, 4, 4G, 4G), low_edges (B, 4G, 4G), iou (B, 4), masks (B, 4, S, S), edges (B, S, S), pass1_logits."""
    B, G, S = inp.shape[0], g.grid, g.inp_size
    feats = O.sam_encoder(inp, sd, g)
    pe = O.dense_pe(sd, G).unsqueeze(0)
    img_f, txt_f, _, score = O.clip_forward(clip_image, clip_mask, sd, c, text_feat, bank)
    v = O.layer_norm(img_f, sd, "sam_visual_proj.0", 1e-5)
    v = O.layer_norm(O.linear(v, sd, "sam_visual_proj.1"), sd, "sam_visual_proj.2", 1e-5)
    t = O.linear(O.layer_norm(txt_f, sd, "sam_text_proj.0", 1e-5), sd, "sam_text_proj.1")
    sparse = torch.cat((v, t), dim=1)                                                                  # (B, 2, 256)
    dense = sd["no_mask_embed.weight"].reshape(1, -1, 1, 1).expand(B, -1, G, G)
    low_m, low_e, iou = predict_masks(feats, pe, sparse, dense, sd, g)
    return dict(low_masks=low_m, low_edges=low_e[:, 0], iou=iou, masks=O.postprocess_masks(low_m, S),
                edges=O.postprocess_masks(low_e, S)[:, 0], pass1_logits=score)
