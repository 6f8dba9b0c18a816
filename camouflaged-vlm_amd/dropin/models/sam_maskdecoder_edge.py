"""Drop-in mirror of the reference wrapper ``models/sam_maskdecoder_edge.py`` (class ``SAM``,
registry name ``sam_maskdecoder_edge``): same constructor arguments, same state_dict keys, same
inference methods (``load_mapleAlphaCLIP``, ``infer_test``, ``infer``, ``postprocess_masks``,
``get_dense_pe``) and the ``clip_model`` attribute -- every operator runs on the MI355X HIP path
(camouflaged_vlm_amd.engine); there is no PyTorch compute fallback.

Differences that are deliberate and documented:
  * batched inputs are supported and are defined as B independent B=1 forwards (the reference's
    decoder only works for B=1, mask_decoder_edge.py:156-158);
  * the image-independent MaPLe text encoder is evaluated once per weight load, not per call;
  * training methods (forward/backward_G/optimize_parameters) are out of scope and raise;
  * ``infer_classes`` is an extension (K class hypotheses per image), not a method of the reference.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from camouflaged_vlm_amd import hip, host, spec
from camouflaged_vlm_amd.engine import Cascade, Precision

from .models import register


@register('sam_maskdecoder_edge')
class SAM(nn.Module):
    def __init__(self, inp_size=None, encoder_mode=None, loss=None, *, seed: int = 0):
        super().__init__()
        self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.geometry = spec.SamGeometry.from_encoder_mode(inp_size, encoder_mode)
        self.embed_dim = encoder_mode['embed_dim']
        self.prompt_embed_dim = encoder_mode['prompt_embed_dim']
        self.inp_size = inp_size
        self.image_embedding_size = inp_size // encoder_mode['patch_size']
        self.loss_mode = loss
        host.populate(self, spec.sam_entries(self.geometry), seed=seed)
        self.image_encoder.img_size = inp_size
        # models/sam_maskdecoder_edge.py:177-182 (relative to CWD; packaged copy as fallback)
        self.train_text_features = host.load_text_bank("train").to(self.device)
        self.test_text_features = host.load_text_bank("test").to(self.device)
        self.precision: Optional[Precision] = None
        self._cascade: Optional[Cascade] = None

    # ---- reference call surface ------------------------------------------------------------------
    def load_mapleAlphaCLIP(self, maple_clip_model, MaPLeAlphaCLIP_checkpoint=None):
        """models/sam_maskdecoder_edge.py:184-201."""
        self.clip_model = maple_clip_model.float()
        for _, p in self.clip_model.named_parameters():
            p.requires_grad = False
        self.clip_model.to(self.device)
        self.clip_model.load_text_features(self.train_text_features, self.test_text_features)
        if MaPLeAlphaCLIP_checkpoint is not None:
            state_dict = dict(host.load_checkpoint_state_dict(MaPLeAlphaCLIP_checkpoint))   # Dassl: {"state_dict": ...}
            for k in ("prompt_learner.token_prefix", "prompt_learner.token_suffix"):
                state_dict.pop(k, None)                     # fixed token vectors are ignored (:196-199)
            self.clip_model.load_state_dict(state_dict, strict=False)
        self._cascade = None

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self._cascade = None
        if hasattr(self, "clip_model"):                      # the recursion bypasses the child's override
            self.clip_model._engine = None
            self.clip_model._engine_text_dirty = True
        return r

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._cascade = None
        try:
            self.device = self.no_mask_embed.weight.device
            self.train_text_features = self.train_text_features.to(self.device)
            self.test_text_features = self.test_text_features.to(self.device)
            if hasattr(self, "clip_model"):
                self.clip_model.load_text_features(self.train_text_features, self.test_text_features)
        except AttributeError:
            pass
        return r

    def cascade(self) -> Cascade:
        if not hasattr(self, "clip_model"):
            raise RuntimeError("call load_mapleAlphaCLIP(...) first (demo.py:87)")
        dev = self.no_mask_embed.weight.device
        if dev.type != "cuda":
            raise RuntimeError("camouflaged_vlm_amd runs on MI355X only: call .cuda() first; there is no CPU fallback")
        clip_engine = self.clip_model.engine()
        if self._cascade is None or self._cascade.clip is not clip_engine:
            prec = self.precision or host.precision_from_env()
            sd = {k: v for k, v in self.state_dict().items() if not k.startswith("clip_model.")}
            self._cascade = Cascade(sd, self.geometry, self.clip_model.geometry, dev, prec, clip=clip_engine)
        return self._cascade

    def get_dense_pe(self) -> torch.Tensor:
        """:210-219 -> (1, C, h, w)."""
        G, C = self.image_embedding_size, self.prompt_embed_dim
        out = torch.empty(G * G, C, device=self.no_mask_embed.weight.device)
        hip.dense_pe(self.pe_layer.positional_encoding_gaussian_matrix, G, C, out)
        return out.reshape(G, G, C).permute(2, 0, 1).unsqueeze(0)

    def maple_alpha_clip_process(self, image, alpha):
        """:268-270 (``self.training`` lands in ``label``: always the test branch, Appendix B.2)."""
        return self.clip_model(image, alpha, self.training)

    # ---- class vocabularies at run time (EXTENSION; INTEGRATION.md, "Vocabularies at run time") ------------------------------------
    def make_vocabulary(self, **kw):
        """EXTENSION, not a reference method: a class vocabulary from token ids (`tokens=`, against `table=` or the CLIP module's
        kept token-embedding table) or embedded prompts (`embeddings=`, `eot=`), with its `bank=` and a `name=`.  -> engine.Vocabulary
        for `vocab=` of the inference methods and `use_vocabulary`; valid until the engines are rebuilt (load_state_dict, .cuda())."""
        if not hasattr(self, "clip_model"):
            raise RuntimeError("call load_mapleAlphaCLIP(...) first (demo.py:87)")
        return self.clip_model.make_vocabulary(**kw)

    def use_vocabulary(self, vocab) -> None:
        """EXTENSION: make `vocab` the default of every inference method (None: the constructor's classes again)."""
        self._vocab(vocab)
        self.cascade().use_vocabulary(vocab)

    def _vocab(self, vocab):
        if vocab is not None:
            if not hasattr(self, "clip_model"):
                raise RuntimeError("call load_mapleAlphaCLIP(...) first (demo.py:87)")
            self.clip_model.check_vocabulary(vocab)
        return vocab

    def infer_test(self, input, clip_image, clip_zero_mask, vocab=None):
        """:331-357 -> (B,1,inp_size,inp_size) fp32 mask logits."""
        H, W = input.shape[-2:]
        assert H == self.inp_size and W == self.inp_size, \
            f"Input image size ({H}*{W}) doesn't match model ({self.inp_size}*{self.inp_size})."
        return self.cascade().infer_test(input.float().contiguous(), clip_image.float().contiguous(),
                                         clip_zero_mask.float().contiguous(), vocab=self._vocab(vocab))

    def infer_classes(self, input, clip_image, clip_zero_mask, classes=None, topk=None, quality=False, vocab=None, masks="logits",
                      overlaps=False, components=None, min_area=0, connectivity=8, holes=None, fill_holes=0, band=None,
                      edge_threshold=None, rle=None, sizes=None, sized_level=128, ground_truth=None, label_maps=False, label_weights=None,
                      overlap_threshold=0.8):
        """EXTENSION, not a reference method: K class hypotheses per image from one encoder pass -- for each, the mask logits,
        the edge map and stage 2 that `infer_test` + demo.py:116-122 give had CLIP pass 1 predicted that class (the reference's
        decoder runs K prompts per image in one call, mask_decoder_edge.py:150-158).  Exactly one of `topk` (the K largest
        pass-1 logits) and `classes` (int64 (B, K)).  masks="bits" / "both" and overlaps=True: packed binary masks, areas, boxes
        and pairwise intersections, components= / min_area= / connectivity=: the connected regions of each packed mask, holes= /
        fill_holes=: its holes and the mask with its pinholes closed, band=: its edge band (:441-445 at radius 2), edge_threshold=:
        the edge head's map (:298-302) above that threshold as bits, counted on the band it is trained against (:441-447), rle="mask" /
        "kept" / "filled": those planes as COCO run-length counts (`rle`, engine.MaskRle), as engine.Cascade.infer_classes documents
        them; sizes= / sized_level=: the masks at each image's own (h, w) -- what test_ovcos_maskdecoder_edge.py:116-130 resizes to -- as
        bits of the uint8 mask >= sized_level (`sized`, engine.SizedMasks), rle="sized": those as COCO RLE with each image's own "size";
        ground_truth=(gt, gt_image): the sized planes' intersections with the annotations of their image (`gt_overlaps`,
        engine.SizedOverlaps, whose `iou()` is the COCO IoU); label_maps=True / label_weights= / overlap_threshold=: one hypothesis per
        pixel at each image's own size (`label_maps`, engine.LabelMaps).
        -> engine.ClassHypotheses ("K class hypotheses per image")."""
        H, W = input.shape[-2:]
        assert H == self.inp_size and W == self.inp_size, \
            f"Input image size ({H}*{W}) doesn't match model ({self.inp_size}*{self.inp_size})."
        return self.cascade().infer_classes(input.float().contiguous(), clip_image.float().contiguous(),
                                            clip_zero_mask.float().contiguous(), classes=classes, topk=topk, quality=quality,
                                            vocab=self._vocab(vocab), masks=masks, overlaps=overlaps, components=components,
                                            min_area=min_area, connectivity=connectivity, holes=holes, fill_holes=fill_holes, band=band,
                                            edge_threshold=edge_threshold, rle=rle, sizes=sizes, sized_level=sized_level,
                                            ground_truth=ground_truth, label_maps=label_maps, label_weights=label_weights,
                                            overlap_threshold=overlap_threshold)

    def pack_masks(self, logits):
        """EXTENSION, not a reference method: (bits, area, box) of (N, S, S) or (N, 1, S, S) f32 mask logits, e.g. `infer_test`'s:
        logits > 0 packed in numpy.packbits' order, the set pixels counted and boxed (engine.Cascade.pack_masks)."""
        return self.cascade().pack_masks(logits)

    def mask_components(self, bits, H, W, components=1, min_area=0, connectivity=8):
        """EXTENSION, not a reference method: the connected regions of (N, H * W / 8) uint8 packed masks, e.g. `pack_masks`' bits -- what
        the reference's visualizer computes on the host with cv2.connectedComponentsWithStats (models/utils/visualizer.py:1254)
        -> engine.MaskComponents (engine.Cascade.mask_components)."""
        return self.cascade().mask_components(bits, H, W, components=components, min_area=min_area, connectivity=connectivity)

    def mask_holes(self, bits, H, W, holes=1, fill_holes=0, connectivity=8):
        """EXTENSION, not a reference method: the holes of (N, H * W / 8) uint8 packed masks, e.g. `pack_masks`' bits -- what the
        reference's GenericMask.has_holes asks cv2.findContours(..., RETR_CCOMP) on the host (models/utils/visualizer.py:110-136) and
        what SAM's remove_small_regions(mask, t, "holes") fills -> engine.MaskHoles (engine.Cascade.mask_holes)."""
        return self.cascade().mask_holes(bits, H, W, holes=holes, fill_holes=fill_holes, connectivity=connectivity)

    def mask_morph(self, bits, H, W, radius=2, dilate=False, erode=False, band=True):
        """EXTENSION, not a reference method: dilation, erosion and edge band of (N, H * W / 8) uint8 packed masks, e.g. `pack_masks`'
        bits, by the (2 radius + 1)^2 square -- radius=2 is the band this model's edge target is (:441-445), and what cv2.dilate /
        cv2.erode do on the host (datasets/de_transform.py:20-30) -> engine.MaskMorph (engine.Cascade.mask_morph)."""
        return self.cascade().mask_morph(bits, H, W, radius=radius, dilate=dilate, erode=erode, band=band)

    def pack_edges(self, prob, size=None, *, threshold, with_bits=None):
        """EXTENSION, not a reference method: (N, h, w) or (N, 1, h, w) f32 edge probabilities, e.g. `infer_test_multimask(...).edges`
        -- the map :298-302 return -- resized to `size` (None: as they are), compared `> threshold` and packed in numpy.packbits'
        order, with their areas and their intersections with `with_bits` -> engine.EdgeBits (engine.Cascade.pack_edges)."""
        return self.cascade().pack_edges(prob, size, threshold=threshold, with_bits=with_bits)

    def pack_masks_sized(self, logits, sizes, *, level=128):
        """EXTENSION, not a reference method: (N, S, S) or (N, 1, S, S) f32 mask logits, e.g. `infer_test`'s, as packed masks at each
        image's own size sizes[i] = (h, w): the bits of sigmoid -> cv2.resize -> * 255 (test_ovcos_maskdecoder_edge.py:103,116-130) >=
        level -> engine.SizedMasks (engine.Cascade.pack_masks_sized)."""
        return self.cascade().pack_masks_sized(logits, sizes, level=level)

    def label_maps(self, logits, sizes, *, K, weights=None, level=128, overlap_threshold=0.8):
        """EXTENSION, not a reference method: (B * K, S, S) or (B * K, 1, S, S) f32 mask logits of K hypotheses per image as one label
        map per image at its own size sizes[b] = (h, w) -- per pixel the hypothesis with the largest weight * resized sigmoid mask, per
        hypothesis the areas and the overlap test of Mask2Former's panoptic_inference -> engine.LabelMaps (engine.Cascade.label_maps)."""
        return self.cascade().label_maps(logits, sizes, K=K, weights=weights, level=level, overlap_threshold=overlap_threshold)

    def label_iou(self, pred, gt, *, num_classes, ignore_index=255, reduce_zero_label=False, totals=None):
        """EXTENSION, not a reference method: the vendored mmseg's intersect_and_union (models/mmseg/core/evaluation/metrics.py:5-59) of a
        label map against ground truth, summed on the device -> int64 (3, num_classes) totals for segeval.eval_metrics
        (engine.Cascade.label_iou)."""
        return self.cascade().label_iou(pred, gt, num_classes=num_classes, ignore_index=ignore_index, reduce_zero_label=reduce_zero_label,
                                        totals=totals)

    def panoptic_remap(self, raw, sizes, segments, *, rgb=False):
        """EXTENSION, not a reference method: a panoptic ground truth -- id maps, or the RGB pixels the reference's visualizer reads through
        panopticapi's rgb2id (models/utils/visualizer.py:606-611) -- as dense slot indices with its slot tables ->
        engine.PanopticGroundTruth (engine.Cascade.panoptic_remap)."""
        return self.cascade().panoptic_remap(raw, sizes, segments, rgb=rgb)

    def panoptic_quality(self, pred, pred_cat, gt, gt_cat, gt_crowd, sizes, *, num_classes, totals=None):
        """EXTENSION, not a reference method: panopticapi's pq_compute of a predicted panoptic map against ground truth, summed on the
        device -> engine.PanopticTotals for segeval.pq_average (engine.Cascade.panoptic_quality)."""
        return self.cascade().panoptic_quality(pred, pred_cat, gt, gt_cat, gt_crowd, sizes, num_classes=num_classes, totals=totals)

    def mask_rle_sized(self, sized):
        """EXTENSION, not a reference method: COCO run-length encoding of an engine.SizedMasks, "size": [h, w] of each image
        -> engine.MaskRle (engine.Cascade.mask_rle_sized)."""
        return self.cascade().mask_rle_sized(sized)

    def rle_decode(self, rles, *, stats=True):
        """EXTENSION, not a reference method: COCO run-length annotations -- a list of {"size": [h, w], "counts": ...} dicts, or an
        engine.MaskRle on the device -- as packed masks at each annotation's own size -> engine.SizedMasks (engine.Cascade.rle_decode)."""
        return self.cascade().rle_decode(rles, stats=stats)

    def polygons_decode(self, anns, *, stats=True):
        """EXTENSION, not a reference method: COCO polygon annotations -- a list of {"size": [h, w], "polygons": [[x0, y0, ...], ...]},
        the list of polygons the reference's GenericMask takes (models/utils/visualizer.py:72-101) -- rasterised as pycocotools'
        frPyObjects + merge + decode do, as packed masks at each annotation's own size -> engine.SizedMasks
        (engine.Cascade.polygons_decode)."""
        return self.cascade().polygons_decode(anns, stats=stats)

    def mask_inter_sized(self, a, b, *, pairs=None, a_image=None, b_image=None):
        """EXTENSION, not a reference method: intersections of pairs of planes of two engine.SizedMasks, detections against annotations
        -> engine.SizedOverlaps, whose `iou(iscrowd)` is pycocotools' rleIou (engine.Cascade.mask_inter_sized)."""
        return self.cascade().mask_inter_sized(a, b, pairs=pairs, a_image=a_image, b_image=b_image)

    def coco_match(self, dets, gts, *, scores, det_image, gt_image, det_category=None, gt_category=None, iscrowd=None, gt_area=None,
                   iou_thrs=None, area_rngs=None, max_det=100, boundary=None):
        """EXTENSION, not a reference method: detections against annotations as pycocotools' COCOeval.evaluateImg matches them, for
        every (image, category) group, area range and IoU threshold -> engine.CocoMatches, from which cocoeval.accumulate / summarize
        give AP and AR (engine.Cascade.coco_match); boundary=0.02 matches on min(mask IoU, boundary IoU): Boundary AP and AR."""
        return self.cascade().coco_match(dets, gts, scores=scores, det_image=det_image, gt_image=gt_image, det_category=det_category,
                                         gt_category=gt_category, iscrowd=iscrowd, gt_area=gt_area, iou_thrs=iou_thrs, area_rngs=area_rngs,
                                         max_det=max_det, boundary=boundary)

    def mask_boundary_sized(self, sized, *, dilation_ratio=0.02, radius=None):
        """EXTENSION, not a reference method: the boundary of each plane of an engine.SizedMasks as boundary_iou_api's mask_to_boundary
        forms it -> engine.SizedMasks (engine.Cascade.mask_boundary_sized)."""
        return self.cascade().mask_boundary_sized(sized, dilation_ratio=dilation_ratio, radius=radius)

    def mask_contours_sized(self, sized, *, connectivity=8):
        """EXTENSION, not a reference method: the outline of each plane of an engine.SizedMasks as closed polygons along the pixel
        edges -- what the reference's GenericMask.mask_to_polygons (models/utils/visualizer.py:125) gets from cv2.findContours on the
        host -> engine.MaskContours, whose `to_coco()` gives the polygon lists (engine.Cascade.mask_contours_sized)."""
        return self.cascade().mask_contours_sized(sized, connectivity=connectivity)

    def simplify_contours(self, contours, *, tolerance=1.0):
        """EXTENSION, not a reference method: the rings of an engine.MaskContours simplified on the device by Ramer-Douglas-Peucker at
        `tolerance` pixels -- what a consumer of the reference's GenericMask.polygons does ring by ring on the host -> engine.MaskPolygons,
        whose `to_coco()` gives the short polygon lists (engine.Cascade.simplify_contours)."""
        return self.cascade().simplify_contours(contours, tolerance=tolerance)

    def mask_distance_sized(self, sized, *, reach=None):
        """EXTENSION, not a reference method: the exact squared Euclidean distance map of each plane of an engine.SizedMasks
        -> engine.MaskDistances (engine.Cascade.mask_distance_sized)."""
        return self.cascade().mask_distance_sized(sized, reach=reach)

    def mask_surface_distances(self, a, b, *, pairs=None, tolerance=0.008, surface="boundary", reach=None):
        """EXTENSION, not a reference method: how far the contours of pairs of planes of two engine.SizedMasks lie apart
        -> engine.SurfaceTotals, from which surfeval.surface_metrics gives the Hausdorff distance, ASSD, NSD and the boundary
        F-measure (engine.Cascade.mask_surface_distances)."""
        return self.cascade().mask_surface_distances(a, b, pairs=pairs, tolerance=tolerance, surface=surface, reach=reach)

    def mask_thin_sized(self, sized, *, max_iter=None, path="auto", steps=64):
        """EXTENSION, not a reference method: each plane of an engine.SizedMasks thinned to its centre lines (Guo & Hall; bwmorph's
        'thin') -> engine.MaskThin (engine.Cascade.mask_thin_sized)."""
        return self.cascade().mask_thin_sized(sized, max_iter=max_iter, path=path, steps=steps)

    def mask_cldice(self, a, b, *, pairs=None, a_image=None, b_image=None):
        """EXTENSION, not a reference method: the counts of centre-line Dice of pairs of planes of two engine.SizedMasks
        -> engine.ClDiceTotals, from which surfeval.cldice gives Tprec, Tsens and clDice (engine.Cascade.mask_cldice)."""
        return self.cascade().mask_cldice(a, b, pairs=pairs, a_image=a_image, b_image=b_image)

    def mask_regions_sized(self, sized, *, regions=8, min_area=0, connectivity=8):
        """EXTENSION, not a reference method: each plane of an engine.SizedMasks split into its connected regions, the `regions` largest
        as sized planes of their own -- what scipy.ndimage.label and a loop over its labels give on the host -> engine.MaskRegions,
        whose `compact()` keeps the real regions (engine.Cascade.mask_regions_sized)."""
        return self.cascade().mask_regions_sized(sized, regions=regions, min_area=min_area, connectivity=connectivity)

    def classify_regions(self, regions, plane_of, mask_logits, clip_image, *, image_of=None, vocab=None):
        """EXTENSION, not a reference method: demo.py:117-122 per region -- the alpha of the mask a region came from, gated by the
        region's own pixels, through the Alpha-CLIP tower against that mask's image -> engine.RegionClasses
        (engine.Cascade.classify_regions)."""
        return self.cascade().classify_regions(regions, plane_of, mask_logits.float().contiguous(), clip_image.float().contiguous(),
                                               image_of=image_of, vocab=self._vocab(vocab))

    def mask_nms_sized(self, instances, *, scores, image, category=None, iou=0.5, measure="iou", method="greedy", sigma=2.0):
        """EXTENSION, not a reference method: non-maximum suppression of instance masks across the class hypotheses of each image --
        greedy, or SOLOv2's Matrix NMS -- on an engine.SizedMasks with areas and boxes -> engine.MaskNms, whose `select(instances)`
        keeps the survivors (engine.Cascade.mask_nms_sized)."""
        return self.cascade().mask_nms_sized(instances, scores=scores, image=image, category=category, iou=iou, measure=measure,
                                             method=method, sigma=sigma)

    def mask_rle(self, bits, H, W):
        """EXTENSION, not a reference method: COCO run-length encoding of (N, H * W / 8) uint8 packed masks, e.g. `pack_masks`' bits --
        the "COCO-style RLE" dict the reference's GenericMask takes (models/utils/visualizer.py:72-101) and pycocotools reads
        -> engine.MaskRle, whose `to_coco()` gives the dicts (engine.Cascade.mask_rle)."""
        return self.cascade().mask_rle(bits, H, W)

    def infer_test_multimask(self, input, clip_image, clip_zero_mask, multimask_output=True, all_masks=False, vocab=None):
        """EXTENSION, not a reference method: `infer_test` with the decoder's multimask output -- the candidate masks and the
        quality `iou_pred` the reference's `mask_decoder(..., multimask_output=...)` returns and `infer_test` drops
        (mask_decoder_edge.py:130-135, 163-190).  -> engine.MaskSet ("Multimask output")."""
        H, W = input.shape[-2:]
        assert H == self.inp_size and W == self.inp_size, \
            f"Input image size ({H}*{W}) doesn't match model ({self.inp_size}*{self.inp_size})."
        return self.cascade().infer_test_multimask(input.float().contiguous(), clip_image.float().contiguous(),
                                                   clip_zero_mask.float().contiguous(), multimask_output=multimask_output,
                                                   all_masks=all_masks, vocab=self._vocab(vocab))

    def encode_images(self, input, clip_image, clip_zero_mask, vocab=None):
        """EXTENSION, not a reference method: the SAM encoder, CLIP pass 1 and the decoder's prompt-independent part, once, for
        any number of `decode_classes` calls on the same images.  -> engine.EncodedImages ("Encode once, decode
        many times")."""
        H, W = input.shape[-2:]
        assert H == self.inp_size and W == self.inp_size, \
            f"Input image size ({H}*{W}) doesn't match model ({self.inp_size}*{self.inp_size})."
        return self.cascade().encode(input.float().contiguous(), clip_image.float().contiguous(),
                                     clip_zero_mask.float().contiguous(), vocab=self._vocab(vocab))

    def decode_classes(self, enc, **kw):
        """EXTENSION, not a reference method: K prompts per encoded image -- `classes=`, `topk=` or caller-supplied text rows
        `text=` (what sam_text_proj takes at :342-344), optionally for a subset `images=`, with `quality=` / `stage2=` / `masks=` /
        `overlaps=` / `components=` / `min_area=` / `connectivity=` / `holes=` / `fill_holes=` / `band=` / `edge_threshold=` / `rle=` / `sizes=` / `sized_level=` / `ground_truth=` / `label_maps=` / `label_weights=` / `overlap_threshold=` as engine.Cascade.decode documents them; `vocab=` decodes against another vocabulary than the one the images were encoded
        with.  No encoder launch.  -> engine.ClassHypotheses."""
        self._vocab(kw.get("vocab"))
        return self.cascade().decode(enc, **kw)

    def infer(self, input, clip_image, clip_zero_mask):
        """:305-329 (bs = 1 variant of infer_test)."""
        return self.infer_test(input, clip_image, clip_zero_mask)

    def postprocess_masks(self, masks, input_size, original_size):
        """:359-388 (bilinear, align_corners=False, twice)."""
        B, C, h, w = masks.shape
        S = self.inp_size
        t = torch.empty(B * C, S, S, device=masks.device)
        hip.bilinear(masks.float().contiguous(), B * C, h, w, t, S, S)
        t = t[..., :input_size, :input_size].contiguous()
        out = torch.empty(B * C, original_size, original_size, device=masks.device)
        hip.bilinear(t, B * C, t.shape[-2], t.shape[-1], out, original_size, original_size)
        return out.reshape(B, C, original_size, original_size)

    # ---- training surface: out of scope --------------------------------
    def forward(self, *a, **k):
        raise NotImplementedError("training forward/backward is outside the MI355X inference path")

    set_input = optimize_parameters = backward_G = forward
