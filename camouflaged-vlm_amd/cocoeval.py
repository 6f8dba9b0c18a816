"""COCO precision / recall accumulation on the host: the published COCOeval.accumulate and summarize in float64, over the
matches cvlm_coco_match left on the device (engine.CocoMatches, read back once each).  Pure numpy, like rle.py; no pycocotools.

    matches = cascade.coco_match(dets, gts, scores=..., det_image=..., gt_image=..., det_category=..., gt_category=...)
    stats = summarize(accumulate(matches))          # AP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl

A dataset evaluated in batches gives a list of CocoMatches: `accumulate` takes the list; the categories are the union, the groups are
concatenated in the order of the list and, inside one CocoMatches, in its own order (category, image) -- pycocotools' order when the
batches follow the sorted image ids, which matters only for detections of equal score.
"""
from __future__ import annotations

import numpy as np

MAX_DETS = (1, 10, 100)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)


def _host(m) -> dict:
    if isinstance(m, dict):
        return m
    if not hasattr(m, "to_host"):
        raise ValueError(f"accumulate: a CocoMatches, its to_host() dict, or a list of them, got {type(m).__name__}")
    return m.to_host()


def accumulate(matches, *, max_dets=MAX_DETS, rec_thrs=None) -> dict:
    """COCOeval.accumulate over one CocoMatches (or its `to_host()` dict) or a list of them -> dict(precision [T, R, K, A, M], recall
    [T, K, A, M], scores [T, R, K, A, M], all -1 where nothing was evaluated; categories: the K category ids, [None] without categories;
    iou_thrs, area_rngs, rec_thrs, max_dets).  Per (category, area range, max_dets entry): the first m ranks of every group, stably
    sorted by -score; tp = matched and not ignored, fp = unmatched and not ignored; the cell is skipped when no annotation of it counts.
    ValueError: parameters that differ between the parts, parts with and without categories, max_dets not ascending ints >= 1 or beyond
    the matching's max_det, a part in which a group was refused."""
    parts = [_host(m) for m in (matches if isinstance(matches, (list, tuple)) else [matches])]
    if not parts:
        raise ValueError("accumulate: no matches")
    first = parts[0]
    thrs, rngs = np.asarray(first["iou_thrs"], dtype=np.float64), np.asarray(first["area_rngs"], dtype=np.float64)
    for h in parts:
        if not np.array_equal(h["iou_thrs"], thrs) or not np.array_equal(h["area_rngs"], rngs) or h["max_det"] != first["max_det"]:
            raise ValueError("accumulate: the parts were matched with different iou_thrs, area_rngs or max_det")
        if h["status"] != 0:
            raise ValueError("accumulate: a part holds a refused group (CocoMatches.check())")
    max_dets = tuple(max_dets)
    if not max_dets or any(isinstance(m, bool) or not isinstance(m, (int, np.integer)) or m < 1 for m in max_dets) \
            or list(max_dets) != sorted(set(max_dets)) or max_dets[-1] > first["max_det"]:
        raise ValueError(f"accumulate: max_dets must be ascending ints in [1, {first['max_det']}], the matching's max_det")
    rec = REC_THRS if rec_thrs is None else np.asarray(rec_thrs, dtype=np.float64)
    if rec.ndim != 1 or rec.size < 1:
        raise ValueError("accumulate: rec_thrs must be a flat sequence of numbers")
    with_cats = {k[0] is not None for h in parts for k in h["keys"]}
    if len(with_cats) > 1:
        raise ValueError("accumulate: parts with and without categories do not mix")
    cats = sorted({k[0] for h in parts for k in h["keys"]}) if with_cats == {True} else [None]
    T, R, K, A, M = thrs.size, rec.size, len(cats), rngs.shape[0], len(max_dets)
    precision, recall, scores = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M)), -np.ones((T, R, K, A, M))
    for ki, cat in enumerate(cats):
        groups = [(h, e) for h in parts for e, key in enumerate(h["keys"]) if key[0] == cat]
        if not groups:
            continue
        for a in range(A):
            gt_ig = np.concatenate([h["gt_ignore"][a, h["gt_offsets"][e]:h["gt_offsets"][e + 1]] for h, e in groups])
            npig = int(np.count_nonzero(gt_ig == 0))
            if npig == 0:
                continue
            for mi, m in enumerate(max_dets):
                sc, dtm, dig = [], [], []
                for h, e in groups:
                    d0 = int(h["det_offsets"][e])
                    d1 = min(int(h["det_offsets"][e + 1]), d0 + m)
                    sc.append(h["score"][h["dt_order"][d0:d1]])
                    dtm.append(h["dt_match"][a, :, d0:d1])
                    dig.append(h["dt_ignore"][a, :, d0:d1])
                sc = np.concatenate(sc)
                inds = np.argsort(-sc, kind="mergesort")
                sc = sc[inds]
                matched = np.concatenate(dtm, axis=1)[:, inds] >= 0
                ignored = np.concatenate(dig, axis=1)[:, inds] != 0
                tp_sum = np.cumsum(matched & ~ignored, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(~matched & ~ignored, axis=1).astype(dtype=float)
                nd = sc.size
                for t in range(T):
                    tp, fp = tp_sum[t], fp_sum[t]
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, ki, a, mi] = rc[-1] if nd else 0
                    pr = np.maximum.accumulate(pr[::-1])[::-1]         # the right-to-left monotone envelope
                    at = np.searchsorted(rc, rec, side="left")
                    ok = at < nd                                      # positions past the end leave 0
                    q, ss = np.zeros(R), np.zeros(R)
                    q[ok], ss[ok] = pr[at[ok]], sc[at[ok]]
                    precision[t, :, ki, a, mi], scores[t, :, ki, a, mi] = q, ss
    return dict(precision=precision, recall=recall, scores=scores, categories=cats, iou_thrs=thrs, area_rngs=rngs, rec_thrs=rec, max_dets=max_dets)


def summarize(acc: dict) -> list:
    """COCOeval.summarize's twelve numbers from `accumulate`'s result: AP, AP at IoU 0.5 and 0.75, AP small / medium / large -- at
    max_dets[-1] --, AR at each of the three max_dets, AR small / medium / large; each the mean over the entries > -1, or -1 if there are
    none.  It reads area ranges 0 .. 3 as all / small / medium / large and wants three max_dets (ValueError otherwise); a threshold that
    was not matched (0.5, 0.75) gives -1."""
    thrs, max_dets = np.asarray(acc["iou_thrs"]), acc["max_dets"]
    if acc["precision"].shape[3] < 4 or len(max_dets) != 3:
        raise ValueError("summarize: the twelve numbers need four area ranges (all, small, medium, large) and three max_dets")

    def one(ap: bool, iou=None, a: int = 0, m: int = 2) -> float:
        s = acc["precision"] if ap else acc["recall"]
        if iou is not None:
            s = s[np.where(iou == thrs)[0]]
        s = s[:, :, :, a, m] if ap else s[:, :, a, m]
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0

    return [one(True), one(True, iou=.5), one(True, iou=.75), one(True, a=1), one(True, a=2), one(True, a=3),
            one(False, m=0), one(False, m=1), one(False, m=2), one(False, a=1), one(False, a=2), one(False, a=3)]
