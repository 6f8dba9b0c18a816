"""Semantic-segmentation metrics from the totals of Cascade.label_iou: the divisions of mmseg's `eval_metrics`
(models/mmseg/core/evaluation/metrics.py:179-229) in float64 on the host.  Pure numpy: no device, no torch.

totals is int64 (3, C) = (area_intersect, area_pred_label, area_label) summed over a dataset's images; area_union is their sum minus
the intersection.  A class that occurs neither in the predictions nor in the ground truth divides 0 by 0 and is NaN, as there;
`nan_to_num` replaces it, the means skip it (mmseg's evaluate() takes np.nanmean of the per-class values)."""
import numpy as np

METRICS = ("mIoU", "mDice")


def _totals(totals) -> np.ndarray:
    t = np.asarray(totals.cpu().numpy() if hasattr(totals, "cpu") else totals)
    if t.ndim != 2 or t.shape[0] != 3 or t.shape[1] < 1 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"segeval: totals must be integers of shape (3, C), got {t.dtype} {t.shape}")
    return t.astype(np.float64)


def eval_metrics(totals, metrics=("mIoU",), nan_to_num=None) -> list:
    """-> [all_acc, acc (C,), then per metric of `metrics` its per-class values (C,)]: all_acc = sum intersect / sum label, acc =
    intersect / label, IoU = intersect / (pred + label - intersect), Dice = 2 intersect / (pred + label)."""
    if isinstance(metrics, str):
        metrics = [metrics]
    if not set(metrics).issubset(METRICS):
        raise KeyError(f"metrics {list(metrics)} is not supported")
    inter, pred, label = _totals(totals)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = [inter.sum() / label.sum(), inter / label]
        for m in metrics:
            out.append(inter / (pred + label - inter) if m == "mIoU" else 2 * inter / (pred + label))
    if nan_to_num is not None:
        out = [np.nan_to_num(v, nan=nan_to_num) for v in out]
    return out


def mean_iou(totals, nan_to_num=None) -> float:
    """The benchmark's number: the mean over classes of IoU, classes that are NaN left out."""
    return float(np.nanmean(eval_metrics(totals, ("mIoU",), nan_to_num)[2]))


def mean_dice(totals, nan_to_num=None) -> float:
    return float(np.nanmean(eval_metrics(totals, ("mDice",), nan_to_num)[2]))


def pq_average(counts, iou_sum, isthing=None) -> dict:
    """Panoptic quality from the totals of Cascade.panoptic_quality, panopticapi's PQStat.pq_average in float64 ->
    {"All" | "Things" | "Stuff": {"pq", "sq", "rq", "n"}, "per_class": {"pq", "sq", "rq"} (C,)}.  counts: integers (3, C) = tp, fp, fn;
    iou_sum: reals (C,); isthing: bools (C,), without which only "All" is returned.  Per class with tp + fp + fn > 0: pq = iou_sum / (tp
    + fp / 2 + fn / 2), sq = iou_sum / tp (0 where tp = 0), rq = tp / (tp + fp / 2 + fn / 2); a class without any count has zeros in the
    per-class table and is left out of the means and of n.  A group with n = 0 is NaN (the published code divides by zero)."""
    c = np.asarray(counts.cpu().numpy() if hasattr(counts, "cpu") else counts)
    s = np.asarray(iou_sum.cpu().numpy() if hasattr(iou_sum, "cpu") else iou_sum, dtype=np.float64)
    if c.ndim != 2 or c.shape[0] != 3 or c.shape[1] < 1 or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f"segeval: counts must be integers of shape (3, C), got {c.dtype} {c.shape}")
    if s.shape != (c.shape[1],):
        raise ValueError(f"segeval: iou_sum must hold one real per class, ({c.shape[1]},), got {s.shape}")
    tp, fp, fn = c.astype(np.float64)
    seen = tp + fp + fn > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        den = tp + 0.5 * fp + 0.5 * fn
        pq = np.where(seen, s / den, 0.0)
        sq = np.where(tp != 0, s / tp, 0.0)
        rq = np.where(seen, tp / den, 0.0)
    groups = {"All": np.ones_like(seen)}
    if isthing is not None:
        thing = np.asarray(isthing)
        if thing.shape != seen.shape or thing.dtype != np.bool_:
            raise ValueError(f"segeval: isthing must be bools of shape {seen.shape}, got {thing.dtype} {thing.shape}")
        groups.update(Things=thing, Stuff=~thing)
    out = {"per_class": {"pq": pq, "sq": sq, "rq": rq}}
    for name, members in groups.items():
        sel = seen & members
        n = int(sel.sum())
        mean = lambda v: float(v[sel].sum() / n) if n else float("nan")
        out[name] = {"pq": mean(pq), "sq": mean(sq), "rq": mean(rq), "n": n}
    return out
