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
