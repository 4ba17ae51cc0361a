"""The numpy oracle of segmentation mean IoU and Dice (docs/parity.md, "Not in the reference"),
shared by tests/metrics/classification/test_mean_iou.py and tests/gpu/test_k17_segmentation.py:
int64 counts by ``np.bincount`` on the definition, values in FP64.  ``sklearn_values`` is a second
opinion on the per-class and micro values, from ``jaccard_score`` and ``f1_score``."""

import numpy as np


def argmax_first(x: np.ndarray) -> np.ndarray:
    """``torch.argmax(x, dim=1)``'s rule on ``[N, C, *spatial]`` scores: the lowest class among the
    maxima, NaN the maximum and the first NaN the winner (numpy's rule too); -0.0 ties +0.0."""
    return np.argmax(x.astype(np.float64), axis=1)


def counts(pred: np.ndarray, target: np.ndarray, num_classes: int, ignore_index=None, drop_bad=False):
    """int64 ``[num_classes]`` (intersection, pred_count, target_count) over the counted pixels of
    two label maps of one shape.  ``drop_bad`` leaves out counted pixels with a label outside
    ``[0, num_classes)`` (what the ROCm path does with them); without it they are an error."""
    p = pred.reshape(-1).astype(np.int64)
    t = target.reshape(-1).astype(np.int64)
    keep = np.ones(t.shape, dtype=bool) if ignore_index is None else t != ignore_index
    ok = (t >= 0) & (t < num_classes) & (p >= 0) & (p < num_classes)
    assert drop_bad or ok[keep].all()
    keep &= ok
    p, t = p[keep], t[keep]
    return (np.bincount(t[t == p], minlength=num_classes), np.bincount(p, minlength=num_classes),
            np.bincount(t, minlength=num_classes))


def value(intersection, pred_count, target_count, dice: bool, average: str):
    """FP64 value: a float for ``"macro"`` / ``"micro"``, a ``[C]`` vector for ``"none"``."""
    i, both = intersection.astype(np.float64), (pred_count + target_count).astype(np.float64)
    union = both - i
    top, bottom = (2.0 * i, both) if dice else (i, union)
    with np.errstate(invalid="ignore", divide="ignore"):
        per_class = top / bottom  # 0 / 0 = NaN: a class absent from both maps
        if average == "none":
            return per_class
        if average == "micro":
            return float(top.sum() / bottom.sum())
        present = union > 0
        return float(per_class[present].mean()) if present.any() else float("nan")


def sklearn_values(pred: np.ndarray, target: np.ndarray, num_classes: int, ignore_index, dice: bool):
    """(per-class values on the classes with ``union > 0``, those classes, micro value) by
    scikit-learn, of label maps whose counted labels are all in range."""
    from sklearn.metrics import f1_score, jaccard_score

    p, t = pred.reshape(-1).astype(np.int64), target.reshape(-1).astype(np.int64)
    if ignore_index is not None:
        p, t = p[t != ignore_index], t[t != ignore_index]
    labels = np.union1d(p, t)
    fn = f1_score if dice else jaccard_score
    return fn(t, p, labels=labels, average=None), labels, float(fn(t, p, labels=labels, average="micro"))
