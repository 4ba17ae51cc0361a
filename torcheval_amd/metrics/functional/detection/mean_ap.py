"""COCO-style detection mean average precision (bbox, area range "all", no crowd), functional API.

Not in the reference tree (docs/parity.md, "Not in the reference", which holds the definition: the
rules of pycocotools' ``evaluateImg`` and ``accumulate``).  Matching depends on one image only, so it
is a step of its own (``_map_match``) whose result is 12 bytes per detection (score, label, a bit
mask of the thresholds it hit) and a count of ground truths per class; the curves are built from
those (``_map_tables``).  ROCm tensors of the native dtypes run K24
(csrc/kernels/detection_map.hip); CPU tensors, float64 boxes and images with more boxes than the
kernel holds in LDS run the ATen form below, which is the definition written with torch ops in a
loop over images and classes.
"""

from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

import torcheval_amd.ops as _ops
from torcheval_amd.ops import detection as _k24
from torcheval_amd.ops.hostread import read_int

__all__ = ["mean_average_precision"]

_MESSAGES = (
    (_k24.BAD_SCORE, "a NaN score"),
    (_k24.BAD_COORDINATE, "a box with a non-finite coordinate"),
    (_k24.BAD_BOX, "a box with x2 < x1 or y2 < y1"),
    (_k24.BAD_LABEL, "a label outside [0, num_classes)"),
)

Counts = Union[Sequence[int], torch.Tensor]


def _linspace(start: float, stop: float, num: int) -> List[float]:
    """``numpy.linspace(start, stop, num)`` as float64, operation for operation."""
    if num == 1:
        return [float(start)]
    step = (stop - start) / (num - 1)
    out = [i * step + start for i in range(num)]
    out[-1] = float(stop)
    return out


def mean_average_precision(
    pred_boxes: torch.Tensor,
    pred_scores: torch.Tensor,
    pred_labels: torch.Tensor,
    pred_counts: Counts,
    target_boxes: torch.Tensor,
    target_labels: torch.Tensor,
    target_counts: Counts,
    *,
    num_classes: int,
    iou_thresholds: Optional[Sequence[float]] = None,
    max_detections: int = 100,
) -> Dict[str, torch.Tensor]:
    """COCO mean average precision of packed detections against packed ground truths.

    Per image and class the detections are taken by score descending (equal scores in input
    order, the first ``max_detections`` only) and each is matched, per IoU threshold, to the
    not yet matched ground truth of the largest IoU at or above the threshold (the later one among
    equal IoUs).  Per class and threshold the average precision is the mean of the precision
    envelope at the 101 recall points ``0, 0.01, ..., 1``; a class without ground truth is NaN and
    enters no mean.  Boxes are ``(x1, y1, x2, y2)`` in continuous coordinates; the IoU is evaluated
    in FP64.

    Class version: ``MeanAveragePrecision``.

    Args:
        pred_boxes: ``[M, 4]`` floating boxes of all images, image after image.
        pred_scores: ``[M]`` floating scores (taken as float32).
        pred_labels: ``[M]`` int64 / int32 classes.
        pred_counts: image ``i`` owns the next ``pred_counts[i]`` rows: a sequence of integers or a
            CPU integer tensor (host values, so passing them costs no synchronisation).
        target_boxes: ``[G, 4]`` floating ground-truth boxes.
        target_labels: ``[G]`` int64 / int32 classes.
        target_counts: as ``pred_counts``, of the same length.
        num_classes: the labels lie in ``[0, num_classes)``.
        iou_thresholds: 1 to 16 values in ``(0, 1]``; default ``numpy.linspace(0.5, 0.95, 10)``.
        max_detections: detections kept per image and class.

    A NaN score, a non-finite coordinate, ``x2 < x1`` or ``y2 < y1`` and a label outside
    ``[0, num_classes)`` raise on CPU; on ROCm the detection or ground truth is counted nowhere and
    the call raises only under ``config.validate``.

    Returns a dict of float32 tensors on the inputs' device: ``map``, ``map_50``, ``map_75`` (NaN
    when the threshold is not in the table), ``mar`` (recall at ``max_detections``), and
    ``map_per_class`` / ``mar_per_class`` ``[num_classes]``.
    """
    thresholds = _map_param_check(num_classes, iou_thresholds, max_detections)
    pc, tc = _map_input_check(pred_boxes, pred_scores, pred_labels, pred_counts, target_boxes, target_labels,
                              target_counts)
    with torch.inference_mode():
        from torcheval_amd.config import config

        err = torch.zeros(1, dtype=torch.int32, device=pred_boxes.device) if pred_boxes.is_cuda and config.validate else None
        scores, labels, hits, gt_count, _ = _map_match(pred_boxes, pred_scores, pred_labels, pc, target_boxes,
                                                       target_labels, tc, num_classes, thresholds, max_detections, err)
        _raise_on_bad_input(err)
        return _map_value(scores, labels, hits, gt_count, thresholds)


# ----------------------------------------------------------------------------- checks
def _map_param_check(num_classes: int, iou_thresholds, max_detections: int) -> torch.Tensor:
    """Checks the parameters; returns the float64 threshold table (CPU)."""
    if not isinstance(num_classes, int) or isinstance(num_classes, bool) or num_classes < 1:
        raise ValueError(f"`num_classes` should be a positive integer, got {num_classes!r}.")
    if not isinstance(max_detections, int) or isinstance(max_detections, bool) or max_detections < 1:
        raise ValueError(f"`max_detections` should be a positive integer, got {max_detections!r}.")
    if iou_thresholds is None:
        return torch.tensor(_linspace(0.5, 0.95, 10), dtype=torch.float64)
    table = torch.as_tensor(iou_thresholds, dtype=torch.float64).detach().cpu()
    if table.dim() != 1 or not 1 <= table.numel() <= _k24.MAX_THRESHOLDS:
        raise ValueError(
            f"`iou_thresholds` should hold 1 to {_k24.MAX_THRESHOLDS} values, got shape {tuple(table.shape)}.")
    if not bool(((table > 0) & (table <= 1)).all()):
        raise ValueError(f"`iou_thresholds` should lie in (0, 1], got {table.tolist()}.")
    return table.clone()


def _counts(counts: Counts, name: str) -> List[int]:
    if isinstance(counts, torch.Tensor):
        if counts.is_cuda or counts.is_floating_point() or counts.dtype == torch.bool or counts.dim() != 1:
            raise ValueError(f"`{name}` should be a sequence of integers or a 1-d CPU integer tensor.")
        counts = counts.tolist()
    out = []
    for v in counts:
        if not isinstance(v, int) or isinstance(v, bool) or v < 0:
            raise ValueError(f"`{name}` should hold non-negative integers, got {v!r}.")
        out.append(v)
    return out


def _map_input_check(pred_boxes, pred_scores, pred_labels, pred_counts, target_boxes, target_labels,
                     target_counts) -> Tuple[List[int], List[int]]:
    for name, boxes in (("pred_boxes", pred_boxes), ("target_boxes", target_boxes)):
        if not boxes.is_floating_point():
            raise ValueError(f"{name} should hold floating coordinates, got dtype {boxes.dtype}.")
        if boxes.dim() != 2 or boxes.shape[1] != 4:
            raise ValueError(f"{name} should be [N, 4] boxes (x1, y1, x2, y2), got shape {tuple(boxes.shape)}.")
    if not pred_scores.is_floating_point():
        raise ValueError(f"pred_scores should be floating, got dtype {pred_scores.dtype}.")
    for name, labels in (("pred_labels", pred_labels), ("target_labels", target_labels)):
        if labels.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"{name} should be int64 or int32 classes, got dtype {labels.dtype}.")
    if pred_scores.shape != pred_boxes.shape[:1] or pred_labels.shape != pred_boxes.shape[:1]:
        raise ValueError(
            f"pred_scores and pred_labels should be [M] for [M, 4] boxes, got shapes {tuple(pred_scores.shape)}, "
            f"{tuple(pred_labels.shape)} and {tuple(pred_boxes.shape)}.")
    if target_labels.shape != target_boxes.shape[:1]:
        raise ValueError(
            f"target_labels should be [G] for [G, 4] boxes, got shapes {tuple(target_labels.shape)} and "
            f"{tuple(target_boxes.shape)}.")
    pc, tc = _counts(pred_counts, "pred_counts"), _counts(target_counts, "target_counts")
    if len(pc) != len(tc):
        raise ValueError(f"pred_counts and target_counts should list the same images, got {len(pc)} and {len(tc)}.")
    if sum(pc) != pred_boxes.shape[0] or sum(tc) != target_boxes.shape[0]:
        raise ValueError(
            f"The counts should sum to the row counts: {sum(pc)} of {pred_boxes.shape[0]} detections and "
            f"{sum(tc)} of {target_boxes.shape[0]} ground truths.")
    return pc, tc


def _bad_input_message(code: int) -> str:
    return "detection metric: the input holds " + "; ".join(m for bit, m in _MESSAGES if code & bit)


def _raise_on_bad_input(err: Optional[torch.Tensor]) -> None:
    """Surface (and clear) the device flag of bad detections and ground truths."""
    if err is None:
        return
    code = read_int(err)
    if code != 0:
        err.zero_()
        raise ValueError(_bad_input_message(code) + " (such boxes were counted nowhere).")


# ----------------------------------------------------------------------------- matching
def _map_match(pred_boxes: torch.Tensor, pred_scores: torch.Tensor, pred_labels: torch.Tensor, pred_counts: List[int],
               target_boxes: torch.Tensor, target_labels: torch.Tensor, target_counts: List[int], num_classes: int,
               thresholds: torch.Tensor, max_detections: int, err: Optional[torch.Tensor] = None,
               want_matched: bool = False):
    """The matching of checked inputs, from whichever path the tensors take: ``(scores f32 [M],
    labels i32 [M], hits i32 [M], gt_count f64 [C], matched_gt i32 [M, T] or None)``.  Every image's
    detections come in the matching order (class, score descending, input order); a dropped
    detection (past ``max_detections``, or bad on ROCm) has label -1 and no hits.  Bit ``k`` of
    ``hits`` says the detection matched under threshold ``k``; ``matched_gt`` (tests) is the index
    within the image of the ground truth it matched, or -1."""
    if _k24.supported(pred_boxes, pred_scores, pred_labels, pred_counts, target_boxes, target_labels, target_counts,
                      num_classes):
        s, l, h, g, m = _k24.map_match(pred_boxes, pred_scores, pred_labels, target_boxes, target_labels,
                                       _k24.offsets_of(pred_counts, target_counts),
                                       thresholds.to(pred_boxes.device), num_classes, max_detections, err,
                                       want_matched)
        return s, l, h, g.double(), m
    return _map_match_aten(pred_boxes, pred_scores, pred_labels, pred_counts, target_boxes, target_labels,
                           target_counts, num_classes, thresholds, max_detections, err, want_matched)


def _box_iou(d: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """``[len(d), len(g)]`` IoUs of float64 boxes: one rounded FP64 operation per step of the
    definition (no fused multiply-add), so every path decides a threshold compare alike."""
    area_d = (d[:, 2] - d[:, 0]) * (d[:, 3] - d[:, 1])
    area_g = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    iw = (torch.minimum(d[:, None, 2], g[None, :, 2]) - torch.maximum(d[:, None, 0], g[None, :, 0])).clamp(min=0.0)
    ih = (torch.minimum(d[:, None, 3], g[None, :, 3]) - torch.maximum(d[:, None, 1], g[None, :, 1])).clamp(min=0.0)
    inter = iw * ih
    union = (area_d[:, None] + area_g[None, :]) - inter
    positive = union > 0
    return torch.where(positive, inter / torch.where(positive, union, 1.0), 0.0)


def _bad_rows(boxes: torch.Tensor, labels: torch.Tensor, num_classes: int):
    nonfinite = ~torch.isfinite(boxes).all(dim=1)
    inverted = ~nonfinite & ((boxes[:, 2] < boxes[:, 0]) | (boxes[:, 3] < boxes[:, 1]))
    label = (labels < 0) | (labels >= num_classes)
    return nonfinite, inverted, label


def _map_match_aten(pred_boxes, pred_scores, pred_labels, pred_counts, target_boxes, target_labels, target_counts,
                    num_classes, thresholds, max_detections, err=None, want_matched=False):
    """The definition with torch ops: a loop over images, classes and kept detections, vectorised
    over the class's ground truths and the thresholds.  Slow and plain; also the CPU path."""
    dev = pred_boxes.device
    target_boxes, target_labels = target_boxes.to(dev), target_labels.to(dev)
    m, t = pred_boxes.shape[0], thresholds.shape[0]
    d, g = pred_boxes.double(), target_boxes.double()
    s = pred_scores.to(dev).float()
    pl, tl = pred_labels.to(dev).long(), target_labels.long()
    nan_score = torch.isnan(s)
    d_nonfinite, d_inverted, d_label = _bad_rows(d, pl, num_classes)
    g_nonfinite, g_inverted, g_label = _bad_rows(g, tl, num_classes)
    kinds = (nan_score.any(), d_nonfinite.any() | g_nonfinite.any(), d_inverted.any() | g_inverted.any(),
             d_label.any() | g_label.any())
    if not pred_boxes.is_cuda:
        code = sum(int(bool(v)) << i for i, v in enumerate(kinds))
        if code != 0:
            raise ValueError(_bad_input_message(code) + ".")
    elif err is not None:
        err.bitwise_or_(sum(v.to(err.dtype) << i for i, v in enumerate(kinds)))
    bad_d = nan_score | d_nonfinite | d_inverted | d_label
    bad_g = g_nonfinite | g_inverted | g_label
    sort_label = torch.where(bad_d, num_classes, pl)
    sort_score = torch.where(bad_d, 0.0, s + 0.0)  # -0.0 + 0.0 is +0.0; a bad detection keeps its place
    gt_label = torch.where(bad_g, -1, tl)
    tmin = torch.minimum(thresholds.to(dev), torch.tensor(1 - 1e-10, dtype=torch.float64, device=dev))
    bits = torch.arange(t, device=dev, dtype=torch.int32)
    rows_t = torch.arange(t, device=dev)

    out_scores = torch.empty(m, dtype=torch.float32, device=dev)
    out_labels = torch.full((m,), -1, dtype=torch.int32, device=dev)
    out_hits = torch.zeros(m, dtype=torch.int32, device=dev)
    matched = torch.full((m, t), -1, dtype=torch.int32, device=dev) if want_matched else None
    d0 = g0 = 0
    for nd, ng in zip(pred_counts, target_counts):
        d1, g1 = d0 + nd, g0 + ng
        if nd:
            first = torch.sort(sort_score[d0:d1], descending=True, stable=True).indices
            second = torch.sort(sort_label[d0:d1][first], stable=True)
            order = first[second.indices] + d0
            out_scores[d0:d1] = s[order]
            classes, sizes = torch.unique_consecutive(second.values, return_counts=True)
            pos = d0
            for c, n in zip(classes.tolist(), sizes.tolist()):
                kept = min(n, max_detections)
                if c < num_classes:
                    out_labels[pos:pos + kept] = c
                    gi = torch.nonzero(gt_label[g0:g1] == c).flatten()
                    if gi.numel():
                        iou = _box_iou(d[order[pos - d0:pos - d0 + kept]], g[g0:g1][gi])
                        taken = torch.zeros(t, gi.numel(), dtype=torch.bool, device=dev)
                        for j in range(kept):
                            row = iou[j][None, :]
                            value = torch.where(~taken & (row >= tmin[:, None]), row, -1.0)
                            has = value.max(dim=1).values >= 0
                            last = gi.numel() - 1 - value.flip(1).argmax(dim=1)  # the later of equal IoUs
                            taken[rows_t, last] |= has
                            out_hits[pos + j] = (has.to(torch.int32) << bits).sum()
                            if matched is not None:
                                matched[pos + j] = torch.where(has, gi[last], -1).to(torch.int32)
                pos += n
        d0, g0 = d1, g1
    gt_count = torch.bincount(gt_label[gt_label >= 0], minlength=num_classes).double()
    return out_scores, out_labels, out_hits, gt_count, matched


# ----------------------------------------------------------------------------- curves
def _map_order(scores: torch.Tensor, labels: torch.Tensor, num_classes: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The global order (label, score descending, stored order) with dropped detections last, and
    the int64 ``[C + 1]`` offsets of the classes in it; ATen on the tensors' device, no host read."""
    label = torch.where(labels < 0, num_classes, labels.long())
    first = torch.sort(scores + 0.0, descending=True, stable=True).indices
    second = torch.sort(label[first], stable=True)
    offsets = torch.searchsorted(second.values, torch.arange(num_classes + 1, device=labels.device))
    return first[second.indices], offsets


def _map_tables(scores: torch.Tensor, labels: torch.Tensor, hits: torch.Tensor, gt_count: torch.Tensor,
                num_thresholds: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The float64 ``AP`` and ``REC`` tables ``[T, C]`` of stored detections."""
    order, offsets = _map_order(scores, labels, gt_count.shape[0])
    if _ops.use_native(hits) and hits.shape[0] < 2**31:
        return _k24.map_curve(hits[order].contiguous(), offsets, gt_count, num_thresholds)[:2]
    return _map_tables_aten(hits[order], offsets, gt_count, num_thresholds)


def _map_tables_aten(hits: torch.Tensor, offsets: torch.Tensor, gt_count: torch.Tensor,
                     num_thresholds: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The 101-point definition per class with a ground truth, all thresholds at once."""
    dev, c, t = hits.device, gt_count.shape[0], num_thresholds
    ap = torch.full((t, c), torch.nan, dtype=torch.float64, device=dev)
    rec = torch.full((t, c), torch.nan, dtype=torch.float64, device=dev)
    grid = torch.tensor(_linspace(0.0, 1.0, 101), dtype=torch.float64, device=dev)[None, :].expand(t, 101).contiguous()
    bits = torch.arange(t, device=dev)
    bounds = offsets.tolist()
    for k in torch.nonzero(gt_count > 0).flatten().tolist():
        lo, hi = bounds[k], bounds[k + 1]
        n = hi - lo
        if n == 0:
            ap[:, k] = 0.0
            rec[:, k] = 0.0
            continue
        hit = ((hits[lo:hi, None] >> bits) & 1).double()
        tp = torch.cumsum(hit, dim=0)
        fp = torch.arange(1, n + 1, device=dev, dtype=torch.float64)[:, None] - tp
        recall = tp / gt_count[k]
        precision = tp / (fp + tp + 2.0**-52)
        envelope = torch.cummax(precision.flip(0), dim=0).values.flip(0)
        at = torch.searchsorted(recall.T.contiguous(), grid)  # [T, 101], the first j with rec_j >= r_q
        sample = torch.where(at < n, envelope.T.gather(1, at.clamp(max=n - 1)), 0.0)
        ap[:, k] = sample.sum(dim=1) / 101.0
        rec[:, k] = tp[-1] / gt_count[k]
    return ap, rec


def _nan_mean(x: torch.Tensor) -> torch.Tensor:
    valid = ~torch.isnan(x)
    n = valid.sum()
    return torch.where(n > 0, torch.where(valid, x, 0.0).sum() / n.clamp(min=1), torch.nan)


def _threshold_index(thresholds: torch.Tensor, value: float) -> int:
    table = thresholds.tolist()
    return table.index(value) if value in table else -1


def _map_value(scores: torch.Tensor, labels: torch.Tensor, hits: torch.Tensor, gt_count: torch.Tensor,
               thresholds: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The dict of results of stored detections; ``thresholds`` is the CPU table."""
    t, c = thresholds.shape[0], gt_count.shape[0]
    i50, i75 = _threshold_index(thresholds, 0.5), _threshold_index(thresholds, 0.75)
    if _ops.use_native(hits) and gt_count.device == hits.device and hits.shape[0] < 2**31:
        order, offsets = _map_order(scores, labels, c)
        _, _, scalars, map_c, mar_c = _k24.map_curve(hits[order].contiguous(), offsets, gt_count, t, i50, i75)
        return {"map": scalars[0], "map_50": scalars[1], "map_75": scalars[2], "mar": scalars[3],
                "map_per_class": map_c, "mar_per_class": mar_c}
    ap, rec = _map_tables(scores, labels, hits, gt_count, t)
    nan = torch.full((), torch.nan, dtype=torch.float64, device=ap.device)
    out = {
        "map": _nan_mean(ap),
        "map_50": _nan_mean(ap[i50]) if i50 >= 0 else nan,
        "map_75": _nan_mean(ap[i75]) if i75 >= 0 else nan,
        "mar": _nan_mean(rec),
        "map_per_class": ap.mean(dim=0),
        "mar_per_class": rec.mean(dim=0),
    }
    return {k: v.to(torch.float32) for k, v in out.items()}
