"""K24 wrapper (csrc/kernels/detection_map.hip): COCO-style detection mean average precision.

``map_match`` is one launch per call.  A workgroup takes an image at a time (the grid is
persistent over the images): it stages the image's boxes in LDS, orders the detections by one u64
key ``label << 42 | ~orderable(score) << 10 | index`` and the ground truths by ``label << 10 |
index`` with an LDS bitonic sort, and then its waves share the class segments; per kept detection
a wave forms its FP64 IoUs with the class's ground truths, 64 at a time, and per threshold picks the
unmatched ground truth of the largest IoU (the later one among equals).  It emits ``(score, label,
hits)`` per detection in the matching order and adds the ground truths per class into an int64
vector with integer atomics.  ``map_curve`` is two launches: a workgroup per (class, threshold)
walks the class's hits from the right (count, scan, precision, suffix maximum) and sums the
101-point interpolation in its count form, and one workgroup takes the means.

The image offsets are host integers and reach the device as one small copy inside the op, which
checks them first (sorted, every image within ``max_boxes()``, ends at the row counts): the kernel
never reads a row the host has not vouched for.  No host read, no float atomics.  All ops are
dispatcher ops only (``torch.ops.torcheval_amd_detection``).
"""

from typing import Optional, Sequence, Tuple

import torch

from torcheval_amd.ops import use_native

# kMapMaxBoxes, kMapBlock, kMapGrid, kMapMaxThresholds, kMapMaxClasses, kMapCurveChunk and
# kMapCurveGrid of csrc/include/tea_kernels.h (held equal by tests/metrics/detection/test_mean_ap.py)
MAX_BOXES = 1024
BLOCK = 256
GRID = 768
MAX_THRESHOLDS = 16
MAX_CLASSES = (1 << 22) - 1
CURVE_CHUNK = 256
CURVE_GRID = 4096

# bits of the device flag
BAD_SCORE = 1  # a NaN score
BAD_COORDINATE = 2  # a non-finite coordinate
BAD_BOX = 4  # x2 < x1 or y2 < y1
BAD_LABEL = 8  # a label outside [0, num_classes)

_BOX_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_LABEL_DTYPES = (torch.int64, torch.int32)


def max_boxes() -> int:
    """The most detections, and the most ground truths, of one image that K24 matches in LDS."""
    return MAX_BOXES


def supported(pred_boxes: torch.Tensor, pred_scores: torch.Tensor, pred_labels: torch.Tensor,
              pred_counts: Sequence[int], target_boxes: torch.Tensor, target_labels: torch.Tensor,
              target_counts: Sequence[int], num_classes: int) -> bool:
    """Whether a checked call runs ``map_match``: ROCm tensors of the native dtypes on one device,
    every image within ``max_boxes()`` and ``num_classes < 2^22``.  Raises on a GPU without the
    extension (``use_native``)."""
    if not use_native(pred_boxes):
        return False
    dev = pred_boxes.device
    if any(t.device != dev for t in (pred_scores, pred_labels, target_boxes, target_labels)):
        return False
    if pred_boxes.dtype not in _BOX_DTYPES or target_boxes.dtype not in _BOX_DTYPES:
        return False
    if pred_scores.dtype not in _BOX_DTYPES:
        return False
    if pred_labels.dtype not in _LABEL_DTYPES or target_labels.dtype not in _LABEL_DTYPES:
        return False
    if num_classes > MAX_CLASSES or pred_boxes.shape[0] >= 2**31 or target_boxes.shape[0] >= 2**31:
        return False
    return max(pred_counts, default=0) <= MAX_BOXES and max(target_counts, default=0) <= MAX_BOXES


def offsets_of(pred_counts: Sequence[int], target_counts: Sequence[int]) -> torch.Tensor:
    """CPU int64 ``[2, B + 1]``: the first detection row and the first ground-truth row of every
    image, and the totals."""
    out = torch.zeros(2, len(pred_counts) + 1, dtype=torch.int64)
    if len(pred_counts):
        out[0, 1:] = torch.cumsum(torch.as_tensor(pred_counts, dtype=torch.int64), 0)
        out[1, 1:] = torch.cumsum(torch.as_tensor(target_counts, dtype=torch.int64), 0)
    return out


def map_match(pred_boxes: torch.Tensor, pred_scores: torch.Tensor, pred_labels: torch.Tensor,
              target_boxes: torch.Tensor, target_labels: torch.Tensor, offsets: torch.Tensor,
              thresholds: torch.Tensor, num_classes: int, max_detections: int,
              err: Optional[torch.Tensor] = None, want_matched: bool = False,
              ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """One ``map_match`` launch of a ``supported`` call: ``(scores f32 [M], labels i32 [M], hits i32
    [M], gt_count i64 [C], matched_gt i32 [M, T] or None)``, the detections of every image in the
    matching order.  ``offsets`` is ``offsets_of`` (CPU), ``thresholds`` float64 ``[T]`` on the
    device."""
    dev = pred_boxes.device
    m, t = pred_boxes.shape[0], thresholds.shape[0]
    if pred_boxes.dtype != torch.float32:
        pred_boxes = pred_boxes.float()
    if target_boxes.dtype != torch.float32:
        target_boxes = target_boxes.float()
    scores = torch.empty(m, dtype=torch.float32, device=dev)
    labels = torch.empty(m, dtype=torch.int32, device=dev)
    hits = torch.empty(m, dtype=torch.int32, device=dev)
    gt_count = torch.zeros(num_classes, dtype=torch.int64, device=dev)
    matched = torch.empty(m, t, dtype=torch.int32, device=dev) if want_matched else None
    torch.ops.torcheval_amd_detection.map_match(
        pred_boxes.contiguous(), pred_scores.contiguous(), pred_labels.contiguous(), target_boxes.contiguous(),
        target_labels.contiguous(), offsets, thresholds, max_detections, scores, labels, hits, gt_count, matched, err)
    return scores, labels, hits, gt_count, matched


def map_curve(hits: torch.Tensor, class_offsets: torch.Tensor, gt_count: torch.Tensor, num_thresholds: int,
              index_50: int = -1, index_75: int = -1):
    """``map_curve``'s two launches: float64 ``AP`` and ``REC`` ``[T, C]`` of the hits in the global
    order ``(label, score descending, stored order)`` with ``class_offsets`` int64 ``[C + 1]`` and
    float64 ``gt_count`` ``[C]``, and the float32 results ``[4]`` (map, map_50, map_75, mar),
    ``map_per_class`` ``[C]`` and ``mar_per_class`` ``[C]``."""
    dev = hits.device
    c = gt_count.shape[0]
    ap = torch.empty(num_thresholds, c, dtype=torch.float64, device=dev)
    rec = torch.empty(num_thresholds, c, dtype=torch.float64, device=dev)
    scalars = torch.empty(4, dtype=torch.float32, device=dev)
    map_c = torch.empty(c, dtype=torch.float32, device=dev)
    mar_c = torch.empty(c, dtype=torch.float32, device=dev)
    torch.ops.torcheval_amd_detection.map_curve(hits, class_offsets, gt_count, index_50, index_75, ap, rec, scalars,
                                                map_c, mar_c)
    return ap, rec, scalars, map_c, mar_c
