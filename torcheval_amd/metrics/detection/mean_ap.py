"""COCO-style detection mean average precision, class API.

Not in the reference tree (docs/parity.md, "Not in the reference").  Matching depends on one image
only, so it runs inside ``update()`` (on ROCm K24's ``map_match``, one launch) and no box is kept:
the states are 12 bytes per detection in three list states (``merge="cat"``: score, label, a bit mask
of the IoU thresholds the detection hit; the distributed toolkit all-gathers them without pickling)
and the float64 ``[num_classes]`` count of ground truths (``merge="sum"``; integers, exact below
2^53).  ``compute()`` orders the stored detections and builds the curves (K24's ``map_curve``).
"""

from typing import Dict, Iterable, List, Optional, Sequence

import torch
from torch import Tensor

from torcheval_amd.metrics.functional.detection.mean_ap import (
    Counts,
    _map_input_check,
    _map_match,
    _map_param_check,
    _map_value,
    _raise_on_bad_input,
)
from torcheval_amd.metrics.metric import Metric, inference_update

__all__ = ["MeanAveragePrecision"]

_LISTS = ("det_scores", "det_labels", "det_hits")


def _field(items: Sequence[Dict[str, Tensor]], name: str, which: str) -> Tensor:
    for item in items:
        if not isinstance(item, dict) or name not in item:
            raise ValueError(f"Every entry of `{which}` should be a dict with the key {name!r}.")
    return torch.cat([item[name] for item in items])


class MeanAveragePrecision(Metric[Dict[str, Tensor]]):
    """COCO mean average precision of all images seen; see ``mean_average_precision`` for the
    definition and the results.

    On ROCm a bad detection or ground truth (a NaN score, a non-finite coordinate, ``x2 < x1`` or
    ``y2 < y1``, a label outside ``[0, num_classes)``) does not stop ``update()``: it is counted
    nowhere, a device flag is set, and ``compute()`` raises once (and clears the flag).  On CPU
    ``update()`` raises and leaves the states untouched.

    Args:
        num_classes: the labels lie in ``[0, num_classes)``.
        iou_thresholds: 1 to 16 values in ``(0, 1]``; default ``numpy.linspace(0.5, 0.95, 10)``.
        max_detections: detections kept per image and class.
        device: where the states live.
    """

    _err: Optional[Tensor] = None
    _err_words = 1

    def __init__(self, num_classes: int, *, iou_thresholds: Optional[Sequence[float]] = None,
                 max_detections: int = 100, device: Optional[torch.device] = None) -> None:
        super().__init__(device=device)
        self.iou_thresholds = _map_param_check(num_classes, iou_thresholds, max_detections)
        self.num_classes = num_classes
        self.max_detections = max_detections
        for name in _LISTS:
            self._add_state(name, [], merge="cat")
        self._add_state("gt_count", torch.zeros(num_classes, dtype=torch.float64, device=self.device), merge="sum")
        if self.device.type == "cuda":
            self._err = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _err_for(self, input: Tensor) -> Optional[Tensor]:
        if not input.is_cuda:
            return None
        if self._err is None or self._err.device != input.device:
            self._err = torch.zeros(1, dtype=torch.int32, device=input.device)
        return self._err

    def _check_device_errors(self) -> None:
        _raise_on_bad_input(self._err)

    @inference_update
    def update(self, preds: Sequence[Dict[str, Tensor]], targets: Sequence[Dict[str, Tensor]]):
        """Add a batch of images: ``preds[i]`` holds ``boxes`` ``[n_i, 4]``, ``scores`` ``[n_i]`` and
        ``labels`` ``[n_i]``, ``targets[i]`` holds ``boxes`` ``[g_i, 4]`` and ``labels`` ``[g_i]`` (the
        lists of dicts of torchmetrics).  Packed with one ``torch.cat`` per field; the counts are
        shapes, so no value is read from the device."""
        if len(preds) != len(targets):
            raise ValueError(f"`preds` and `targets` should list the same images, got {len(preds)} and {len(targets)}.")
        if len(preds) == 0:
            return self
        return self.update_packed(
            _field(preds, "boxes", "preds"), _field(preds, "scores", "preds"), _field(preds, "labels", "preds"),
            [int(p["boxes"].shape[0]) for p in preds],
            _field(targets, "boxes", "targets"), _field(targets, "labels", "targets"),
            [int(t["boxes"].shape[0]) for t in targets])

    @inference_update
    def update_packed(self, pred_boxes: Tensor, pred_scores: Tensor, pred_labels: Tensor, pred_counts: Counts,
                      target_boxes: Tensor, target_labels: Tensor, target_counts: Counts):
        """Add a batch of images in the packed layout of ``mean_average_precision``."""
        pc, tc = _map_input_check(pred_boxes, pred_scores, pred_labels, pred_counts, target_boxes, target_labels,
                                  target_counts)
        scores, labels, hits, gt_count, _ = _map_match(
            pred_boxes, pred_scores, pred_labels, pc, target_boxes, target_labels, tc, self.num_classes,
            self.iou_thresholds, self.max_detections, self._err_for(pred_boxes))
        if scores.shape[0]:
            self.det_scores.append(scores.to(self.device))
            self.det_labels.append(labels.to(self.device))
            self.det_hits.append(hits.to(self.device))
        self.gt_count += gt_count.to(self.device)
        return self

    def _stored(self) -> List[Tensor]:
        if self.det_scores:
            return [torch.cat(getattr(self, name)) for name in _LISTS]
        return [torch.empty(0, dtype=dtype, device=self.device)
                for dtype in (torch.float32, torch.int32, torch.int32)]

    @torch.inference_mode()
    def compute(self) -> Dict[str, Tensor]:
        """The dict of float32 results on the metric's device; NaN everywhere while no class has a
        ground truth."""
        scores, labels, hits = self._stored()
        out = _map_value(scores, labels, hits, self.gt_count, self.iou_thresholds)
        self._check_device_errors()
        return out

    @torch.inference_mode()
    def merge_state(self, metrics: Iterable["MeanAveragePrecision"]):
        for metric in metrics:
            for name in _LISTS:
                getattr(self, name).extend(t.to(self.device) for t in getattr(metric, name))
            self.gt_count += metric.gt_count.to(self.device)
        return self

    @torch.inference_mode()
    def _prepare_for_merge_state(self) -> None:
        if self.det_scores:
            for name in _LISTS:
                setattr(self, name, [torch.cat(getattr(self, name))])
