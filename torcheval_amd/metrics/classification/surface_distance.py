"""Hausdorff distance and average surface distance of segmentations, class API.

Not in the reference tree (docs/parity.md, "Not in the reference").  The states are three float64
``[K]`` vectors with merge kind ``"sum"`` (the sum of the finite per-image values, their number and the
number of ``+inf`` values, per class), so they live in the contiguous state buffer and sync through
the existing plans.  A ROCm update is K27's launches (csrc/kernels/surface_distance.hip): the combine
launch adds the batch's values straight into the states, with no host synchronisation.
"""

from typing import Iterable, Optional, Sequence

import torch

from torcheval_amd.metrics.functional.classification.surface_distance import (
    _surface_average_check,
    _surface_batch,
    _surface_input_check,
    _surface_param_check,
)
from torcheval_amd.metrics.metric import Metric, inference_update

__all__ = ["AverageSurfaceDistance", "HausdorffDistance"]

_STATES = ("distance_sum", "num_finite", "num_inf")


class _SurfaceMetric(Metric[torch.Tensor]):
    _mode = 0
    _quantile = -1.0
    _both = True

    def __init__(self, num_classes: int, include_background: bool, spacing: Optional[Sequence[float]],
                 average: Optional[str], device: Optional[torch.device]) -> None:
        super().__init__(device=device)
        _surface_param_check(num_classes, include_background, spacing)
        self.average = _surface_average_check(average)
        self.num_classes = num_classes
        self.include_background = include_background
        self.spacing = spacing
        classes = num_classes - (0 if include_background else 1)
        for name in _STATES:
            self._add_state(name, torch.zeros(classes, dtype=torch.float64, device=self.device), merge="sum")

    @inference_update
    def update(self, input: torch.Tensor, target: torch.Tensor):
        """Add the images of one batch: labels ``[N, H, W]`` or scores ``[N, C, H, W]``, and the
        labels ``[N, H, W]``."""
        _surface_input_check(input, target, self.num_classes)
        _surface_batch(input, target, self.num_classes, self.include_background, self._mode, self._quantile,
                       self._both, self.spacing, (self.distance_sum, self.num_finite, self.num_inf))
        return self

    @torch.inference_mode()
    def compute(self) -> torch.Tensor:
        """Per class the mean of the finite per-image values seen, float32: ``[K]`` for
        ``average="none"``, or the mean over the classes that have a value; NaN where there is none."""
        per_class = self.distance_sum / self.num_finite  # 0 / 0: no finite value
        if _surface_average_check(self.average) == "none":
            return per_class.float()
        has = self.num_finite > 0
        return (torch.where(has, per_class, 0.0).sum() / has.sum()).float()

    @torch.inference_mode()
    def merge_state(self, metrics: Iterable["_SurfaceMetric"]):
        for metric in metrics:
            for name in _STATES:
                getattr(self, name).add_(getattr(metric, name).to(self.device))
        return self


class HausdorffDistance(_SurfaceMetric):
    """Mean over the images seen of the per-image Hausdorff distance of each class; see
    ``hausdorff_distance`` for the definition.  An image whose value is ``+inf`` (the class is absent
    from exactly one map) or NaN (from both) is left out of the mean; ``num_inf`` counts the former.

    Args:
        num_classes: number of classes.
        include_background: whether class 0 gets a value.
        percentile: ``None`` for the maximum, or a number in ``[0, 100]`` (95: HD95).
        directed: only from the prediction's surface to the target's.
        spacing: the pixel size along ``(H, W)``; ``None`` is ``(1, 1)``.
        average: ``"macro"`` (over the classes that have a value), ``"none"`` or ``None`` (per class).
        device: where the states live.
    """

    def __init__(
        self,
        *,
        num_classes: int,
        include_background: bool = False,
        percentile: Optional[float] = None,
        directed: bool = False,
        spacing: Optional[Sequence[float]] = None,
        average: Optional[str] = "macro",
        device: Optional[torch.device] = None,
    ) -> None:
        super().__init__(num_classes, include_background, spacing, average, device)
        if percentile is not None and (isinstance(percentile, bool) or not isinstance(percentile, (int, float))
                                       or not 0 <= percentile <= 100):
            raise ValueError(f"`percentile` should be None or a number in [0, 100], got {percentile!r}.")
        self.percentile = percentile
        self.directed = directed
        self._quantile = -1.0 if percentile is None else percentile / 100.0
        self._both = not directed


class AverageSurfaceDistance(_SurfaceMetric):
    """Mean over the images seen of the per-image average surface distance of each class; see
    ``average_surface_distance`` for the definition and ``HausdorffDistance`` for the other arguments
    and the handling of ``+inf`` and NaN.

    Args:
        symmetric: both directions over both surfaces (ASSD); otherwise from the prediction only.
    """

    _mode = 1

    def __init__(
        self,
        *,
        num_classes: int,
        include_background: bool = False,
        symmetric: bool = True,
        spacing: Optional[Sequence[float]] = None,
        average: Optional[str] = "macro",
        device: Optional[torch.device] = None,
    ) -> None:
        super().__init__(num_classes, include_background, spacing, average, device)
        self.symmetric = symmetric
        self._both = bool(symmetric)
