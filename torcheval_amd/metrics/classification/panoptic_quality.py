"""Panoptic quality, class API.

Not in the reference tree (docs/parity.md, "Not in the reference").  The states are four float64 ``[K]``
vectors with merge kind ``"sum"`` (the sum of the matched IoUs and the numbers of true positives, false
positives and false negatives, per class), so they live in the contiguous state buffer and sync
through the existing plans.  A ROCm update is K28's three launches (csrc/kernels/panoptic.hip): the
finish launch adds the batch's per-image partials, in image order, straight into the states, with no
host synchronisation.  ``compute()`` on ROCm is one single-wave launch and one read of the flag word.
"""

from typing import Collection, Iterable, Optional

import torch

from torcheval_amd.metrics.functional.classification.panoptic_quality import (
    _class_table,
    _panoptic_classes,
    _panoptic_input_check,
    _panoptic_update,
    _panoptic_value,
    _raise_on_flags,
)
from torcheval_amd.metrics.metric import Metric, inference_update
from torcheval_amd.ops import panoptic as _k28
from torcheval_amd.ops import use_native

__all__ = ["PanopticQuality"]

_STATES = ("iou_sum", "true_positives", "false_positives", "false_negatives")


class PanopticQuality(Metric[torch.Tensor]):
    """Panoptic quality over all images seen; see ``panoptic_quality`` for the definition.  Segments
    are matched per image, and the four per-class sums add over the images.

    On ROCm an unknown ``input`` category without ``allow_unknown_preds_category`` does not stop
    ``update()``: it is taken as void, a device flag is set, and ``compute()`` raises ``ValueError``
    once (and clears the flag).  An image above the kernel's capacities (docs/parity.md) or with a thing
    instance id outside ``[0, 2^32)`` makes ``compute()`` raise ``RuntimeError``.  On CPU ``update()``
    raises on an unknown category and has no limits.

    Args:
        things: the category ids with instances.
        stuffs: the category ids without; disjoint from ``things``.
        allow_unknown_preds_category: an unknown category in ``input`` is void.
        return_sq_and_rq: ``compute()`` returns ``(PQ, SQ, RQ)`` along a last axis of 3.
        return_per_class: ``compute()`` returns the ``[K]`` per-class values and not their mean.
        device: where the states live.
    """

    _err: Optional[torch.Tensor] = None
    _err_words = 1

    def __init__(
        self,
        *,
        things: Collection[int],
        stuffs: Collection[int],
        allow_unknown_preds_category: bool = False,
        return_sq_and_rq: bool = False,
        return_per_class: bool = False,
        device: Optional[torch.device] = None,
    ) -> None:
        super().__init__(device=device)
        self._classes = _panoptic_classes(things, stuffs)
        self.things, self.stuffs = tuple(sorted(set(things))), tuple(sorted(set(stuffs)))
        self.allow_unknown_preds_category = bool(allow_unknown_preds_category)
        self.return_sq_and_rq = bool(return_sq_and_rq)
        self.return_per_class = bool(return_per_class)
        for name in _STATES:
            self._add_state(name, torch.zeros(len(self._classes[0]), dtype=torch.float64, device=self.device),
                            merge="sum")
        if self.device.type == "cuda":
            self._err = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _check_device_errors(self) -> None:
        _raise_on_flags(self._err)

    def _states(self):
        return tuple(getattr(self, name) for name in _STATES)

    @inference_update
    def update(self, input: torch.Tensor, target: torch.Tensor):
        """Add the images of one batch: two integer ``[N, *spatial, 2]`` maps of
        ``(category_id, instance_id)``."""
        _panoptic_input_check(input, target)
        if input.numel() == 0:
            return self
        table = _class_table(self._classes, input.device)
        if input.device == self.iou_sum.device and _k28.supported(input, target, table.shape[1]):
            if self._err is None or self._err.device != input.device:
                self._err = torch.zeros(1, dtype=torch.int32, device=input.device)
            _k28.panoptic_quality(input, target, table, self.allow_unknown_preds_category, self._err, self._states(),
                                  True)
            return self
        for state, batch in zip(self._states(), _panoptic_update(input, target, table,
                                                                 self.allow_unknown_preds_category)):
            state += batch.to(self.device)
        return self

    @torch.inference_mode()
    def compute(self) -> torch.Tensor:
        """PQ over all images seen, float32: a scalar, ``[3]`` with SQ and RQ, ``[K]`` or ``[K, 3]``
        per class; NaN before any update."""
        if use_native(self.iou_sum):
            values = _k28.panoptic_value(self._states(), self.return_per_class)
        else:
            values = _panoptic_value(*self._states(), self.return_per_class)
        self._check_device_errors()
        return values if self.return_sq_and_rq else values[..., 0]

    @torch.inference_mode()
    def merge_state(self, metrics: Iterable["PanopticQuality"]):
        for metric in metrics:
            for mine, theirs in zip(self._states(), metric._states()):
                mine += theirs.to(self.device)
        return self
