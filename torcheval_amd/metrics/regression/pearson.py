"""Pearson and Lin's concordance correlation, class API.

Not in the reference tree (docs/parity.md, "Not in the reference").  The state is one float64
``[6, num_tasks]`` tensor of moments (``n, mean_x, mean_y, m2_x, m2_y, c_xy``).  It merges by the
pairwise update, none of sum / max / min / cat, so it is declared with ``merge=None``: the
distributed toolkit gathers it and calls ``merge_state``.  A ROCm update is K16's two launches
(csrc/kernels/corrcoef.hip) with no host synchronisation and no ATen op; ``merge_state`` and
``compute()`` on ROCm are one launch each.
"""

from typing import Iterable, Optional

import torch

from torcheval_amd.metrics.functional.regression.pearson import (
    _batch_moments,
    _moments_merge,
    _moments_value,
    _pearson_param_check,
    _pearson_update_input_check,
)
from torcheval_amd.metrics.metric import Metric, inference_update
from torcheval_amd.ops import corrcoef as _k16
from torcheval_amd.ops import use_native

__all__ = ["PearsonCorrCoef", "ConcordanceCorrCoef"]


class PearsonCorrCoef(Metric[torch.Tensor]):
    """Pearson's r of all samples seen, per task; see ``pearson_corrcoef`` for the definition.  A
    NaN or an infinity in a task keeps that task NaN until ``reset()``.

    Args:
        num_tasks: number of independent tasks; updates are ``[n]`` for one task, else
            ``[num_tasks, n]``.
        device: where the state lives.
    """

    _kind = "pearson"

    def __init__(self, *, num_tasks: int = 1, device: Optional[torch.device] = None) -> None:
        super().__init__(device=device)
        _pearson_param_check(num_tasks)
        self.num_tasks = num_tasks
        self._add_state("moments", torch.zeros(6, num_tasks, dtype=torch.float64, device=self.device), merge=None)

    def _merge(self, other: torch.Tensor) -> None:
        other = other.to(self.moments.device)
        if use_native(self.moments):
            _k16.corrcoef_merge(self.moments, other.contiguous())
        else:
            self.moments.copy_(_moments_merge(self.moments, other))

    @inference_update
    def update(self, input: torch.Tensor, target: torch.Tensor) -> "PearsonCorrCoef":
        """Merge one batch of samples, ``[n]`` or ``[num_tasks, n]``, into the state."""
        _pearson_update_input_check(input, target, self.num_tasks)
        if input.shape[-1] == 0:
            return self
        if input.device == self.moments.device and _k16.supported(input, target):
            _k16.corrcoef_update(input, target, self.moments)
        else:
            self._merge(_batch_moments(input, target))
        return self

    @torch.inference_mode()
    def compute(self) -> torch.Tensor:
        """The value as float32: a scalar for one task, else ``[num_tasks]``; NaN before any
        update."""
        if use_native(self.moments):
            out = _k16.corrcoef_value(self.moments, self._kind)
        else:
            out = _moments_value(self.moments, self._kind).float()
        return out[0] if self.num_tasks == 1 else out

    @torch.inference_mode()
    def merge_state(self, metrics: Iterable["PearsonCorrCoef"]) -> "PearsonCorrCoef":
        for metric in metrics:
            self._merge(metric.moments)
        return self


class ConcordanceCorrCoef(PearsonCorrCoef):
    """Lin's concordance correlation of all samples seen, per task; see ``concordance_corrcoef``.
    The state and its updates are ``PearsonCorrCoef``'s; only the value formula differs."""

    _kind = "concordance"
