"""Kendall rank correlation (tau-b / tau-c), class API.

Not in the reference tree (docs/parity.md, "Not in the reference").  The statistic is a property of
the whole sample, so the samples are kept on device as list states (``merge="cat"``, appended as
they are; the distributed toolkit all-gathers them without pickling) and ``compute()`` is the
functional on their concatenation: on ROCm two K3a sorts and K19 (csrc/kernels/kendall.hip).
"""

from typing import Optional

import torch

from torcheval_amd.metrics.classification._sample_store import SampleStoreMetric
from torcheval_amd.metrics.functional.regression.kendall import (
    _kendall_compute,
    _kendall_param_check,
    _kendall_update_input_check,
)

__all__ = ["KendallRankCorrCoef"]


class KendallRankCorrCoef(SampleStoreMetric[torch.Tensor]):
    """Kendall's tau of all samples seen, per task; see ``kendall_rank_corrcoef`` for the definition.

    Args:
        num_tasks: number of independent tasks; updates are ``[n]`` for one task, else
            ``[num_tasks, n]``.
        variant: ``"b"`` or ``"c"``.
        device: where the samples are kept.
    """

    _cat_dim = -1

    def __init__(self, *, num_tasks: int = 1, variant: str = "b", device: Optional[torch.device] = None) -> None:
        super().__init__(device=device)
        _kendall_param_check(num_tasks, variant)
        self.num_tasks = num_tasks
        self.variant = variant

    def _check(self, input: torch.Tensor, target: torch.Tensor) -> None:
        _kendall_update_input_check(input, target, self.num_tasks)

    @torch.inference_mode()
    def compute(self) -> torch.Tensor:
        """tau as float32 (float64 for float64 samples): a scalar for one task, else
        ``[num_tasks]``; NaN before any update."""
        if not self.inputs:
            shape = () if self.num_tasks == 1 else (self.num_tasks,)
            return torch.full(shape, torch.nan, dtype=torch.float32, device=self.device)
        return _kendall_compute(*self._cat(), self.variant)
