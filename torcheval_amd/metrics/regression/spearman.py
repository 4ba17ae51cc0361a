"""Spearman rank correlation, class API.

Not in the reference tree (docs/parity.md, "Not in the reference").  Ranks are a property of the
whole sample, so the samples are kept on device as list states (``merge="cat"``, appended as they
are; the distributed toolkit all-gathers them without pickling) and ``compute()`` is the
functional on their concatenation: on ROCm one K3a sort of both operands and K14
(csrc/kernels/rankcorr.hip).
"""

from typing import Optional

import torch

from torcheval_amd.metrics.classification._sample_store import SampleStoreMetric
from torcheval_amd.metrics.functional.regression.spearman import (
    _spearman_compute,
    _spearman_param_check,
    _spearman_update_input_check,
)

__all__ = ["SpearmanCorrCoef"]


class SpearmanCorrCoef(SampleStoreMetric[torch.Tensor]):
    """Spearman's rho of all samples seen, per task; see ``spearman_corrcoef`` for the definition.

    Args:
        num_tasks: number of independent tasks; updates are ``[n]`` for one task, else
            ``[num_tasks, n]``.
        device: where the samples are kept.
    """

    _cat_dim = -1

    def __init__(self, *, num_tasks: int = 1, device: Optional[torch.device] = None) -> None:
        super().__init__(device=device)
        _spearman_param_check(num_tasks)
        self.num_tasks = num_tasks

    def _check(self, input: torch.Tensor, target: torch.Tensor) -> None:
        _spearman_update_input_check(input, target, self.num_tasks)

    @torch.inference_mode()
    def compute(self) -> torch.Tensor:
        """rho as float32 (float64 for float64 samples): a scalar for one task, else
        ``[num_tasks]``; NaN before any update."""
        if not self.inputs:
            shape = () if self.num_tasks == 1 else (self.num_tasks,)
            return torch.full(shape, torch.nan, dtype=torch.float32, device=self.device)
        return _spearman_compute(*self._cat())
