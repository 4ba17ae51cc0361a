"""Normalized discounted cumulative gain (NDCG), class API.

Not in the reference tree (docs/parity.md, "Not in the reference").  The states are two float64
scalars with merge kind ``"sum"``, so they live in the contiguous state buffer and sync through
the existing plans.  A ROCm update is K13's two launches (csrc/kernels/ndcg.hip): the row launch
writes one FP64 partial per block and the finish launch adds them, in a fixed order, and the row
count straight into the states, with no host synchronisation and no ATen op.
"""

from typing import Iterable, Optional

import torch

from torcheval_amd.metrics.functional.ranking.ndcg import (
    _ndcg_input_check,
    _ndcg_update,
    _raise_on_bad_relevance,
    _report_bad_rows,
)
from torcheval_amd.metrics.metric import Metric, inference_update
from torcheval_amd.ops import ndcg as _k13

__all__ = ["NormalizedDCG"]


class NormalizedDCG(Metric[torch.Tensor]):
    """Mean NDCG@k over all rows seen; see ``normalized_dcg`` for the definition.

    On ROCm a negative or NaN relevance does not stop ``update()``: its row scores NaN, a device
    flag is set, and ``compute()`` raises (and clears the flag; the states keep the NaN until
    ``reset()``).  On CPU ``update()`` raises and leaves the states untouched.

    Args:
        k: the cutoff; ``None`` ranks all items of a row.
        exponential_gain: use ``2^target - 1`` instead of ``target`` as the gain.
        device: where the states live.
    """

    _err: Optional[torch.Tensor] = None
    _err_words = 1

    def __init__(
        self,
        *,
        k: Optional[int] = None,
        exponential_gain: bool = False,
        device: Optional[torch.device] = None,
    ) -> None:
        super().__init__(device=device)
        if k is not None and k <= 0:
            raise ValueError(f"k should be None or positive, got {k}.")
        self.k = k
        self.exponential_gain = exponential_gain
        self._add_state("ndcg_sum", torch.tensor(0.0, dtype=torch.float64, device=self.device), merge="sum")
        self._add_state("num_rows", torch.tensor(0.0, dtype=torch.float64, device=self.device), merge="sum")
        if self.device.type == "cuda":
            self._err = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _err_for(self, input: torch.Tensor) -> Optional[torch.Tensor]:
        if not input.is_cuda:
            return None
        if self._err is None or self._err.device != input.device:
            self._err = torch.zeros(1, dtype=torch.int32, device=input.device)
        return self._err

    def _check_device_errors(self) -> None:
        _raise_on_bad_relevance(self._err)

    @inference_update
    def update(self, input: torch.Tensor, target: torch.Tensor) -> "NormalizedDCG":
        """Add the rows of one ``[N, C]`` batch of scores and graded relevance."""
        _ndcg_input_check(input, target, self.k)
        n, c = input.shape
        if n == 0:
            return self
        if c == 0:  # no items: every row's value is 0
            self.num_rows += n
            return self
        cutoff = c if self.k is None else min(int(self.k), c)
        if input.device == self.ndcg_sum.device and _k13.supported(input, target):
            _k13.ndcg(input, target, cutoff, self.exponential_gain, None, self.ndcg_sum, self.num_rows,
                      self._err_for(input))
            return self
        values, bad = _ndcg_update(input, target, cutoff, self.exponential_gain)
        _report_bad_rows(bad, self._err_for(input))
        self.ndcg_sum += values.sum().to(self.device)
        self.num_rows += n
        return self

    @torch.inference_mode()
    def compute(self) -> torch.Tensor:
        """The mean NDCG of all rows as float32; NaN before any update."""
        out = (self.ndcg_sum / self.num_rows).float()
        self._check_device_errors()
        return out

    @torch.inference_mode()
    def merge_state(self, metrics: Iterable["NormalizedDCG"]) -> "NormalizedDCG":
        for metric in metrics:
            self.ndcg_sum += metric.ndcg_sum.to(self.device)
            self.num_rows += metric.num_rows.to(self.device)
        return self
