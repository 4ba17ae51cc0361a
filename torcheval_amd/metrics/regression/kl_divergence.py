"""KL divergence between two score tensors, class API.

Not in the reference tree (docs/parity.md, "Not in the reference").  The states are two float64
scalars, the sum of the counted rows' values and their number, with merge kind ``"sum"``, so they
live in the contiguous state buffer and sync through the existing plans.  A ROCm update is K18's
two launches (csrc/kernels/kl_divergence.hip): the row launch writes one FP64 ``(sum, count)``
partial per block and the finish launch adds them, in block order, straight into the states, with
no host synchronisation and no ATen op (a mask that is not contiguous is copied first).
``compute()`` is ATen on the two scalars.
"""

from typing import Iterable, Optional

import torch

from torcheval_amd.metrics.functional.regression.kl_divergence import _kl_input_check, _kl_rows, _kl_sums
from torcheval_amd.metrics.metric import Metric, inference_update
from torcheval_amd.ops import kl_divergence as _k18

__all__ = ["KLDivergence"]


class KLDivergence(Metric[torch.Tensor]):
    """Mean KL divergence ``KL(P || Q)`` over all counted rows seen, ``P`` from ``target`` and
    ``Q`` from ``input``; see ``kl_divergence`` for the definition.  There is no error flag: a NaN
    or ``inf`` row keeps the value NaN or ``inf`` until ``reset()``.

    Args:
        from_logits: the operands are logits (or log-probabilities); ``False``: non-negative
            weights, normalised by their row sums.
        device: where the states live.
    """

    def __init__(self, *, from_logits: bool = True, device: Optional[torch.device] = None) -> None:
        super().__init__(device=device)
        self.from_logits = from_logits
        self._add_state("kl_sum", torch.tensor(0.0, dtype=torch.float64, device=self.device), merge="sum")
        self._add_state("num_rows", torch.tensor(0.0, dtype=torch.float64, device=self.device), merge="sum")

    @inference_update
    def update(self, input: torch.Tensor, target: torch.Tensor, *,
               mask: Optional[torch.Tensor] = None) -> "KLDivergence":
        """Add the rows of one ``[..., C]`` pair of score tensors; rows whose ``mask`` (bool
        ``[...]``) is ``False`` are not read and not counted.  Without a counted row the states
        stay as they are."""
        _kl_input_check(input, target, mask)
        if input.numel() == 0:
            return self
        if input.device == self.kl_sum.device and _k18.supported(input, target, mask):
            _k18.kl_update(input, target, mask, self.from_logits, self.kl_sum, self.num_rows)
            return self
        total, count = _kl_sums(_kl_rows(input, target, self.from_logits, mask), mask)
        self.kl_sum += total.to(self.device)
        self.num_rows += count.to(self.device)
        return self

    @torch.inference_mode()
    def compute(self) -> torch.Tensor:
        """The mean row value as a float32 scalar; NaN before any counted row."""
        return (self.kl_sum / self.num_rows).float()

    @torch.inference_mode()
    def merge_state(self, metrics: Iterable["KLDivergence"]) -> "KLDivergence":
        for metric in metrics:
            self.kl_sum += metric.kl_sum.to(self.device)
            self.num_rows += metric.num_rows.to(self.device)
        return self
