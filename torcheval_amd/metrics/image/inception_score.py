"""Inception Score, class API.

Not in the reference tree (docs/parity.md, "Not in the reference").  The states are three float64
tensors with merge kind ``"sum"``: per split the column sums of the rows' softmax probabilities
``[S, C]``, the sum of the rows' negative entropies ``[S]`` and the number of rows ``[S]``.  They
live in the contiguous state buffer and sync through the existing plans; nothing of size ``N`` is
kept.  A ROCm update is K21's two launches (csrc/kernels/inception_score.hip) straight into the
states and ``compute()`` is its value launch, with no host synchronisation.
"""

from typing import Iterable, Optional, Tuple

import torch
from torch import nn, Tensor

from torcheval_amd.metrics.functional.image.inception_score import (
    _inception_score_values,
    _is_input_check,
    _is_param_check,
    _stats_add,
)
from torcheval_amd.metrics.metric import Metric, inference_update

__all__ = ["InceptionScore"]


class InceptionScore(Metric[Tuple[Tensor, Tensor]]):
    """Inception Score of generated images: ``(mean, std)`` over the splits; see
    ``inception_score`` for the definition.

    A row belongs to split ``(first + i) mod splits``, ``i`` its position in the call and ``first``
    the number of rows this object has seen since construction or ``reset()``, so several updates
    partition like one call on their concatenation.  ``first`` is a host integer, not a state:
    ``state_dict``, ``load_state_dict`` and ``merge_state`` leave it as it is.

    Args:
        model: classifier mapping images to ``[B, num_classes]`` logits; default the native
            Inception-v3 with its 1000-way layer (``InceptionV3Logits``).
        num_classes: width of the logits (1000 for the default model).
        splits: number of splits, ``>= 1``.
        device: where the states live.
    """

    def __init__(
        self,
        model: Optional[nn.Module] = None,
        num_classes: int = 1000,
        splits: int = 10,
        device: Optional[torch.device] = None,
    ) -> None:
        super().__init__(device=device)
        _is_param_check(splits)
        if not isinstance(num_classes, int) or isinstance(num_classes, bool) or num_classes < 1:
            raise ValueError(f"`num_classes` should be a positive integer, but received {num_classes}.")
        if model is None:
            if num_classes != 1000:
                raise ValueError("When the default Inception v3 model is used, num_classes needs to be set to 1000")
            from torcheval_amd.models.inception import InceptionV3Logits

            model = InceptionV3Logits()
        self.model = model.to(self.device)
        self.model.eval()
        self.num_classes = num_classes
        self.splits = splits
        self._rows_seen = 0  # mod splits: the split of the next row
        kw = dict(dtype=torch.float64, device=self.device)
        self._add_state("prob_sum", torch.zeros(splits, num_classes, **kw), merge="sum")
        self._add_state("neg_entropy_sum", torch.zeros(splits, **kw), merge="sum")
        self._add_state("num_rows", torch.zeros(splits, **kw), merge="sum")

    @inference_update
    def update(self, images: Tensor) -> "InceptionScore":
        """Add a batch of [B, 3, H, W] images (float32 in [0, 1] for the default model)."""
        from torcheval_amd.metrics.image.fid import FrechetInceptionDistance

        FrechetInceptionDistance._FID_update_input_check(self, images=images, is_real=True)
        return self.update_logits(self.model(images.to(self.device)))

    @inference_update
    def update_logits(self, logits: Tensor) -> "InceptionScore":
        """Add precomputed ``[B, num_classes]`` logits (skips the classifier).  No rows: a no-op."""
        _is_input_check(logits)
        if logits.shape[1] != self.num_classes:
            raise ValueError(f"Expected [B, {self.num_classes}] logits, but got shape {tuple(logits.shape)}.")
        n = logits.shape[0]
        if n == 0:
            return self
        if logits.device != self.prob_sum.device:
            logits = logits.to(self.prob_sum.device)
        _stats_add(logits, self._rows_seen, self.prob_sum, self.neg_entropy_sum, self.num_rows)
        self._rows_seen = (self._rows_seen + n) % self.splits
        return self

    @torch.inference_mode()
    def compute(self) -> Tuple[Tensor, Tensor]:
        """``(mean, std)`` as float32 scalars on the metric's device; NaN before any row."""
        _, mean, std = _inception_score_values(self.prob_sum, self.neg_entropy_sum, self.num_rows)
        return mean, std

    @torch.inference_mode()
    def merge_state(self, metrics: Iterable["InceptionScore"]) -> "InceptionScore":
        for metric in metrics:
            self.prob_sum += metric.prob_sum.to(self.device)
            self.neg_entropy_sum += metric.neg_entropy_sum.to(self.device)
            self.num_rows += metric.num_rows.to(self.device)
        return self

    def reset(self) -> "InceptionScore":
        super().reset()
        self._rows_seen = 0
        return self

    def to(self, device, *args, **kwargs) -> "InceptionScore":
        super().to(device, *args, **kwargs)
        self.model.to(self.device)
        return self
