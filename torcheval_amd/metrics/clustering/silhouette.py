"""Silhouette coefficient, class API.

Not in the reference tree (docs/parity.md, "Not in the reference").  The score is a statistic of all
pairwise distances of the samples seen, so the features and their labels are kept on device as two
list states (``merge="cat"``, appended as they are; the distributed toolkit all-gathers them without
pickling) and ``compute()`` is the functional on their concatenation: on ROCm K23
(csrc/kernels/silhouette.hip).
"""

from typing import Iterable, Optional

import torch
from torch import Tensor

from torcheval_amd.metrics.functional.clustering.silhouette import (
    _silhouette_checked,
    _silhouette_input_check,
    _silhouette_param_check,
)
from torcheval_amd.metrics.metric import Metric, inference_update

__all__ = ["SilhouetteScore"]


class SilhouetteScore(Metric[Tensor]):
    """Mean silhouette coefficient of all samples seen; see ``silhouette_score`` for the definition
    and for degenerate inputs.

    Args:
        num_clusters: the labels lie in ``[0, num_clusters)``.  ``None`` reads the largest label on
            the host at ``compute()``, which then is the call's only host synchronisation.
        device: where the features and labels are kept.
    """

    def __init__(self, num_clusters: Optional[int] = None, device: Optional[torch.device] = None) -> None:
        super().__init__(device=device)
        _silhouette_param_check(num_clusters)
        self.num_clusters = num_clusters
        self._add_state("features", [], merge="cat")
        self._add_state("labels", [], merge="cat")

    @inference_update
    def update(self, input: Tensor, labels: Tensor):
        """Add a batch of ``[B, D]`` features and their ``[B]`` int64 / int32 cluster ids."""
        _silhouette_input_check(input, labels)
        if self.features and (input.shape[1] != self.features[0].shape[1] or input.dtype != self.features[0].dtype):
            raise ValueError(
                f"Expected [B, {self.features[0].shape[1]}] features of dtype {self.features[0].dtype}, "
                f"got shape {tuple(input.shape)} and dtype {input.dtype}."
            )
        self.features.append(input.to(self.device))
        self.labels.append(labels.to(self.device, torch.int64))
        return self

    @torch.inference_mode()
    def merge_state(self, metrics: Iterable["SilhouetteScore"]):
        for metric in metrics:
            self.features.extend(t.to(self.device) for t in metric.features)
            self.labels.extend(t.to(self.device) for t in metric.labels)
        return self

    @torch.inference_mode()
    def _prepare_for_merge_state(self) -> None:
        if self.features:
            self.features = [torch.cat(self.features)]
            self.labels = [torch.cat(self.labels)]

    @torch.inference_mode()
    def compute(self) -> Tensor:
        """The score as a float32 scalar (float64 for float64 features) on the metric's device; NaN
        before any update and while fewer than two clusters have a member."""
        if not self.features:
            return torch.full((), torch.nan, device=self.device)
        input, labels = torch.cat(self.features), torch.cat(self.labels)
        out = _silhouette_checked(input, labels, self.num_clusters)
        return out["score64"][0] if input.dtype == torch.float64 else out["score"][0]
