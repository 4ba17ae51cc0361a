"""Improved precision / recall and density / coverage, class API.

Not in the reference tree (docs/parity.md, "Not in the reference").  Both are k-nearest-neighbour
statistics of all features seen, so the features are kept on device as two list states
(``merge="cat"``, appended as they are; the distributed toolkit all-gathers them without pickling,
and the feature extractor is never transferred) and ``compute()`` is the functional on their
concatenation: on ROCm K22 (csrc/kernels/prdc.hip).  The two metrics differ in their default ``k``
and in which two of the four values they return, so they share one base class.
"""

from typing import Iterable, Optional, Tuple

import torch
from torch import nn, Tensor

from torcheval_amd.metrics.functional.image.prdc import _prdc, _prdc_input_check, _prdc_param_check
from torcheval_amd.metrics.metric import Metric, inference_update

__all__ = ["DensityCoverage", "ImprovedPrecisionRecall"]


class _NeighbourMetric(Metric[Tuple[Tensor, Tensor]]):
    """Feature lists of real and generated images, and two of the four values of ``_prdc``."""

    _VALUES: Tuple[int, int] = (0, 1)  # positions in ``values``: precision, recall, density, coverage

    def __init__(
        self,
        model: Optional[nn.Module],
        feature_dim: int,
        k: int,
        device: Optional[torch.device],
    ) -> None:
        super().__init__(device=device)
        from torcheval_amd.metrics.image.fid import FrechetInceptionDistance
        from torcheval_amd.models.inception import FIDInceptionV3

        FrechetInceptionDistance._FID_parameter_check(self, model=model, feature_dim=feature_dim)
        _prdc_param_check(k)
        if model is None:
            model = FIDInceptionV3()
        self.model = model.to(self.device)
        self.model.eval()
        self._feature_dim = feature_dim
        self.k = k
        self._add_state("real_features", [], merge="cat")
        self._add_state("fake_features", [], merge="cat")

    @inference_update
    def update(self, images: Tensor, is_real: bool):
        """Add a batch of [B, 3, H, W] images (float32 in [0, 1] for the default model)."""
        from torcheval_amd.metrics.image.fid import FrechetInceptionDistance

        FrechetInceptionDistance._FID_update_input_check(self, images=images, is_real=is_real)
        return self.update_activations(self.model(images.to(self.device)), is_real)

    @torch.inference_mode()
    def update_activations(self, activations: Tensor, is_real: bool):
        """Add precomputed [B, feature_dim] activations (skips the feature extractor)."""
        if type(is_real) != bool:
            raise ValueError(f"Expected 'real' to be of type bool but got {type(is_real)}.")
        if activations.dim() != 2 or activations.shape[1] != self._feature_dim:
            raise ValueError(
                f"Expected [B, {self._feature_dim}] activations, but got shape {tuple(activations.shape)}."
            )
        (self.real_features if is_real else self.fake_features).append(activations.to(self.device))
        return self

    @torch.inference_mode()
    def merge_state(self, metrics: Iterable["_NeighbourMetric"]):
        for metric in metrics:
            self.real_features.extend(t.to(self.device) for t in metric.real_features)
            self.fake_features.extend(t.to(self.device) for t in metric.fake_features)
        return self

    @torch.inference_mode()
    def _prepare_for_merge_state(self) -> None:
        if self.real_features:
            self.real_features = [torch.cat(self.real_features)]
        if self.fake_features:
            self.fake_features = [torch.cat(self.fake_features)]

    @torch.inference_mode()
    def compute(self) -> Tuple[Tensor, Tensor]:
        """The metric's two values as float32 scalars on its device; ``ValueError`` while either
        side holds fewer than ``k + 1`` rows."""
        empty = torch.empty(0, self._feature_dim, device=self.device)
        real = torch.cat(self.real_features) if self.real_features else empty
        fake = torch.cat(self.fake_features) if self.fake_features else empty
        _prdc_input_check(real, fake, self.k)
        values = _prdc(real, fake, self.k)["values"]
        return values[self._VALUES[0]], values[self._VALUES[1]]

    def to(self, device, *args, **kwargs):
        super().to(device, *args, **kwargs)
        self.model.to(self.device)
        return self


class ImprovedPrecisionRecall(_NeighbourMetric):
    """Improved precision and recall between real and generated images: ``(precision, recall)``;
    see ``improved_precision_recall`` for the definition.

    Args:
        model: feature extractor mapping images to ``[B, feature_dim]`` activations; default the
            native Inception-v3 (``FIDInceptionV3``, as ``FrechetInceptionDistance``).
        feature_dim: activation width (2048 for the default model).
        k: the neighbour that sets a row's radius.
        device: where the features are kept.
    """

    _VALUES = (0, 1)

    def __init__(
        self,
        model: Optional[nn.Module] = None,
        feature_dim: int = 2048,
        k: int = 3,
        device: Optional[torch.device] = None,
    ) -> None:
        super().__init__(model, feature_dim, k, device)


class DensityCoverage(_NeighbourMetric):
    """Density and coverage between real and generated images: ``(density, coverage)``; see
    ``density_coverage`` for the definition.

    Args:
        model, feature_dim, device: as ``ImprovedPrecisionRecall``.
        k: the neighbour that sets a real row's radius.
    """

    _VALUES = (2, 3)

    def __init__(
        self,
        model: Optional[nn.Module] = None,
        feature_dim: int = 2048,
        k: int = 5,
        device: Optional[torch.device] = None,
    ) -> None:
        super().__init__(model, feature_dim, k, device)
