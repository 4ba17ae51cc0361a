"""Kernel Inception Distance, class API.

Not in the reference tree (docs/parity.md, "Not in the reference").  The statistic is a property of
random subsets of all features seen, so the features are kept on device as two list states
(``merge="cat"``, appended as they are; the distributed toolkit all-gathers them without pickling,
and the feature extractor is never transferred) and ``compute()`` is the functional on their
concatenation: on ROCm K20 (csrc/kernels/kid.hip), two launches behind the index draws.
"""

from typing import Iterable, Optional, Tuple

import torch
from torch import nn, Tensor

from torcheval_amd.metrics.functional.image.kid import (
    _kid_compute,
    _kid_input_check,
    _kid_param_check,
)
from torcheval_amd.metrics.metric import Metric, inference_update

__all__ = ["KernelInceptionDistance"]


class KernelInceptionDistance(Metric[Tuple[Tensor, Tensor]]):
    """KID between real and generated images: ``(mean, std)`` of the polynomial-kernel MMD^2 over
    random subsets of the features; see ``kernel_inception_distance`` for the definition.

    Args:
        model: feature extractor mapping images to ``[B, feature_dim]`` activations; default the
            native Inception-v3 (``FIDInceptionV3``, as ``FrechetInceptionDistance``).
        feature_dim: activation width (2048 for the default model).
        subsets, subset_size, degree, gamma, coef: as ``kernel_inception_distance``.
        seed: when set, every ``compute()`` draws its subsets from a fresh generator seeded with
            it, so ``compute()`` is idempotent and equal on all ranks after a sync; when ``None``
            the global RNG is used.
        device: where the features are kept.
    """

    def __init__(
        self,
        model: Optional[nn.Module] = None,
        feature_dim: int = 2048,
        subsets: int = 100,
        subset_size: int = 1000,
        degree: int = 3,
        gamma: Optional[float] = None,
        coef: float = 1.0,
        seed: Optional[int] = None,
        device: Optional[torch.device] = None,
    ) -> None:
        super().__init__(device=device)
        from torcheval_amd.metrics.image.fid import FrechetInceptionDistance
        from torcheval_amd.models.inception import FIDInceptionV3

        FrechetInceptionDistance._FID_parameter_check(self, model=model, feature_dim=feature_dim)
        _kid_param_check(subsets, subset_size, degree)
        if model is None:
            model = FIDInceptionV3()
        self.model = model.to(self.device)
        self.model.eval()
        self._feature_dim = feature_dim
        self.subsets = subsets
        self.subset_size = subset_size
        self.degree = degree
        self.gamma = gamma
        self.coef = coef
        self.seed = seed
        self._add_state("real_features", [], merge="cat")
        self._add_state("fake_features", [], merge="cat")

    @inference_update
    def update(self, images: Tensor, is_real: bool) -> "KernelInceptionDistance":
        """Add a batch of [B, 3, H, W] images (float32 in [0, 1] for the default model)."""
        from torcheval_amd.metrics.image.fid import FrechetInceptionDistance

        FrechetInceptionDistance._FID_update_input_check(self, images=images, is_real=is_real)
        return self.update_activations(self.model(images.to(self.device)), is_real)

    @torch.inference_mode()
    def update_activations(self, activations: Tensor, is_real: bool) -> "KernelInceptionDistance":
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
    def merge_state(self, metrics: Iterable["KernelInceptionDistance"]) -> "KernelInceptionDistance":
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
        """``(mean, std)`` as float32 scalars on the metric's device; ``ValueError`` while either
        side holds fewer than ``subset_size`` rows."""
        empty = torch.empty(0, self._feature_dim, device=self.device)
        real = torch.cat(self.real_features) if self.real_features else empty
        fake = torch.cat(self.fake_features) if self.fake_features else empty
        _kid_input_check(real, fake, self.subset_size)
        generator = None
        if self.seed is not None:
            generator = torch.Generator(device=self.device).manual_seed(self.seed)
        gamma = 1.0 / self._feature_dim if self.gamma is None else self.gamma
        return _kid_compute(real, fake, self.subsets, self.subset_size, self.degree, gamma, self.coef, generator)

    def to(self, device, *args, **kwargs) -> "KernelInceptionDistance":
        super().to(device, *args, **kwargs)
        self.model.to(self.device)
        return self
