"""Structural similarity (SSIM), class API.

Not in the reference tree (docs/parity.md, "Not in the reference").  The states are two float64
scalars with merge kind ``"sum"``, so they live in the contiguous state buffer and sync through
the existing plans.  A ROCm update is K12's two launches (csrc/kernels/ssim.hip): the finish
launch adds the batch's per-image values and its image count straight into the states, with no
host synchronisation and no ATen op.
"""

from typing import Iterable, Optional

import torch

from torcheval_amd.metrics.functional.image.ssim import (
    _ssim_constants,
    _ssim_input_check,
    _ssim_param_check,
    _ssim_update,
)
from torcheval_amd.metrics.metric import Metric, inference_update
from torcheval_amd.ops import ssim as _k12

__all__ = ["StructuralSimilarity"]


class StructuralSimilarity(Metric[torch.Tensor]):
    """Mean structural similarity over all images seen; see ``structural_similarity`` for the
    definition and the parameters.

    Args:
        data_range: the value range of the images (1.0, or 255.0 for 8-bit data).
        kernel_size: odd window size, at least 3.
        sigma: standard deviation of the Gaussian window.
        k1, k2: the stabilising constants of the luminance and contrast terms.
        device: where the states live.
    """

    def __init__(
        self,
        data_range: float = 1.0,
        *,
        kernel_size: int = 11,
        sigma: float = 1.5,
        k1: float = 0.01,
        k2: float = 0.03,
        device: Optional[torch.device] = None,
    ) -> None:
        super().__init__(device=device)
        _ssim_param_check(data_range, kernel_size, sigma)
        self.data_range = data_range
        self.kernel_size = kernel_size
        self.sigma = sigma
        self.k1 = k1
        self.k2 = k2
        self._add_state("mssim_sum", torch.tensor(0.0, dtype=torch.float64, device=self.device), merge="sum")
        self._add_state("num_images", torch.tensor(0.0, dtype=torch.float64, device=self.device), merge="sum")

    @inference_update
    def update(self, input: torch.Tensor, target: torch.Tensor) -> "StructuralSimilarity":
        """Add the images of one ``[N, C, H, W]`` batch pair."""
        _ssim_input_check(input, target, self.kernel_size)
        n = input.shape[0]
        if n == 0:
            return self
        c1, c2 = _ssim_constants(self.data_range, self.k1, self.k2)
        if input.shape[1] == 0:  # no channels: every image's value is the mean over nothing
            self.mssim_sum += torch.nan
            self.num_images += n
            return self
        if input.device == self.mssim_sum.device and _k12.supported(input, target, self.kernel_size):
            _k12.ssim(input.contiguous(), target.contiguous(), _k12.gaussian_taps(self.kernel_size, self.sigma),
                      c1, c2, None, False, self.mssim_sum, self.num_images)
            return self
        per_image = _ssim_update(input, target, c1, c2, self.kernel_size, self.sigma)
        self.mssim_sum += per_image.sum(dtype=torch.float64).to(self.device)
        self.num_images += n
        return self

    @torch.inference_mode()
    def compute(self) -> torch.Tensor:
        """The mean SSIM of all images as float32; NaN before any update."""
        return (self.mssim_sum / self.num_images).float()

    @torch.inference_mode()
    def merge_state(self, metrics: Iterable["StructuralSimilarity"]) -> "StructuralSimilarity":
        for metric in metrics:
            self.mssim_sum += metric.mssim_sum.to(self.device)
            self.num_images += metric.num_images.to(self.device)
        return self
