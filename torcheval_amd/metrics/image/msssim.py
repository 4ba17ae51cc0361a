"""Multi-scale structural similarity (MS-SSIM), class API.

Not in the reference tree (docs/parity.md, "Not in the reference").  As ``StructuralSimilarity``: the
states are two float64 scalars with merge kind ``"sum"``, so they live in the contiguous state buffer
and sync through the existing plans.  A ROCm update is K26's launches (csrc/kernels/msssim.hip): the
finish launch adds the batch's per-image values and its image count straight into the states, with no
host synchronisation and no ATen op.
"""

from typing import Iterable, Optional, Tuple

import torch

from torcheval_amd.metrics.functional.image.msssim import (
    _BETAS,
    _msssim_betas_check,
    _msssim_input_check,
    _msssim_update,
)
from torcheval_amd.metrics.functional.image.ssim import _ssim_constants, _ssim_param_check
from torcheval_amd.metrics.metric import Metric, inference_update
from torcheval_amd.ops import msssim as _k26
from torcheval_amd.ops import ssim as _k12

__all__ = ["MultiScaleStructuralSimilarity"]


class MultiScaleStructuralSimilarity(Metric[torch.Tensor]):
    """Mean multi-scale structural similarity over all images seen; see
    ``multiscale_structural_similarity`` for the definition and the parameters.

    Args:
        data_range: the value range of the images (1.0, or 255.0 for 8-bit data).
        kernel_size: odd window size, at least 3.
        sigma: standard deviation of the Gaussian window.
        k1, k2: the stabilising constants of the luminance and contrast terms.
        betas: the exponent of each level, a non-empty tuple of non-negative floats.
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
        betas: Tuple[float, ...] = _BETAS,
        device: Optional[torch.device] = None,
    ) -> None:
        super().__init__(device=device)
        _ssim_param_check(data_range, kernel_size, sigma)
        _msssim_betas_check(betas)
        self.data_range = data_range
        self.kernel_size = kernel_size
        self.sigma = sigma
        self.k1 = k1
        self.k2 = k2
        self.betas = betas
        self._add_state("msssim_sum", torch.tensor(0.0, dtype=torch.float64, device=self.device), merge="sum")
        self._add_state("num_images", torch.tensor(0.0, dtype=torch.float64, device=self.device), merge="sum")

    @inference_update
    def update(self, input: torch.Tensor, target: torch.Tensor) -> "MultiScaleStructuralSimilarity":
        """Add the images of one ``[N, C, H, W]`` batch pair."""
        _msssim_input_check(input, target, self.kernel_size, len(self.betas))
        n = input.shape[0]
        if n == 0:
            return self
        c1, c2 = _ssim_constants(self.data_range, self.k1, self.k2)
        if input.shape[1] == 0:  # no channels: every image's value is the mean over nothing
            self.msssim_sum += torch.nan
            self.num_images += n
            return self
        if input.device == self.msssim_sum.device and _k26.supported(input, target, self.kernel_size,
                                                                     len(self.betas)):
            _k26.msssim(input.contiguous(), target.contiguous(), _k12.gaussian_taps(self.kernel_size, self.sigma),
                        self.betas, c1, c2, None, False, self.msssim_sum, self.num_images)
            return self
        per_image = _msssim_update(input, target, c1, c2, self.kernel_size, self.sigma, self.betas)
        self.msssim_sum += per_image.sum(dtype=torch.float64).to(self.device)
        self.num_images += n
        return self

    @torch.inference_mode()
    def compute(self) -> torch.Tensor:
        """The mean MS-SSIM of all images as float32; NaN before any update."""
        return (self.msssim_sum / self.num_images).float()

    @torch.inference_mode()
    def merge_state(
        self, metrics: Iterable["MultiScaleStructuralSimilarity"]
    ) -> "MultiScaleStructuralSimilarity":
        for metric in metrics:
            self.msssim_sum += metric.msssim_sum.to(self.device)
            self.num_images += metric.num_images.to(self.device)
        return self
