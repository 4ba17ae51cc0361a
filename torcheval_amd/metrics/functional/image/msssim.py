"""Multi-scale structural similarity (MS-SSIM), functional API.

Not in the reference tree (docs/parity.md, "Not in the reference"): Wang, Simoncelli and Bovik 2003
with SSIM's separable Gaussian window applied without padding and 2 x 2 average pooling between the
levels.  ROCm tensors run K26 (csrc/kernels/msssim.hip); CPU tensors, float64 / mixed dtypes, windows
above 15 taps and more than 8 levels run the ATen form below, which is the definition written out.
"""

from typing import Tuple

import torch
import torch.nn.functional as F

from torcheval_amd.metrics.functional.image.ssim import _ssim_constants, _ssim_param_check
from torcheval_amd.ops import msssim as _k26
from torcheval_amd.ops import ssim as _k12

__all__ = ["multiscale_structural_similarity"]

_BETAS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


@torch.inference_mode()
def multiscale_structural_similarity(
    input: torch.Tensor,
    target: torch.Tensor,
    data_range: float = 1.0,
    *,
    kernel_size: int = 11,
    sigma: float = 1.5,
    k1: float = 0.01,
    k2: float = 0.03,
    betas: Tuple[float, ...] = _BETAS,
    reduction: str = "mean",
) -> torch.Tensor:
    """Multi-scale structural similarity of ``[N, C, H, W]`` image pairs over ``M = len(betas)`` levels.

    Level 0 is the input pair and level ``j + 1`` is ``avg_pool2d(level j, 2)`` (floor: an odd last
    row or column is dropped).  Per level and plane (image, channel), with the window, ``C1`` and
    ``C2`` of ``structural_similarity``: ``cs = (2 sxy + C2) / (sxx + syy + C2)`` and
    ``ssim = cs (2 mx my + C1) / (mx^2 + my^2 + C1)``, each averaged over the level's positions.  A
    plane's value is ``prod_{j < M-1} max(cs_j, 0)^betas[j] * max(ssim_{M-1}, 0)^betas[M-1]`` and an
    image's value the mean of its planes' values (the per-channel product of ``pytorch-msssim`` and
    TensorFlow).  Class version: ``MultiScaleStructuralSimilarity``.

    Args:
        input, target: images of one shape ``[N, C, H, W]`` with
            ``min(H, W) >> (M - 1) >= kernel_size``.
        data_range: the value range of the images (1.0, or 255.0 for 8-bit data).
        kernel_size: odd window size, at least 3.
        sigma: standard deviation of the window.
        k1, k2: the stabilising constants of the luminance and contrast terms.
        betas: the exponent of each level, a non-empty tuple of non-negative floats.
        reduction: ``"mean"`` (0-d float32 mean over the images) or ``"none"`` (``[N]`` float32).
    """
    _ssim_param_check(data_range, kernel_size, sigma, reduction)
    _msssim_betas_check(betas)
    _msssim_input_check(input, target, kernel_size, len(betas))
    mean = reduction == "mean"
    n = input.shape[0]
    if input.shape[1] == 0:  # no channels: the mean over nothing
        return torch.full(() if mean else (n,), torch.nan, device=input.device)
    if n == 0:
        return torch.full((), torch.nan, device=input.device) if mean else torch.empty(0, device=input.device)
    c1, c2 = _ssim_constants(data_range, k1, k2)
    if _k26.supported(input, target, kernel_size, len(betas)):
        out = torch.empty(() if mean else (n,), dtype=torch.float32, device=input.device)
        _k26.msssim(input.contiguous(), target.contiguous(), _k12.gaussian_taps(kernel_size, sigma), betas, c1, c2,
                    out, mean)
        return out
    per_image = _msssim_update(input, target, c1, c2, kernel_size, sigma, betas)
    return (per_image.mean() if mean else per_image).float()


def _msssim_betas_check(betas: Tuple[float, ...]) -> None:
    if type(betas) is not tuple or len(betas) == 0 or any(type(b) is not float or not b >= 0 for b in betas):
        raise ValueError(f"`betas` needs to be a non-empty `tuple` of non-negative `float`s, got {betas}.")


def _msssim_input_check(input: torch.Tensor, target: torch.Tensor, kernel_size: int, levels: int) -> None:
    if input.shape != target.shape:
        raise ValueError(
            f"The `input` and `target` must have the same shape, got shapes {input.shape} and {target.shape}."
        )
    if input.ndim != 4:
        raise ValueError(f"The `input` and `target` must be 4-D [N, C, H, W] tensors, got shape {input.shape}.")
    if min(input.shape[2], input.shape[3]) >> (levels - 1) < kernel_size:
        raise ValueError(
            f"The image height and width must be at least {_k26.min_side(kernel_size, levels)} for {levels} levels "
            f"and `kernel_size` {kernel_size}, got shape {input.shape}."
        )


def _msssim_update(input: torch.Tensor, target: torch.Tensor, c1: float, c2: float, kernel_size: int, sigma: float,
                   betas: Tuple[float, ...]) -> torch.Tensor:
    """The ATen form, exactly as defined: per-image MS-SSIM ``[N]`` in float64 when either input is
    float64, in float32 otherwise."""
    dtype = torch.float64 if torch.float64 in (input.dtype, target.dtype) else torch.float32
    x, y = input.to(dtype), target.to(dtype)
    channels = x.shape[1]
    g = torch.tensor(_k12.gaussian_taps(kernel_size, sigma), dtype=torch.float64, device=x.device)
    window = torch.outer(g, g).to(dtype).expand(channels, 1, kernel_size, kernel_size).contiguous()

    def filt(t: torch.Tensor) -> torch.Tensor:
        return F.conv2d(t, window, groups=channels)

    value = None
    for j, beta in enumerate(betas):
        if j > 0:
            x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
        mx, my = filt(x), filt(y)
        sxx = filt(x * x) - mx * mx
        syy = filt(y * y) - my * my
        sxy = filt(x * y) - mx * my
        term = (2 * sxy + c2) / (sxx + syy + c2)
        if j == len(betas) - 1:
            term = term * (2 * mx * my + c1) / (mx * mx + my * my + c1)
        term = term.mean(dim=(2, 3)).clamp(min=0) ** beta  # [N, C]
        value = term if value is None else value * term
    return value.mean(dim=1)
