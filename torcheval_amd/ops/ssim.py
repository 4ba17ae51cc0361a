"""K12 wrapper (csrc/kernels/ssim.hip): structural similarity of [N, C, H, W] image pairs on ROCm.

Two launches, no host synchronisation: ``ssim_tiles`` (one workgroup per plane and output tile:
LDS halos of both inputs, the separable window, the SSIM expression, one FP64 partial) and
``ssim_finish`` (per-image values or their mean, and the class states).  Native inputs are
contiguous float32 / float16 / bfloat16 / uint8 pairs of one dtype with an odd window of at most
``max_kernel_size()`` taps; everything else is the caller's ATen form.
"""

import functools
import math
from typing import Optional, Tuple

import torch

import torcheval_amd.ops as _ops
from torcheval_amd.ops import native, use_native

_DTYPES = (torch.float32, torch.float16, torch.bfloat16, torch.uint8)


@functools.lru_cache(maxsize=32)
def gaussian_taps(kernel_size: int, sigma: float) -> Tuple[float, ...]:
    """``exp(-(i - (ks - 1) / 2)^2 / (2 sigma^2))``, normalised to sum 1 in FP64."""
    mid = (kernel_size - 1) / 2.0
    g = [math.exp(-((i - mid) ** 2) / (2.0 * sigma * sigma)) for i in range(kernel_size)]
    total = math.fsum(g)
    return tuple(v / total for v in g)


def tile_shape() -> Tuple[int, int]:
    """(rows, columns) of one workgroup's output tile."""
    return native().ssim_tile_rows(), native().ssim_tile_cols()


def max_kernel_size() -> int:
    return native().ssim_max_kernel_size()


def supported(input: torch.Tensor, target: torch.Tensor, kernel_size: int) -> bool:
    """Whether the pair runs K12: ROCm tensors of one native dtype, non-empty, a window and a
    geometry the launch covers.  Raises on a GPU without the extension (``use_native``)."""
    if not use_native(input) or target.device != input.device:
        return False
    if input.dtype != target.dtype or input.dtype not in _DTYPES or input.numel() == 0:
        return False
    n, c, h, w = input.shape
    return native().ssim_geometry_ok(n * c, h, w, kernel_size)


def ssim(input: torch.Tensor, target: torch.Tensor, taps, c1: float, c2: float, out: Optional[torch.Tensor],
         mean: bool, mssim_sum: Optional[torch.Tensor] = None, num_images: Optional[torch.Tensor] = None) -> None:
    """``out`` <- per-image SSIM ([N] float32) or its mean (one element) of contiguous inputs;
    ``mssim_sum`` += the sum of the N values and ``num_images`` += N (float64 scalars).
    Eager calls take the pybind entry; under torch.compile the dispatcher op keeps the call in
    the graph."""
    if _ops.compiling():
        torch.ops.torcheval_amd.ssim(input, target, list(taps), c1, c2, out, mean, mssim_sum, num_images)
        return
    native().ssim(input, target, taps, c1, c2, out, mean, mssim_sum, num_images)
