"""K26 wrapper (csrc/kernels/msssim.hip): multi-scale SSIM of [N, C, H, W] image pairs on ROCm.

Level 0 is the input pair and level ``j + 1`` the 2 x 2 average of level ``j``.  A level whose plane
does not fit one K12 halo is one ``msssim_level`` launch (K12's tiles; it also writes the pooled
(x, y) pairs of the next level into the workspace); from the first level that fits, one ``msssim_tail``
launch runs every remaining level out of LDS; ``msssim_finish`` forms the per-image values or their
mean, and the class states.  No host synchronisation.  Native inputs are contiguous float32 / float16
/ bfloat16 / uint8 pairs of one dtype with an odd window of at most K12's ``max_kernel_size()`` taps
and at most ``MAX_LEVELS`` levels; everything else is the caller's ATen form.  The op is a dispatcher
op only (``torch.ops.torcheval_amd_msssim``), so eager and compiled calls take the same route.
"""

from typing import Dict, Optional, Sequence

import torch

from torcheval_amd.ops import native, use_native
from torcheval_amd.ops import ssim as _k12

MAX_LEVELS = 8  # kMsssimMaxLevels of csrc/include/tea_kernels.h

_DTYPES = (torch.float32, torch.float16, torch.bfloat16, torch.uint8)


def min_side(kernel_size: int, levels: int) -> int:
    """The smallest image side whose last level still holds one window."""
    return kernel_size << (levels - 1)


def plan(h: int, w: int, kernel_size: int, levels: int) -> Dict[str, object]:
    """The level plan as host integers (``msssim_plan`` of the kernel file): the plane ``sizes`` per
    level, the first level of the tail launch (``tail == levels``: none), per level the partials of a
    plane (``per``) and the per-plane offsets of the level's partials (``part_off``) and of its
    workspace pairs (``ws_off``, levels 1 .. ``tail``), and the per-plane totals.

    A hand-kept twin of ``msssim_plan`` in csrc/kernels/msssim.hip: change both together.  The binding
    checks the buffers sized from here against the C++ plan and raises when they are too small."""
    th, tw = _k12.tile_shape()
    sizes = [(h >> j, w >> j) for j in range(levels)]
    tail = next((j for j, (hj, wj) in enumerate(sizes) if hj <= th + kernel_size - 1 and wj <= tw + kernel_size - 1),
                levels)
    per, part_off, ws_off, partials, ws_pairs = [], [], [], 0, 0
    for j, (hj, wj) in enumerate(sizes):
        per.append(-(-(hj - kernel_size + 1) // th) * -(-(wj - kernel_size + 1) // tw) if j < tail else 1)
        part_off.append(partials)
        partials += per[-1]
        ws_off.append(ws_pairs if 1 <= j <= tail else 0)
        if 1 <= j <= tail:
            ws_pairs += hj * wj
    return {"sizes": sizes, "tail": tail, "per": per, "part_off": part_off, "ws_off": ws_off,
            "partials": partials, "ws_pairs": ws_pairs}


def supported(input: torch.Tensor, target: torch.Tensor, kernel_size: int, levels: int) -> bool:
    """Whether the pair runs K26: ROCm tensors of one native dtype, non-empty, a window, a number of
    levels and a geometry the launches cover.  Raises on a GPU without the extension (``use_native``).
    The geometry test is a hand-kept twin of ``msssim_geometry_ok`` in csrc/kernels/msssim.hip (K12's
    ``ssim_geometry_ok`` and the level rule): change both together."""
    if not use_native(input) or target.device != input.device:
        return False
    if input.dtype != target.dtype or input.dtype not in _DTYPES or input.numel() == 0:
        return False
    n, c, h, w = input.shape
    if not 1 <= levels <= MAX_LEVELS or min(h, w) < min_side(kernel_size, levels):
        return False
    return native().ssim_geometry_ok(n * c, h, w, kernel_size)


def msssim(input: torch.Tensor, target: torch.Tensor, taps: Sequence[float], betas: Sequence[float], c1: float,
           c2: float, out: Optional[torch.Tensor], mean: bool, value_sum: Optional[torch.Tensor] = None,
           num_images: Optional[torch.Tensor] = None) -> None:
    """``out`` <- per-image MS-SSIM ([N] float32) or its mean (one element) of contiguous ``supported``
    inputs; ``value_sum`` += the sum of the N values and ``num_images`` += N (float64 scalars)."""
    n, c, h, w = input.shape
    p = plan(h, w, len(taps), len(betas))
    workspace = torch.empty(n * c * p["ws_pairs"] * 2, dtype=torch.float32, device=input.device)
    partials = torch.empty(n * c * p["partials"], dtype=torch.float64, device=input.device)
    torch.ops.torcheval_amd_msssim.msssim(input, target, list(taps), list(betas), c1, c2, workspace, partials, out,
                                          mean, value_sum, num_images)
