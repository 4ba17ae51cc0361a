"""K27 wrapper (csrc/kernels/surface_distance.hip): Hausdorff and average surface distance of integer
label-map pairs ``[N, H, W]`` on ROCm, for unit pixel spacing.

A plane is (image, class, side).  The row launch writes, per plane, the distance along the row to the
nearest surface pixel (``g``, 16 bits) and counts the surface pixels; the search launch walks the other
side's ``g`` up and down the column of every surface pixel and writes its squared distance (``d2``, 32
bits); the finish launch reduces a plane to a maximum, a percentile or a sum, and the combine launch
forms the ``[N, K]`` values and the class states.  Squared distances are integers until the final
square root, so a result is exact and bit-identical from run to run.  No host synchronisation.  Native
inputs are contiguous maps of ``LABEL_DTYPES`` with sides of at most ``MAX_SIDE`` and at most
``MAX_CLASSES`` classes; everything else is the caller's ATen form.  A batch whose workspaces exceed
``WORKSPACE_CAP`` bytes runs in chunks of whole images.  The op is a dispatcher op only
(``torch.ops.torcheval_amd_surface``), so eager and compiled calls take the same route.
"""

from typing import Optional

import torch

from torcheval_amd.ops import use_native
from torcheval_amd.ops.segmentation import LABEL_DTYPES

MAX_SIDE = 2048  # kSurfMaxSide of csrc/include/tea_kernels.h
MAX_CLASSES = 64  # kSurfMaxClasses
WORKSPACE_CAP = 256 << 20  # bytes of g and d2 per call of the op
_PLANE_BYTES = 6  # of g (2) and d2 (4) per pixel of a plane


def supported(input: torch.Tensor, target: torch.Tensor, num_classes: int) -> bool:
    """Whether the (checked) pair of label maps runs K27.  Raises on a GPU without the extension
    (``use_native``).  The geometry test is a hand-kept twin of ``surface_distance_geometry_ok`` in
    the kernel file, which the binding applies again."""
    if not use_native(input) or target.device != input.device:
        return False
    if input.dtype not in LABEL_DTYPES or target.dtype not in LABEL_DTYPES or input.ndim != 3:
        return False
    if not (input.is_contiguous() and target.is_contiguous()) or input.numel() == 0:
        return False
    return 1 <= num_classes <= MAX_CLASSES and max(input.shape[1:]) <= MAX_SIDE


def images_per_call(classes: int, h: int, w: int) -> int:
    """The most whole images whose ``g`` and ``d2`` stay within ``WORKSPACE_CAP`` (at least one)."""
    return max(1, WORKSPACE_CAP // (classes * 2 * h * w * _PLANE_BYTES))


def surface_distance(input: torch.Tensor, target: torch.Tensor, classes: int, class_base: int, mode: int,
                     quantile: float, both: bool, out: Optional[torch.Tensor],
                     value_sum: Optional[torch.Tensor] = None, num_finite: Optional[torch.Tensor] = None,
                     num_inf: Optional[torch.Tensor] = None) -> None:
    """``out`` ([N, classes] float32) <- the values of ``supported`` maps, column ``k`` the class
    ``k + class_base``; the ``[classes]`` float64 states += the finite values, their number and the
    number of ``+inf``.  ``mode`` 0: Hausdorff (``quantile`` < 0 the maximum, else percentile / 100);
    1: average surface distance.  ``both``: both directions."""
    n, h, w = input.shape
    step = min(n, images_per_call(classes, h, w))
    planes = step * classes * 2
    dev = input.device
    g = torch.empty(planes * h * w, dtype=torch.int16, device=dev)
    d2 = torch.empty(planes * h * w, dtype=torch.int32, device=dev)
    counts = torch.empty(planes, dtype=torch.int32, device=dev)
    partials = torch.empty(planes * 2, dtype=torch.float64, device=dev)
    for i in range(0, n, step):
        torch.ops.torcheval_amd_surface.surface_distance(
            input[i:i + step], target[i:i + step], classes, class_base, mode, quantile, both, g, d2, counts, partials,
            None if out is None else out[i:i + step], value_sum, num_finite, num_inf)
