"""K20 wrapper (csrc/kernels/kid.hip): the Kernel Inception Distance of index-listed subsets.

Per call two launches: ``kid_gram`` (one block per 128 x 128 tile of the XX, YY and XY Gram blocks of
every subset on FP32 MFMA, rows fetched through the index lists, the polynomial kernel, the mask
and the sum applied in registers, one FP64 partial per tile) and ``kid_finish`` (the three sums and
``mmd2`` per subset, then their mean and population standard deviation).  No host synchronisation,
no atomics.  Native inputs are float32 features with unit stride along the feature axis and any row
stride; float16 / bfloat16 features are widened here (one exact copy); everything else is the
caller's ATen form.
"""

from typing import Tuple

import torch

from torcheval_amd.ops import use_native

# kKidTile of csrc/include/tea_kernels.h (held equal by tests/metrics/image/test_kid.py): the side
# of one Gram tile, at whose edges the GPU tests place their subset sizes
TILE = 128

_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def items(m: int) -> int:
    """Tiles per subset of ``m`` rows: ``T (T + 1) / 2`` of XX, as many of YY, ``T^2`` of XY."""
    t = (m + TILE - 1) // TILE
    return t * (t + 1) + t * t


def supported(real: torch.Tensor, fake: torch.Tensor, idx_r: torch.Tensor, idx_f: torch.Tensor) -> bool:
    """Whether the call runs K20: ROCm ``[n, D]`` features of one native dtype family on one device
    with unit stride along ``D >= 1``, and ``[S >= 1, m >= 2]`` index tensors of one shape on that
    device.  Raises on a GPU without the extension (``use_native``)."""
    if not use_native(real) or any(t.device != real.device for t in (fake, idx_r, idx_f)):
        return False
    if real.dtype not in _DTYPES or fake.dtype not in _DTYPES:
        return False
    if real.dim() != 2 or fake.dim() != 2 or real.shape[1] != fake.shape[1] or real.shape[1] < 1:
        return False
    if real.shape[0] < 1 or fake.shape[0] < 1 or max(real.shape[0], fake.shape[0]) >= 2**31:
        return False
    if real.shape[1] > 1 and (real.stride(1) != 1 or fake.stride(1) != 1):
        return False
    if idx_r.dim() != 2 or idx_r.shape != idx_f.shape or idx_r.shape[0] < 1 or idx_r.shape[1] < 2:
        return False
    return idx_r.shape[1] < 2**24 and idx_r.shape[0] * items(idx_r.shape[1]) < 2**31 - 8


def kid(real: torch.Tensor, fake: torch.Tensor, idx_r: torch.Tensor, idx_f: torch.Tensor, degree: int,
        gamma: float, coef: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(out, values, sums)`` of a ``supported`` call: float32 ``[2]`` (mean, population standard
    deviation of ``values``), float64 ``[S]`` ``mmd2`` per subset and float64 ``[S, 3]``
    ``(sxx, syy, sxy)``.  Indices in ``[0, n)`` are the precondition (the kernel clamps, so a bad
    one reads a wrong row, never outside the tensor).  Both ops are dispatcher ops only
    (``torch.ops.torcheval_amd_kid``), so the call stays in a compiled graph."""
    if real.dtype != torch.float32:
        real = real.float()
    if fake.dtype != torch.float32:
        fake = fake.float()
    if idx_r.dtype != torch.int32 or not idx_r.is_contiguous():
        idx_r = idx_r.to(torch.int32).contiguous()
    if idx_f.dtype != torch.int32 or not idx_f.is_contiguous():
        idx_f = idx_f.to(torch.int32).contiguous()
    subsets, m = idx_r.shape
    dev = real.device
    partials = torch.empty(subsets, items(m), dtype=torch.float64, device=dev)
    sums = torch.empty(subsets, 3, dtype=torch.float64, device=dev)
    values = torch.empty(subsets, dtype=torch.float64, device=dev)
    out = torch.empty(2, dtype=torch.float32, device=dev)
    torch.ops.torcheval_amd_kid.kid_gram(real, fake, idx_r, idx_f, float(gamma), float(coef), int(degree), partials)
    torch.ops.torcheval_amd_kid.kid_finish(partials, m, sums, values, out)
    return out, values, sums
