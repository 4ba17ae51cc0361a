"""K19 wrapper (csrc/kernels/kendall.hip): Kendall's tau per row of [rows, n] operand pairs.

Per call: ``target`` packed to float32 and sorted by K3a (descending, the int32 source permutation
as its order); ``kendall_prepare`` (the tie-run start ``s`` of every sorted position, ``input``
gathered into that order, the target's tie partials); a second, stable K3a
sort of the gathered ``input`` that carries ``s`` as its payload; then ``kendall_count``:
``kendall_ties`` (tie partials of ``input`` and of both operands), ``kendall_tile`` (tiles of the
carried sequence sorted in LDS, their strict inversions counted), one ``kendall_merge`` launch per
level of ``ceil(log2 tiles)`` and ``kendall_finish`` (the value and the six integer counts per row).
No host synchronisation anywhere.  Native inputs are float32 / float16 / bfloat16 and int8 / uint8 /
int16, all exact in float32, with any strides; everything else is the caller's ATen form.
"""

from typing import Tuple

import torch

import torcheval_amd.ops as _ops
from torcheval_amd.ops import native, use_native
from torcheval_amd.ops.rankcorr import _DTYPES, _pack

# kKendallTile of csrc/include/tea_kernels.h (held equal by tests/metrics/regression/test_kendall.py):
# the span of the run kernels and the tile of the merge kernels, at whose edges the GPU tests place
# their shapes
TILE = 2048


def supported(input: torch.Tensor, target: torch.Tensor) -> bool:
    """Whether the pair runs K19: ROCm tensors of native dtypes on one device, equal ``[n]`` or
    ``[rows, n]`` shapes, ``rows >= 1`` and ``2 <= n < 2^31``.  Raises on a GPU without the
    extension (``use_native``)."""
    if not use_native(input) or target.device != input.device:
        return False
    if input.dtype not in _DTYPES or target.dtype not in _DTYPES:
        return False
    if input.dim() not in (1, 2) or target.shape != input.shape or input.shape[0] == 0:
        return False
    return 2 <= input.shape[-1] < 2**31


def _sort(x: torch.Tensor, s: torch.Tensor, order: torch.Tensor, payload, kind: int) -> None:
    """K3a: its pybind entry in eager calls, its dispatcher op under torch.compile."""
    if _ops.compiling():
        torch.ops.torcheval_amd.sort_desc(x, s, order, payload, kind, False)
    else:
        native().sort_desc(x, s, order, payload, kind)


def kendall(input: torch.Tensor, target: torch.Tensor, variant_c: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """Float32 ``[rows]`` tau (tau-c when ``variant_c``) and int64 ``[rows, 6]`` counts
    ``(n1, n2, n3, Q, mx, my)`` of a ``supported`` pair; a row that holds a NaN has NaN and counts
    of -1.  ``kendall_prepare`` and ``kendall_count`` are dispatcher ops only
    (``torch.ops.torcheval_amd_kendall``), so the call stays in a compiled graph."""
    x = input if input.dim() == 2 else input.unsqueeze(0)
    y = target if target.dim() == 2 else target.unsqueeze(0)
    rows, n = x.shape
    dev = x.device
    xp, yp, ys, xg, xs = (torch.empty(rows, n, dtype=torch.float32, device=dev) for _ in range(5))
    perm, s, carried = (torch.empty(rows, n, dtype=torch.int32, device=dev) for _ in range(3))
    part = torch.empty(rows, 6, (n + TILE - 1) // TILE, dtype=torch.int64, device=dev)
    flags = torch.empty(rows, 2, dtype=torch.int32, device=dev)
    out = torch.empty(rows, dtype=torch.float32, device=dev)
    counts = torch.empty(rows, 6, dtype=torch.int64, device=dev)
    _pack(yp, y)
    _pack(xp, x)
    _sort(yp, ys, perm, None, 0)
    torch.ops.torcheval_amd_kendall.kendall_prepare(ys, perm, xp, s, xg, part, flags)
    _sort(xg, xs, carried, s, 2)
    torch.ops.torcheval_amd_kendall.kendall_count(xs, carried, part, flags, int(variant_c), out, counts)
    return out, counts
