"""K16 wrapper (csrc/kernels/corrcoef.hip): Pearson and concordance correlation per task from the
six-moment state ``[6, tasks]`` (``n, mean_x, mean_y, m2_x, m2_y, c_xy``, float64).

A class update or a functional call is two launches and no host synchronisation: the sums launch
(row arm for a unit stride along the samples, column arm for the transposed view of a row-major
``[n, tasks]`` tensor) writes one FP64 5-tuple per (task, block), and the finish launch, a wave per
task, forms the batch's moments and merges them into the state or writes the value.
``merge_state`` and ``compute()`` of the class are one launch each.  Native inputs are float32 /
float16 / bfloat16 operands, each with its own dtype, strides and alignment; everything else is
the caller's ATen form.  The ops are dispatcher ops only (``torch.ops.torcheval_amd_corrcoef``), so
eager and compiled calls take the same route.
"""

import torch

from torcheval_amd.ops import use_native

_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
KINDS = ("pearson", "concordance")  # the kernels' kind codes are the positions

# kCorrRowSpan / kCorrColSpan / kCorrColTasks of csrc/include/tea_kernels.h (held equal by
# tests/metrics/regression/test_pearson.py): the tile edges at which the GPU tests place their shapes
ROW_SPAN = 4096
COL_SPAN = 128
COL_TASKS = 64


def _rows(v: torch.Tensor) -> torch.Tensor:
    return v if v.dim() == 2 else v.unsqueeze(0)


def arm(input: torch.Tensor, target: torch.Tensor) -> str:
    """``"row"``, ``"column"`` or ``""`` (no arm takes the layout) for ``[tasks, n]`` operands: unit
    strides along the samples, or the transposed views of row-major ``[n, >= tasks]`` parents
    (``stride(0) == 1``, ``stride(1) >= tasks``).  A shape both arms could take goes to the row arm;
    one task's samples at a stride (``x[::2]``) go to neither."""
    tasks, n = input.shape
    if n == 1 or (input.stride(1) == 1 and target.stride(1) == 1):
        return "row"
    if input.stride(0) == 1 and target.stride(0) == 1 and min(input.stride(1), target.stride(1)) >= tasks:
        return "column"
    return ""


def supported(input: torch.Tensor, target: torch.Tensor) -> bool:
    """Whether the pair runs K16: ROCm tensors of native dtypes on one device, equal ``[n]`` or
    ``[tasks, n]`` shapes with ``tasks >= 1`` and ``1 <= n < 2^31``, in a layout one of the arms
    takes.  Raises on a GPU without the extension (``use_native``)."""
    if not use_native(input) or target.device != input.device:
        return False
    if input.dtype not in _DTYPES or target.dtype not in _DTYPES:
        return False
    if input.dim() not in (1, 2) or target.shape != input.shape or input.shape[0] == 0:
        return False
    if not 1 <= input.shape[-1] < 2**31:
        return False
    return arm(_rows(input), _rows(target)) != ""


def corrcoef_update(input: torch.Tensor, target: torch.Tensor, moments: torch.Tensor) -> None:
    """``moments`` (float64 ``[6, tasks]``) <- its pairwise merge with the moments of one
    ``supported`` batch."""
    torch.ops.torcheval_amd_corrcoef.corrcoef_update(_rows(input), _rows(target), moments)


def corrcoef_batch(input: torch.Tensor, target: torch.Tensor, kind: str) -> torch.Tensor:
    """Float32 ``[tasks]`` value (``kind`` one of ``KINDS``) of one ``supported`` batch."""
    x, y = _rows(input), _rows(target)
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    torch.ops.torcheval_amd_corrcoef.corrcoef_batch(x, y, KINDS.index(kind), out)
    return out


def corrcoef_merge(moments: torch.Tensor, other: torch.Tensor) -> None:
    """``moments`` <- its pairwise merge with ``other``, both float64 ``[6, tasks]`` on one ROCm
    device."""
    torch.ops.torcheval_amd_corrcoef.corrcoef_merge(moments, other)


def corrcoef_value(moments: torch.Tensor, kind: str) -> torch.Tensor:
    """Float32 ``[tasks]`` value of a float64 ``[6, tasks]`` ROCm state."""
    out = torch.empty(moments.shape[1], dtype=torch.float32, device=moments.device)
    torch.ops.torcheval_amd_corrcoef.corrcoef_value(moments, KINDS.index(kind), out)
    return out
