"""K18 wrapper (csrc/kernels/kl_divergence.hip): KL divergence of corresponding rows of two
``[..., C]`` tensors of logits or of non-negative weights.

One wave streams both rows of a counted row pair once.  ``"none"`` is that launch alone; ``"sum"``,
``"mean"`` and the class update add a finish launch that folds the per-block FP64 ``(sum, count)``
partials in block order into the scalar result or into the two states: two launches, no atomic, no
host synchronisation, results bit-identical from run to run.  Native inputs are two ROCm tensors of
one dtype (float32 / float16 / bfloat16) with a unit stride along ``C``, leading dimensions that
flatten to one row stride, and corresponding rows at the same offset from a 16-byte boundary;
everything else is the caller's ATen form.  The ops are dispatcher ops only
(``torch.ops.torcheval_amd_kldiv``), so eager and compiled calls take the same route; a traced call
cannot see addresses, so there the op itself refuses (raises on) operands at different offsets.
A mask that is not contiguous is copied by the op first (one ATen copy); a contiguous one is read
in place.
"""

from typing import Optional, Tuple

import torch

from torcheval_amd.ops import compiling, use_native

_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
REDUCTIONS = ("none", "sum", "mean")  # the kernel's reduction codes are the positions

# kKlMaxBlocks of csrc/include/tea_kernels.h: the row launch's grid cap in blocks of four waves,
# one row per wave (held equal by tests/metrics/regression/test_kl_divergence.py)
MAX_BLOCKS = 1024
WAVES_PER_BLOCK = 4
ROWS_PER_LAUNCH = MAX_BLOCKS * WAVES_PER_BLOCK  # rows the row launch covers before its waves grid-stride


def _flat_rows(t: torch.Tensor) -> Optional[Tuple[int, int]]:
    """(rows, row stride in elements) of a ``[..., C]`` tensor, or None when its leading dimensions
    do not flatten to one stride."""
    rows, stride, first = 1, t.shape[-1], True
    for i in range(t.dim() - 2, -1, -1):
        if t.shape[i] == 1:
            continue
        if first:
            stride = t.stride(i)
        elif t.stride(i) != rows * stride:
            return None
        first = False
        rows *= t.shape[i]
    return (rows, stride) if stride >= 0 else None


def _same_phase(input: torch.Tensor, target: torch.Tensor) -> bool:
    """Whether the first rows lie element-aligned at one offset from a 16-byte boundary.  While
    torch.compile traces there are no addresses to ask: the answer is yes, and the op, which checks
    the addresses when it runs, raises where it was wrong (operands that torch allocated and that
    start at the same element offset of their rows never are)."""
    if compiling():
        return True
    a, b = input.data_ptr(), target.data_ptr()
    return a % input.element_size() == 0 and (a - b) % 16 == 0


def supported(input: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None) -> bool:
    """Whether the checked pair runs K18: ROCm tensors on one device, one native dtype, at least
    one row, ``1 <= C < 2^31``, unit strides along ``C``, leading dimensions that flatten, and
    corresponding rows at one offset from a 16-byte boundary.  Raises on a GPU without the
    extension (``use_native``)."""
    if not use_native(input) or target.device != input.device:
        return False
    if mask is not None and mask.device != input.device:
        return False
    if input.dtype not in _DTYPES or target.dtype != input.dtype:
        return False
    c = input.shape[-1]
    if not 1 <= c < 2**31 or input.numel() == 0:
        return False
    if c > 1 and (input.stride(-1) != 1 or target.stride(-1) != 1):
        return False
    fi, ft = _flat_rows(input), _flat_rows(target)
    if fi is None or ft is None:
        return False
    if not _same_phase(input, target):
        return False
    return fi[0] == 1 or ((fi[1] - ft[1]) * input.element_size()) % 16 == 0


def kl_update(input: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor], from_logits: bool,
              kl_sum: torch.Tensor, num_rows: torch.Tensor) -> None:
    """The two float64 scalar states += the sum of the counted rows' values and their number."""
    torch.ops.torcheval_amd_kldiv.kl_update(input, target, mask, from_logits, kl_sum, num_rows)


def kl_batch(input: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor], from_logits: bool,
             reduction: str) -> torch.Tensor:
    """Float32 result of one ``supported`` batch: the row values in the leading shape (0 for
    uncounted rows) for ``"none"``, else a scalar."""
    shape = input.shape[:-1] if reduction == "none" else ()
    out = torch.empty(shape, dtype=torch.float32, device=input.device)
    torch.ops.torcheval_amd_kldiv.kl_batch(input, target, mask, from_logits, REDUCTIONS.index(reduction), out)
    return out
