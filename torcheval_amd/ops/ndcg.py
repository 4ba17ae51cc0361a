"""K13 wrapper (csrc/kernels/ndcg.hip): normalized DCG per row of [N, C] scores / graded relevance.

One launch for the row values (a wave per row for ``C <= 64``, a workgroup per row with the row
sorted in LDS up to ``max_columns()``); with class states a finish launch adds the blocks' FP64
partials in a fixed order.  Native inputs are float32 / float16 / bfloat16 scores and float32 /
float16 / bfloat16 / int64 / int32 / int16 / int8 / uint8 relevance with a unit column stride and
any row stride; everything else is the caller's ATen form.  The discount prefix table the kernel
reads is built on the host and cached per device by the extension.
"""

from typing import Optional

import torch

import torcheval_amd.ops as _ops
from torcheval_amd.ops import native, use_native

_SCORE_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_RELEVANCE_DTYPES = (
    torch.float32,
    torch.float16,
    torch.bfloat16,
    torch.int64,
    torch.int32,
    torch.int16,
    torch.int8,
    torch.uint8,
)


# read once at import: a plain int, so ``supported`` also traces under torch.compile
_MAX_COLUMNS: Optional[int] = _ops._C.ndcg_max_columns() if _ops.native_loaded() else None


def max_columns() -> int:
    """The widest row K13 takes."""
    return native().ndcg_max_columns() if _MAX_COLUMNS is None else _MAX_COLUMNS


def supported(input: torch.Tensor, target: torch.Tensor) -> bool:
    """Whether the pair runs K13: ROCm tensors of native dtypes, ``1 <= C <= max_columns()`` and a
    unit column stride.  Raises on a GPU without the extension (``use_native``)."""
    if not use_native(input) or target.device != input.device:
        return False
    if input.dtype not in _SCORE_DTYPES or target.dtype not in _RELEVANCE_DTYPES:
        return False
    if input.dim() != 2 or target.shape != input.shape or input.shape[0] == 0:
        return False
    c = input.shape[1]
    if c < 1 or c > max_columns():
        return False
    return c == 1 or (input.stride(1) == 1 and target.stride(1) == 1)


def ndcg(input: torch.Tensor, target: torch.Tensor, k: int, exponential_gain: bool, out: Optional[torch.Tensor],
         ndcg_sum: Optional[torch.Tensor] = None, num_rows: Optional[torch.Tensor] = None,
         err: Optional[torch.Tensor] = None) -> None:
    """``out`` <- the [N] float32 row values at cutoff ``k`` (``1 <= k <= C``); ``ndcg_sum`` += the
    sum of the unrounded values and ``num_rows`` += N (float64 scalars); bit 0 of ``err`` is set
    when a relevance is negative or NaN (its row scores NaN).  Eager calls take the pybind entry;
    under torch.compile the dispatcher op keeps the call in the graph."""
    if _ops.compiling():
        torch.ops.torcheval_amd.ndcg(input, target, k, exponential_gain, out, ndcg_sum, num_rows, err)
        return
    native().ndcg(input, target, k, exponential_gain, out, ndcg_sum, num_rows, err)
