"""K14 wrapper (csrc/kernels/rankcorr.hip): Spearman's rho per row of [rows, n] operand pairs.

Per call: both operands packed into one ``[2 rows, n]`` float32 buffer, one K3a radix sort of it
(descending, the int32 source permutation as its order), then one ``rank_corr`` op of three
launches: ``rank_center`` (tie runs of the sorted rows -> centred doubled ranks, scattered back to
source order), ``rank_moments`` (FP64 partials of the three co-moments) and ``rank_finish``
(float32 rho per row, NaN rules applied).  No host synchronisation anywhere.  Native inputs are
float32 / float16 / bfloat16 and int8 / uint8 / int16, all exact in float32, with any strides;
everything else is the caller's ATen form.
"""

import torch

import torcheval_amd.ops as _ops
from torcheval_amd.ops import native, use_native

_DTYPES = (torch.float32, torch.float16, torch.bfloat16, torch.int8, torch.uint8, torch.int16)

# kRankCenterSpan / kRankMomentsSpan of csrc/include/tea_kernels.h (held equal by
# tests/metrics/regression/test_spearman.py): the spans at whose edges the GPU tests place their shapes
CENTER_SPAN = 2048
MOMENTS_SPAN = 4096


def supported(input: torch.Tensor, target: torch.Tensor) -> bool:
    """Whether the pair runs K14: ROCm tensors of native dtypes on one device, equal ``[n]`` or
    ``[rows, n]`` shapes, ``rows >= 1`` and ``2 <= n < 2^31``.  Raises on a GPU without the
    extension (``use_native``)."""
    if not use_native(input) or target.device != input.device:
        return False
    if input.dtype not in _DTYPES or target.dtype not in _DTYPES:
        return False
    if input.dim() not in (1, 2) or target.shape != input.shape or input.shape[0] == 0:
        return False
    return 2 <= input.shape[-1] < 2**31


def _pack(dst: torch.Tensor, v: torch.Tensor) -> None:
    """``dst`` (contiguous float32 rows) <- the values of ``v``, converted and packed in one pass.
    The transposed view of a row-major ``[n, rows]`` float32 tensor goes through the LDS-tiled
    ``transpose_f32`` (ATen's strided copy of such a view is ~10x slower)."""
    if v.dim() == 2 and v.dtype == torch.float32 and v.stride(-1) != 1 and v.stride(0) == 1 and v.t().is_contiguous():
        if _ops.compiling():
            torch.ops.torcheval_amd.transpose_f32(v.t(), dst)
        else:
            native().transpose_f32(v.t(), dst)
    else:
        dst.copy_(v)


def spearman(input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Float32 ``[rows]`` rho of a ``supported`` pair.  Both operands are packed into one
    ``[2 rows, n]`` float32 buffer and sorted by one K3a call: measured against one call per
    operand it is 1.2 - 1.3x faster end to end at every shape class, the two copies included
    (profiles/spearman_r10.json), so that arm is gone.  The sort takes its pybind entry in eager
    calls and its dispatcher op under torch.compile; ``rank_corr`` is a dispatcher op only
    (``torch.ops.torcheval_amd_rankcorr``), so the call stays in a compiled graph."""
    x = input if input.dim() == 2 else input.unsqueeze(0)
    y = target if target.dim() == 2 else target.unsqueeze(0)
    rows, n = x.shape
    both = torch.empty(2 * rows, n, dtype=torch.float32, device=x.device)
    _pack(both[:rows], x)
    _pack(both[rows:], y)
    s = torch.empty_like(both)
    order = torch.empty(both.shape, dtype=torch.int32, device=x.device)
    out = torch.empty(rows, dtype=torch.float32, device=x.device)
    if _ops.compiling():
        torch.ops.torcheval_amd.sort_desc(both, s, order, None, 0, False)
    else:
        native().sort_desc(both, s, order, None, 0)
    torch.ops.torcheval_amd_rankcorr.rank_corr(s, order, out)
    return out
