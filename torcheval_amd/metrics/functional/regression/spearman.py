"""Spearman rank correlation, functional API.

Not in the reference tree (docs/parity.md, "Not in the reference"): Pearson's correlation of the
tie-averaged ranks, evaluated on integers.  ROCm tensors of native dtypes run K14
(csrc/kernels/rankcorr.hip) behind one K3a radix sort of both operands; CPU tensors, float64,
int32 / int64 and bool operands run the ATen form below, which is the definition written with
``torch.sort`` and ``torch.searchsorted``.
"""

import torch

import torcheval_amd.ops as _ops
from torcheval_amd.ops import rankcorr as _k14

__all__ = ["spearman_corrcoef"]


def spearman_corrcoef(
    input: torch.Tensor,
    target: torch.Tensor,
    *,
    num_tasks: int = 1,
) -> torch.Tensor:
    """Spearman's rho of ``input`` against ``target``, per task.

    For an operand ``v`` of ``n`` samples and item ``i``, with ``lo_i`` the number of values below
    ``v_i`` and ``hi_i = lo_i +`` the number equal to it (itself included), the centred doubled
    rank is ``c_i = lo_i + hi_i - n``: ``2 rank_i - (n + 1)`` for the 1-based tie-averaged rank
    (scipy's ``rankdata(method="average")``), an integer.  With ``cx``, ``cy`` the ranks of the two
    operands, ``rho = sum(cx cy) / sqrt(sum(cx^2) sum(cy^2))``, every term formed and summed in
    FP64.  Values compare as floats: ``-0.0 == +0.0``, and ``+-inf`` are ordinary values.  A NaN
    anywhere in a task's operands makes that task NaN; a constant operand or ``n < 2`` gives NaN.
    For ``n <= 2^17`` the three sums are exact, so the value does not depend on the order of the
    samples or of the operands.  Class version: ``SpearmanCorrCoef``.

    Args:
        input: ``[n]``, or ``[num_tasks, n]`` when ``num_tasks > 1``.
        target: the same shape.
        num_tasks: number of independent tasks (rows).

    Returns float32 (float64 when an operand is float64): a scalar for ``num_tasks == 1``, else
    ``[num_tasks]``.
    """
    _spearman_param_check(num_tasks)
    _spearman_update_input_check(input, target, num_tasks)
    if _ops.compiling():
        # no inference mode inside a traced graph: AOT autograd cannot functionalize a view of a
        # graph input (``unsqueeze`` of a 1-D operand, ``t()`` of a transposed one) taken under it
        return _spearman_compute(input, target)
    with torch.inference_mode():
        return _spearman_compute(input, target)


def _spearman_param_check(num_tasks: int) -> None:
    if num_tasks < 1:
        raise ValueError(f"`num_tasks` value should be greater than or equal to 1, but received {num_tasks}. ")


def _spearman_update_input_check(input: torch.Tensor, target: torch.Tensor, num_tasks: int) -> None:
    if input.shape != target.shape:
        raise ValueError(
            "The `input` and `target` should have the same shape, "
            f"got shapes {input.shape} and {target.shape}."
        )
    if num_tasks == 1:
        if len(input.shape) != 1:
            raise ValueError(
                f"`num_tasks = 1`, `input` is expected to be one-dimensional tensor, but got shape ({input.shape})."
            )
    elif len(input.shape) != 2 or input.shape[0] != num_tasks:
        raise ValueError(
            f"`num_tasks = {num_tasks}`, `input`'s shape is expected to be ({num_tasks}, num_samples), but got shape ({input.shape})."
        )


def _spearman_compute(input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """rho of checked ``[n]`` or ``[rows, n]`` operands."""
    if _k14.supported(input, target):
        out = _k14.spearman(input, target)
    else:
        wide = input.dtype == torch.float64 or target.dtype == torch.float64
        out = _spearman_aten(input, target).to(torch.float64 if wide else torch.float32)
    return out[0] if input.dim() == 1 else out


def _centred_ranks(v: torch.Tensor) -> torch.Tensor:
    """``lo + hi - n`` per item of every row of ``[rows, n]``, as float64."""
    if v.dtype in (torch.float16, torch.bfloat16, torch.bool):
        v = v.float()  # exact, and keeps the order and the ties
    v = v.contiguous()
    s = torch.sort(v, dim=-1).values
    lo = torch.searchsorted(s, v, right=False)
    hi = torch.searchsorted(s, v, right=True)
    return (lo + hi - v.shape[-1]).double()


def _spearman_aten(input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """The ATen form, exactly as defined: float64 ``[rows]``.  Each operand is ranked in its own
    dtype, so mixed dtypes need no promotion."""
    x = input if input.dim() == 2 else input.unsqueeze(0)
    y = target if target.dim() == 2 else target.unsqueeze(0)
    cx, cy = _centred_ranks(x), _centred_ranks(y)
    sxy, sxx, syy = (cx * cy).sum(-1), (cx * cx).sum(-1), (cy * cy).sum(-1)
    undefined = x.isnan().any(-1) | y.isnan().any(-1) | (sxx == 0) | (syy == 0)  # n < 2: both sums are 0
    return torch.where(undefined, torch.nan, sxy / torch.sqrt(sxx * syy))
