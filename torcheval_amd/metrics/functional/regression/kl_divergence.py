"""KL divergence between two score tensors, functional API.

Not in the reference tree (docs/parity.md, "Not in the reference").  The value of a row is
``KL(P || Q) = sum_j p_j (log p_j - log q_j)`` with ``P`` from ``target`` and ``Q`` from ``input``,
the direction of ``F.kl_div(log q, p)``.  Two ROCm tensors of one dtype (float32 / float16 /
bfloat16) run K18 (csrc/kernels/kl_divergence.hip), which reads both operands once; CPU tensors,
float64, mixed dtypes and layouts K18 does not take run the ATen form below, which is the
definition.
"""

import math
from typing import Optional, Tuple

import torch

import torcheval_amd.ops as _ops
from torcheval_amd.ops import kl_divergence as _k18

__all__ = ["kl_divergence"]

_REDUCTIONS = ("none", "sum", "mean")


def kl_divergence(
    input: torch.Tensor,
    target: torch.Tensor,
    *,
    from_logits: bool = True,
    mask: Optional[torch.Tensor] = None,
    reduction: str = "mean",
) -> torch.Tensor:
    """KL divergence ``KL(P || Q)`` of every row of ``target`` (``P``: teacher, reference model)
    from the same row of ``input`` (``Q``: student, policy), reduced over the counted rows.

    ``from_logits=True``: ``p = softmax(target)``, ``q = softmax(input)``.  Log-probabilities are
    logits whose softmax is themselves, so this mode takes them as they are.  ``-inf`` is a masked
    entry of probability 0: a term with ``target_j == -inf`` is 0 whatever ``input_j`` is,
    ``input_j == -inf`` under ``p_j > 0`` makes the row ``+inf``, a NaN or ``+inf`` in either
    operand makes the row NaN, and so does a row that is all ``-inf`` in either operand.

    ``from_logits=False``: both operands are non-negative weights, ``p = t / sum(t)`` and
    ``q = x / sum(x)``.  A term with ``t_j == 0`` is 0, ``t_j > 0`` with ``x_j == 0`` makes the row
    ``+inf``, and a negative, NaN or ``+inf`` entry anywhere in the row or a zero sum makes it NaN.

    There is no error flag: a NaN or ``inf`` row makes a reduced value NaN or ``inf``.  Class
    version: ``KLDivergence``.

    Args:
        input: ``[..., C]`` floating-point scores of the prediction.
        target: the same shape; the distribution ``input`` is held against.
        from_logits: see above.
        mask: optional bool ``[...]``; a row whose mask is ``False`` is not read and not counted.
        reduction: ``"none"`` (the row values in shape ``[...]``, ``0.0`` for uncounted rows),
            ``"sum"`` or ``"mean"`` over the counted rows (NaN when there are none); the sum and
            the count are formed in FP64.

    Returns float32, or float64 when an operand is float64.
    """
    _kl_param_check(reduction)
    _kl_input_check(input, target, mask)
    if _ops.compiling():
        # no inference mode inside a traced graph (as pearson_corrcoef)
        return _kl_compute(input, target, from_logits, mask, reduction)
    with torch.inference_mode():
        return _kl_compute(input, target, from_logits, mask, reduction)


def _kl_param_check(reduction: str) -> None:
    if reduction not in _REDUCTIONS:
        raise ValueError(f"`reduction` should be one of {_REDUCTIONS}, got {reduction!r}.")


def _kl_input_check(input: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor]) -> None:
    if input.shape != target.shape:
        raise ValueError(
            f"The `input` and `target` should have the same shape, got shapes {input.shape} and {target.shape}."
        )
    if input.dim() < 1:
        raise ValueError("`input` should have at least one dimension, `[..., C]`, got a scalar.")
    if not (input.is_floating_point() and target.is_floating_point()):
        raise ValueError(
            f"`input` and `target` should be floating-point tensors, got {input.dtype} and {target.dtype}."
        )
    if input.shape[-1] == 0 and input.shape[:-1].numel() > 0:
        raise ValueError("`input` should have at least one column (`C >= 1`) when it has rows.")
    if mask is not None and (mask.dtype != torch.bool or mask.shape != input.shape[:-1]):
        raise ValueError(
            f"`mask` should be a bool tensor of shape {tuple(input.shape[:-1])}, "
            f"got {mask.dtype} of shape {tuple(mask.shape)}."
        )


def _result_dtype(input: torch.Tensor, target: torch.Tensor) -> torch.dtype:
    wide = input.dtype == torch.float64 or target.dtype == torch.float64
    return torch.float64 if wide else torch.float32


def _kl_compute(input: torch.Tensor, target: torch.Tensor, from_logits: bool, mask: Optional[torch.Tensor],
                reduction: str) -> torch.Tensor:
    """The result of checked operands."""
    if input.numel() > 0 and _k18.supported(input, target, mask):
        return _k18.kl_batch(input, target, mask, from_logits, reduction)
    rows = _kl_rows(input, target, from_logits, mask)
    if reduction == "none":
        return rows
    total, count = _kl_sums(rows, mask)
    return (total / count if reduction == "mean" else total).to(rows.dtype)


def _kl_rows(input: torch.Tensor, target: torch.Tensor, from_logits: bool,
             mask: Optional[torch.Tensor]) -> torch.Tensor:
    """The ATen form of the row values, exactly as defined: ``[...]`` in the result dtype, 0 for
    uncounted rows."""
    dt = _result_dtype(input, target)
    x, t = input.to(dt), target.to(dt)
    if from_logits:
        off = t == -math.inf
        lp, lq = torch.log_softmax(t, dim=-1), torch.log_softmax(x, dim=-1)
        term = lp.exp() * (lp - lq)
        term = torch.where(lq == -math.inf, math.inf, term)  # q_j = 0 under p_j > 0, also where p_j underflowed
        rows = torch.where(off, 0.0, term).sum(dim=-1)  # p_j = 0: no term, never -inf - -inf
        rows = torch.where(off.all(dim=-1), math.nan, rows)  # an all -inf input row is NaN by the arithmetic
    else:
        bad = ((t < 0) | (x < 0) | ~torch.isfinite(t) | ~torch.isfinite(x)).any(dim=-1)
        st, sx = t.sum(dim=-1, keepdim=True), x.sum(dim=-1, keepdim=True)
        p, q = t / st, x / sx
        term = torch.where(t > 0, p * (p.log() - q.log()), 0.0)
        rows = torch.where(bad | (st[..., 0] == 0) | (sx[..., 0] == 0), math.nan, term.sum(dim=-1))
    if mask is not None:
        rows = torch.where(mask, rows, 0.0)
    return rows


def _kl_sums(rows: torch.Tensor, mask: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """FP64 (sum of the counted rows' values, their number) of ``_kl_rows``' result."""
    total = rows.double().sum()
    if mask is None:
        return total, torch.full_like(total, float(rows.numel()))
    return total, mask.sum().double()
