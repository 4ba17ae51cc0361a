"""Pearson and Lin's concordance correlation, functional API.

Not in the reference tree (docs/parity.md, "Not in the reference").  Both are value formulas on six
FP64 moments per task (``n, mean_x, mean_y, m2_x, m2_y, c_xy``), which a batch forms from five sums
of differences to its first sample and which merge by the pairwise update, so the class version is
a streaming metric.  ROCm tensors of float32 / float16 / bfloat16 run K16
(csrc/kernels/corrcoef.hip); CPU tensors, float64, integer and bool operands and layouts K16 does
not take run the ATen form below, which is the definition written in FP64.
"""

import torch

import torcheval_amd.ops as _ops
from torcheval_amd.ops import corrcoef as _k16

__all__ = ["pearson_corrcoef", "concordance_corrcoef"]


def pearson_corrcoef(
    input: torch.Tensor,
    target: torch.Tensor,
    *,
    num_tasks: int = 1,
) -> torch.Tensor:
    """Pearson's r of ``input`` against ``target``, per task.

    Every sample is widened to FP64 and taken against the pivot ``(p_x, p_y)``, the task's first
    sample: with ``d_x = x - p_x``, ``d_y = y - p_y`` and the sums ``S_x, S_y, S_xx, S_yy, S_xy``
    of ``d_x, d_y, d_x^2, d_y^2, d_x d_y``, the moments are ``mean = p + S / n``,
    ``m2_x = max(S_xx - S_x^2 / n, 0)`` (``m2_y`` likewise) and ``c_xy = S_xy - S_x S_y / n``, and
    ``r = clamp(c_xy / sqrt(m2_x m2_y), -1, 1)``.  The cancellation is governed by the pivot's
    distance from the mean in standard deviations, not by the mean's.  A constant operand gives
    ``m2 == 0`` exactly and NaN, as does ``n < 2``; a NaN or an infinity anywhere in a task makes
    that task NaN.  Class version: ``PearsonCorrCoef``.

    Args:
        input: ``[n]``, or ``[num_tasks, n]`` when ``num_tasks > 1``.
        target: the same shape.
        num_tasks: number of independent tasks (rows).

    Returns float32 (float64 when an operand is float64): a scalar for ``num_tasks == 1``, else
    ``[num_tasks]``.
    """
    return _corrcoef(input, target, num_tasks, "pearson")


def concordance_corrcoef(
    input: torch.Tensor,
    target: torch.Tensor,
    *,
    num_tasks: int = 1,
) -> torch.Tensor:
    """Lin's concordance correlation of ``input`` against ``target``, per task:
    ``2 c_xy / (m2_x + m2_y + n (mean_x - mean_y)^2)`` on the moments of ``pearson_corrcoef``; NaN
    for ``n < 2``, for a zero denominator (both operands one and the same constant) and for a task
    with a NaN or an infinity.  Arguments and result as ``pearson_corrcoef``.  Class version:
    ``ConcordanceCorrCoef``."""
    return _corrcoef(input, target, num_tasks, "concordance")


def _corrcoef(input: torch.Tensor, target: torch.Tensor, num_tasks: int, kind: str) -> torch.Tensor:
    _pearson_param_check(num_tasks)
    _pearson_update_input_check(input, target, num_tasks)
    if _ops.compiling():
        # no inference mode inside a traced graph (as spearman_corrcoef)
        return _corrcoef_compute(input, target, kind)
    with torch.inference_mode():
        return _corrcoef_compute(input, target, kind)


def _pearson_param_check(num_tasks: int) -> None:
    if num_tasks < 1:
        raise ValueError(f"`num_tasks` value should be greater than or equal to 1, but received {num_tasks}. ")


def _pearson_update_input_check(input: torch.Tensor, target: torch.Tensor, num_tasks: int) -> None:
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


def _corrcoef_compute(input: torch.Tensor, target: torch.Tensor, kind: str) -> torch.Tensor:
    """The value of checked ``[n]`` or ``[tasks, n]`` operands."""
    if _k16.supported(input, target):
        out = _k16.corrcoef_batch(input, target, kind)
    else:
        wide = input.dtype == torch.float64 or target.dtype == torch.float64
        out = _moments_value(_batch_moments(input, target), kind).to(torch.float64 if wide else torch.float32)
    return out[0] if input.dim() == 1 else out


def _batch_moments(input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """The ATen form of one batch's moments, exactly as defined: float64 ``[6, tasks]`` (all zeros
    for ``n == 0``)."""
    x = (input if input.dim() == 2 else input.unsqueeze(0)).double()
    y = (target if target.dim() == 2 else target.unsqueeze(0)).double()
    tasks, n = x.shape
    if n == 0:
        return torch.zeros(6, tasks, dtype=torch.float64, device=x.device)
    px, py = x[:, :1], y[:, :1]
    dx, dy = x - px, y - py
    sx, sy = dx.sum(-1), dy.sum(-1)
    sxx, syy, sxy = (dx * dx).sum(-1), (dy * dy).sum(-1), (dx * dy).sum(-1)
    m2x, m2y = sxx - sx * sx / n, syy - sy * sy / n
    zero = torch.zeros_like(m2x)
    return torch.stack([
        torch.full_like(sx, float(n)),
        px[:, 0] + sx / n,
        py[:, 0] + sy / n,
        torch.where(m2x < 0, zero, m2x),  # a negative rounding residue becomes 0; a NaN stays
        torch.where(m2y < 0, zero, m2y),
        sxy - sx * sy / n,
    ])


def _moments_merge(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The pairwise (Chan et al.) merge of two float64 ``[6, tasks]`` states; a side with
    ``n == 0`` contributes nothing and the other is taken as it is."""
    na, nb = a[0], b[0]
    n = na + nb
    safe = torch.where(n == 0, torch.ones_like(n), n)
    d = b[1:3] - a[1:3]
    wb, wab = nb / safe, na * nb / safe
    merged = torch.cat([
        n.unsqueeze(0),
        a[1:3] + d * wb,
        a[3:5] + b[3:5] + d * d * wab,
        (a[5] + b[5] + d[0] * d[1] * wab).unsqueeze(0),
    ])
    return torch.where(nb == 0, a, torch.where(na == 0, b, merged))


def _moments_value(moments: torch.Tensor, kind: str) -> torch.Tensor:
    """Float64 ``[tasks]`` value of a float64 ``[6, tasks]`` state."""
    n, mx, my, m2x, m2y, c = moments.unbind(0)
    if kind == "concordance":
        num, den = 2.0 * c, m2x + m2y + n * (mx - my) ** 2
    else:
        num, den = c, torch.sqrt(m2x * m2y)
    r = num / den
    if kind != "concordance":
        r = r.clamp(-1.0, 1.0)  # keeps NaN
    return torch.where((n < 2) | (den == 0), torch.nan, r)
