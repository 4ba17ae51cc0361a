"""Kendall rank correlation (tau-b / tau-c), functional API.

Not in the reference tree (docs/parity.md, "Not in the reference"): a ratio of exact 64-bit
integers, the numbers of tied and of discordant pairs.  ROCm tensors of native dtypes run K19
(csrc/kernels/kendall.hip) behind two K3a radix sorts; CPU tensors, float64, int32 / int64 and bool
operands run the ATen form below, which evaluates the same integers with ``torch.sort``, run
boundaries and a bottom-up loop of ``torch.searchsorted``.
"""

import torch

import torcheval_amd.ops as _ops
from torcheval_amd.ops import kendall as _k19

__all__ = ["kendall_rank_corrcoef"]

_VARIANTS = ("b", "c")


def kendall_rank_corrcoef(
    input: torch.Tensor,
    target: torch.Tensor,
    *,
    num_tasks: int = 1,
    variant: str = "b",
) -> torch.Tensor:
    """Kendall's tau of ``input`` against ``target``, per task (``scipy.stats.kendalltau`` without
    its p-value).

    For ``n`` samples let ``n0 = n (n - 1) / 2``, ``n1 = sum t (t - 1) / 2`` over the tie groups of
    ``input``, ``n2`` the same for ``target``, ``n3`` the same over the groups tied in both, ``Q``
    the number of discordant pairs and ``mx``, ``my`` the numbers of distinct values; all are kept
    in int64.  ``S = n0 - n1 - n2 + n3 - 2 Q`` is the number of concordant minus discordant pairs
    and ``tau_b = S / (sqrt(n0 - n1) sqrt(n0 - n2))``,
    ``tau_c = 2 S / (n^2 (m - 1) / m)`` with ``m = min(mx, my)``, each evaluated once in FP64.
    Values compare as floats: ``-0.0 == +0.0``, and ``+-inf`` are ordinary values.  A NaN anywhere
    in a task's operands makes that task NaN; a constant operand or ``n < 2`` gives NaN (both
    variants, without a warning).  The integers do not depend on the order of the samples, so the
    value is bit-identical under any permutation of them, and tau-b under a swap of the operands.
    Class version: ``KendallRankCorrCoef``.

    Args:
        input: ``[n]``, or ``[num_tasks, n]`` when ``num_tasks > 1``.
        target: the same shape.
        num_tasks: number of independent tasks (rows).
        variant: ``"b"`` or ``"c"``.

    Returns float32 (float64 when an operand is float64): a scalar for ``num_tasks == 1``, else
    ``[num_tasks]``.
    """
    _kendall_param_check(num_tasks, variant)
    _kendall_update_input_check(input, target, num_tasks)
    if _ops.compiling():
        # no inference mode inside a traced graph (as spearman_corrcoef)
        return _kendall_compute(input, target, variant)
    with torch.inference_mode():
        return _kendall_compute(input, target, variant)


def _kendall_param_check(num_tasks: int, variant: str) -> None:
    if num_tasks < 1:
        raise ValueError(f"`num_tasks` value should be greater than or equal to 1, but received {num_tasks}. ")
    if variant not in _VARIANTS:
        raise ValueError(f"`variant` should be one of {_VARIANTS}, but received {variant!r}.")


def _kendall_update_input_check(input: torch.Tensor, target: torch.Tensor, num_tasks: int) -> None:
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


def _kendall_compute(input: torch.Tensor, target: torch.Tensor, variant: str) -> torch.Tensor:
    """tau of checked ``[n]`` or ``[rows, n]`` operands."""
    if _k19.supported(input, target):
        out = _k19.kendall(input, target, variant == "c")[0]
    else:
        wide = input.dtype == torch.float64 or target.dtype == torch.float64
        out = _kendall_aten(input, target, variant).to(torch.float64 if wide else torch.float32)
    return out[0] if input.dim() == 1 else out


def _kendall_counts(input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """int64 ``[tasks, 6]``: ``(n1, n2, n3, Q, mx, my)`` per task of ``[n]`` or ``[tasks, n]``
    operands, from whichever path the tensors take; -1 six times for a task that holds a NaN."""
    with torch.inference_mode():
        if _k19.supported(input, target):
            return _k19.kendall(input, target, False)[1]
        return _kendall_counts_aten(input, target)


def _run_starts(new: torch.Tensor) -> torch.Tensor:
    """For ``new`` ``[rows, n]`` (position k starts a run), the start of each position's run."""
    idx = torch.arange(new.shape[-1], device=new.device).expand_as(new)
    return torch.cummax(torch.where(new, idx, 0), dim=-1).values


def _starts_flag(differs: torch.Tensor) -> torch.Tensor:
    """``[rows, n]`` run-start flags from ``differs[:, k] = item k + 1 differs from item k``."""
    first = torch.ones(differs.shape[0], 1, dtype=torch.bool, device=differs.device)
    return torch.cat([first, differs], dim=-1)


def _inversions(seq: torch.Tensor) -> torch.Tensor:
    """Strict inversions (``i < j``, ``seq_i > seq_j``) per row of int64 ``[rows, n]``, bottom-up:
    at run length L the row is viewed as ``[pairs, 2, L]`` (padded with the maximum, which sits at
    the end and adds nothing), every real element of a right run adds the number of larger elements
    of its left run, and each ``2 L`` run is re-sorted."""
    rows, n = seq.shape
    width = 1 << max(n - 1, 0).bit_length()
    big = torch.iinfo(torch.int64).max
    a = torch.full((rows, width), big, dtype=torch.int64, device=seq.device)
    a[:, :n] = seq
    q = torch.zeros(rows, dtype=torch.int64, device=seq.device)
    run = 1
    while run < width:
        v = a.view(rows, width // (2 * run), 2, run)
        left, right = v[:, :, 0, :].contiguous(), v[:, :, 1, :].contiguous()
        larger = run - torch.searchsorted(left, right, right=True)
        q += torch.where(right != big, larger, 0).sum(dim=(-1, -2))
        a = v.reshape(rows, width // (2 * run), 2 * run).sort(dim=-1).values.reshape(rows, width)
        run *= 2
    return q


def _comparable(v: torch.Tensor) -> torch.Tensor:
    if v.dtype in (torch.float16, torch.bfloat16, torch.bool):
        v = v.float()  # exact, and keeps the order and the ties
    return v.contiguous()


def _kendall_counts_aten(input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """The counting identity in ATen.  Sort ``target`` descending and stable and let ``s`` be the
    position at which an item's tie run starts; take ``input`` in that order and sort it descending
    and stable, carrying ``s``.  Inside an ``input`` tie group ``s`` is then non-decreasing, ``Q`` is
    the number of strict inversions of the carried sequence, and ``n3`` comes from the (contiguous)
    runs on which the sorted ``input`` and ``s`` are both equal.  Each operand is ranked in its own
    dtype, so mixed dtypes need no promotion."""
    x = _comparable(input if input.dim() == 2 else input.unsqueeze(0))
    y = _comparable(target if target.dim() == 2 else target.unsqueeze(0))
    rows, n = x.shape
    if n < 2:
        return torch.zeros(rows, 6, dtype=torch.int64, device=x.device)
    pos = torch.arange(n, device=x.device)
    ys, perm = torch.sort(y, dim=-1, descending=True, stable=True)
    new_y = _starts_flag(ys[:, 1:] != ys[:, :-1])
    s = _run_starts(new_y)
    n2, my = (pos - s).sum(-1), new_y.sum(-1)
    xs, perm2 = torch.sort(x.gather(-1, perm), dim=-1, descending=True, stable=True)
    carried = s.gather(-1, perm2)
    differs_x = xs[:, 1:] != xs[:, :-1]
    new_x = _starts_flag(differs_x)
    n1, mx = (pos - _run_starts(new_x)).sum(-1), new_x.sum(-1)
    new_joint = _starts_flag(differs_x | (carried[:, 1:] != carried[:, :-1]))
    n3 = (pos - _run_starts(new_joint)).sum(-1)
    counts = torch.stack([n1, n2, n3, _inversions(carried), mx, my], dim=-1)
    nan = x.isnan().any(-1) | y.isnan().any(-1)
    return torch.where(nan.unsqueeze(-1), -1, counts)


def _kendall_aten(input: torch.Tensor, target: torch.Tensor, variant: str) -> torch.Tensor:
    """The ATen form: float64 ``[rows]`` from the integer counts."""
    n = input.shape[-1]
    counts = _kendall_counts_aten(input, target)
    n1, n2, n3, q, mx, my = counts.unbind(-1)
    n0 = n * (n - 1) // 2
    s = (n0 - n1 - n2 + n3 - 2 * q).double()
    if variant == "b":
        tau = s / (torch.sqrt((n0 - n1).double()) * torch.sqrt((n0 - n2).double()))
    else:
        m = torch.minimum(mx, my).double()
        tau = (2.0 * s) / (float(n) * float(n) * ((m - 1.0) / m))
    undefined = (n1 < 0) | (n1 == n0) | (n2 == n0)  # a NaN in the task; a constant operand; n < 2: n0 = n1 = 0
    return torch.where(undefined, torch.nan, tau)
