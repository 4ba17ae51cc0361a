"""Normalized discounted cumulative gain (NDCG), functional API.

Not in the reference tree (docs/parity.md, "Not in the reference"): graded relevance, the
``1 / log2(rank + 2)`` discount, tie-averaged DCG (sklearn's ``ignore_ties=False``).  ROCm tensors
of native dtypes run K13 (csrc/kernels/ndcg.hip, one launch); CPU tensors, float64 / other dtype
combinations and rows wider than the kernel's cap run the ATen form below, which is the
definition written with two sorts and run boundaries, in FP64.
"""

import functools
from typing import Optional, Tuple

import torch

from torcheval_amd.ops import ndcg as _k13
from torcheval_amd.ops.hostread import read_int

__all__ = ["normalized_dcg"]

_BAD_RELEVANCE = "NDCG: `target` holds a negative or NaN relevance; the graded relevance must be >= 0"


@torch.inference_mode()
def normalized_dcg(
    input: torch.Tensor,
    target: torch.Tensor,
    *,
    k: Optional[int] = None,
    exponential_gain: bool = False,
) -> torch.Tensor:
    """NDCG@k of every row of ``[N, C]`` scores against ``[N, C]`` graded relevance.

    With ``K = C`` (``k is None``) or ``min(k, C)``, discounts ``d[r] = 1 / log2(r + 2)`` and their
    prefix sums ``D``, the gain ``target`` (or ``2^target - 1``), and for item ``i`` the counts
    ``g_i`` of strictly larger and ``e_i`` of equal scores (itself included),
    ``DCG = sum_i gain_i (D[min(g_i + e_i, K)] - D[min(g_i, K)]) / e_i``: tied items share the
    discounts of the positions their group occupies.  Scores order descending with
    ``-0.0 == +0.0`` and every NaN equal and above ``+inf``.  ``IDCG`` is the same with the
    relevance as the score; a row's value is ``DCG / IDCG``, and 0 where ``IDCG == 0``.
    Class version: ``NormalizedDCG``.

    Args:
        input: scores ``[N, C]``.
        target: graded relevance ``[N, C]``, ``>= 0``.  On CPU a negative or NaN relevance raises;
            on ROCm its row scores NaN, and the call raises only under ``config.validate``.
        k: the cutoff; ``None`` ranks all ``C`` items.
        exponential_gain: use ``2^target - 1`` instead of ``target``.

    Returns float32 ``[N]``.
    """
    return _normalized_dcg(input, target, k, exponential_gain, None)


def _ndcg_input_check(input: torch.Tensor, target: torch.Tensor, k: Optional[int]) -> None:
    if input.ndim != 2:
        raise ValueError(f"input should be a two-dimensional tensor, got shape {input.shape}.")
    if target.shape != input.shape:
        raise ValueError(
            f"`input` and `target` should have the same shape, got shapes {input.shape} and {target.shape}."
        )
    if k is not None and k <= 0:
        raise ValueError(f"k should be None or positive, got {k}.")


def _raise_on_bad_relevance(err: Optional[torch.Tensor]) -> None:
    """Surface (and clear) the device flag K13 sets for a negative or NaN relevance."""
    if err is not None and read_int(err) != 0:
        err.zero_()
        raise ValueError(_BAD_RELEVANCE + " (such rows scored NaN in an earlier update).")


def _normalized_dcg(input: torch.Tensor, target: torch.Tensor, k: Optional[int], exponential_gain: bool,
                    err: Optional[torch.Tensor]) -> torch.Tensor:
    """``normalized_dcg`` with the class metric's device error flag (``err``, or None for the
    functional's own)."""
    from torcheval_amd.config import config

    _ndcg_input_check(input, target, k)
    n, c = input.shape
    if n == 0 or c == 0:
        return torch.zeros(n, dtype=torch.float32, device=input.device)
    cutoff = c if k is None else min(int(k), c)
    if _k13.supported(input, target):
        own = err is None and config.validate
        if own:
            err = torch.zeros(1, dtype=torch.int32, device=input.device)
        out = torch.empty(n, dtype=torch.float32, device=input.device)
        _k13.ndcg(input, target, cutoff, exponential_gain, out, None, None, err)
        if own:
            _raise_on_bad_relevance(err)
        return out
    values, bad = _ndcg_update(input, target, cutoff, exponential_gain)
    _report_bad_rows(bad, err)
    return values.float()


def _report_bad_rows(bad: torch.Tensor, err: Optional[torch.Tensor]) -> None:
    """The ATen form's side of the K10 contract: CPU raises at the call; a ROCm tensor records
    into ``err`` (class) or raises under ``config.validate`` (functional)."""
    from torcheval_amd.config import config

    if not bad.is_cuda:
        if bool(bad.any()):
            raise ValueError(_BAD_RELEVANCE + ".")
    elif err is not None:
        err.bitwise_or_(bad.any().to(err.dtype))
    elif config.validate and bool(bad.any()):
        raise ValueError(_BAD_RELEVANCE + ".")


@functools.lru_cache(maxsize=64)
def _discount_table(k: int, device: torch.device) -> torch.Tensor:
    """``D[0 .. k]`` in float64 on ``device``: ``D[0] = 0``, ``D[m] = d[0] + ... + d[m - 1]`` with
    ``d[r] = 1 / log2(r + 2)``, summed sequentially on the host.  Cached; never modified."""
    d = 1.0 / torch.log2(torch.arange(k, dtype=torch.float64) + 2.0)
    return torch.cat([torch.zeros(1, dtype=torch.float64), torch.cumsum(d, dim=0)]).to(device)


def _ndcg_update(input: torch.Tensor, target: torch.Tensor, cutoff: int,
                 exponential_gain: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """The ATen form, exactly as defined, in FP64: (row values ``[N]`` float64, ``[N]`` bool mask
    of rows holding a negative or NaN relevance, which score NaN).  ``1 <= cutoff <= C``.

    Two sorts and run boundaries, no ``[N, C, C]`` tensor: the gains are sorted descending (which
    is also the ideal order), then the scores stably on top of that order, so the sequence of
    (score, gain) pairs, and with it every sum, does not depend on the column order."""
    n, c = input.shape
    scores = input if input.is_floating_point() else input.double()
    t = target.double()
    bad = ~(t >= 0)
    gain = torch.exp2(t) - 1.0 if exponential_gain else t
    gain = torch.where(gain > 0, gain, 0.0)  # also clears -0.0 and the rows that are bad anyway
    table = _discount_table(cutoff, input.device)
    ideal, by_gain = torch.sort(gain, dim=1, descending=True)
    idcg = (ideal[:, :cutoff] * (table[1:] - table[:-1])).sum(dim=1)
    s, by_score = torch.sort(scores.gather(1, by_gain), dim=1, descending=True, stable=True)  # NaNs first
    g = ideal.gather(1, by_score)
    same = (s[:, 1:] == s[:, :-1]) | (s[:, 1:].isnan() & s[:, :-1].isnan())  # -0.0 == +0.0; NaNs tie
    edge = torch.ones(n, 1, dtype=torch.bool, device=input.device)
    pos = torch.arange(c, device=input.device).expand(n, c)
    start = torch.cummax(torch.where(torch.cat([edge, ~same], dim=1), pos, 0), dim=1).values
    last = torch.where(torch.cat([~same, edge], dim=1), pos + 1, c)
    end = torch.cummin(last.flip(1), dim=1).values.flip(1)
    share = (table[end.clamp(max=cutoff)] - table[start.clamp(max=cutoff)]) / (end - start)
    dcg = (g * share).sum(dim=1)
    values = torch.where(idcg == 0, 0.0, dcg / idcg)
    bad_row = bad.any(dim=1)
    return torch.where(bad_row, torch.nan, values), bad_row
