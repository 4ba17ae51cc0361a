"""Inception Score (Salimans et al. 2016), functional API.

Not in the reference tree (docs/parity.md, "Not in the reference").  The score is written as
sufficient statistics: per split the column sums of the rows' softmax probabilities, the sum of
the rows' negative entropies and the number of rows, so nothing of size ``N`` is kept.  ROCm
float32 / float16 / bfloat16 logits of up to 2048 columns and up to 64 splits run K21
(csrc/kernels/inception_score.hip), which reads the logits once; CPU tensors, float64, wider rows,
more splits and other strides run the ATen form below, which is the definition.
"""

import math
from typing import Tuple

import torch

import torcheval_amd.ops as _ops
from torcheval_amd.ops import inception_score as _k21

__all__ = ["inception_score"]


def inception_score(logits: torch.Tensor, *, splits: int = 10) -> Tuple[torch.Tensor, torch.Tensor]:
    """Inception Score of ``[N, C]`` class logits (or log-probabilities, which are logits whose
    softmax is themselves): ``(mean, std)`` over ``splits`` splits of ``exp(mean_i KL(p_i || q))``,
    ``p_i = softmax(logits_i)`` and ``q`` the mean of the split's ``p_i``.

    Row ``i`` belongs to split ``i mod splits``.  This interleaved partition does not depend on the
    content, as the shuffle-then-chunk of torchmetrics does not, and input that arrives ordered by
    class is spread over all splits; values agree with torchmetrics in distribution, not bit for
    bit.  The standard deviation is the population form (``unbiased=False``, as the paper's code);
    torchmetrics' sample form is larger by ``sqrt(S / (S - 1))``.  Splits without rows are left
    out; with one split that has rows the deviation is 0, with none both results are NaN.

    ``-inf`` is a masked class of probability 0.  A NaN or ``+inf`` logit or a row that is all
    ``-inf`` makes its split, and thereby both results, NaN; there is no error flag.  Class version:
    ``InceptionScore``.

    Returns float32 scalars on the logits' device, float64 for float64 logits.
    """
    _is_param_check(splits)
    _is_input_check(logits)
    if _ops.compiling():
        # no inference mode inside a traced graph (as kernel_inception_distance)
        return _is_compute(logits, splits)
    with torch.inference_mode():
        return _is_compute(logits, splits)


def _is_param_check(splits: int) -> None:
    if not isinstance(splits, int) or isinstance(splits, bool) or splits < 1:
        raise ValueError(f"`splits` should be an integer greater than or equal to 1, but received {splits}.")


def _is_input_check(logits: torch.Tensor) -> None:
    if logits.dim() != 2:
        raise ValueError(f"`logits` should be two-dimensional, `[N, C]`, got shape {tuple(logits.shape)}.")
    if not logits.is_floating_point():
        raise ValueError(f"`logits` should be a floating-point tensor, got {logits.dtype}.")
    if logits.shape[1] == 0 and logits.shape[0] > 0:
        raise ValueError("`logits` should have at least one column (`C >= 1`) when it has rows.")


def _result_dtype(logits: torch.Tensor) -> torch.dtype:
    return torch.float64 if logits.dtype == torch.float64 else torch.float32


def _is_compute(logits: torch.Tensor, splits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean, std) of checked logits."""
    dtype = _result_dtype(logits)
    if logits.shape[0] == 0:
        nan = torch.full((), math.nan, dtype=dtype, device=logits.device)
        return nan, nan.clone()
    _, mean, std = _inception_score_values(*_inception_score_stats(logits, splits), dtype=dtype)
    return mean, std


def _zero_states(splits: int, c: int, device: torch.device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return (torch.zeros(splits, c, dtype=torch.float64, device=device),
            torch.zeros(splits, dtype=torch.float64, device=device),
            torch.zeros(splits, dtype=torch.float64, device=device))


def _inception_score_stats(logits: torch.Tensor, splits: int,
                           first_split: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """float64 ``(prob_sum [S, C], neg_entropy_sum [S], num_rows [S])`` of ``[N, C]`` logits whose
    row ``i`` belongs to split ``(first_split + i) mod S``, from whichever path the tensor takes."""
    states = _zero_states(splits, logits.shape[1], logits.device)
    _stats_add(logits, first_split % splits, *states)
    return states


def _stats_add(logits: torch.Tensor, first_split: int, prob_sum: torch.Tensor, neg_entropy_sum: torch.Tensor,
               num_rows: torch.Tensor) -> None:
    """The three states, on the logits' device, += the statistics of the rows."""
    if logits.shape[0] == 0:
        return
    if _k21.supported(logits, prob_sum, neg_entropy_sum, num_rows):
        _k21.inception_update(logits, first_split, prob_sum, neg_entropy_sum, num_rows)
    else:
        _stats_add_aten(logits, first_split, prob_sum, neg_entropy_sum, num_rows)


def _stats_add_aten(logits: torch.Tensor, first_split: int, prob_sum: torch.Tensor, neg_entropy_sum: torch.Tensor,
                    num_rows: torch.Tensor) -> None:
    """The ATen form, exactly as defined: ``softmax`` and ``log_softmax`` in float32 (FP64 for
    float64 logits), widened to FP64, and three ``index_add_`` s."""
    x = logits.to(_result_dtype(logits))
    p = torch.softmax(x, dim=-1).double()  # NaN for a row with NaN or +inf, and for one that is all -inf
    lp = torch.log_softmax(x, dim=-1).double()
    h = torch.where(x == -math.inf, 0.0, p * lp).sum(dim=-1)  # a masked class: p = 0, term 0
    h = torch.where(p.isnan().any(dim=-1), math.nan, h)
    splits = prob_sum.shape[0]
    split = (torch.arange(x.shape[0], device=x.device) + first_split) % splits
    prob_sum.index_add_(0, split, p)
    neg_entropy_sum.index_add_(0, split, h)
    num_rows.index_add_(0, split, torch.ones_like(h))


def _inception_score_values(prob_sum: torch.Tensor, neg_entropy_sum: torch.Tensor, num_rows: torch.Tensor,
                            dtype: torch.dtype = torch.float32) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(split_log, mean, std)`` of the three states: float64 ``[S]`` log scores (NaN for a split
    without rows), and the mean and population standard deviation of their exponentials over the
    splits with rows as ``dtype`` scalars, from whichever path the states take."""
    if dtype == torch.float32 and _k21.value_supported(prob_sum, neg_entropy_sum, num_rows):
        split_log, out = _k21.inception_value(prob_sum, neg_entropy_sum, num_rows)
        return split_log, out[0], out[1]
    have = num_rows > 0
    q = prob_sum / num_rows[:, None]
    cross = torch.where(q == 0, 0.0, q * q.log()).sum(dim=1)
    split_log = torch.where(have, neg_entropy_sum / num_rows - cross, math.nan)
    value = split_log.exp()
    count = have.sum()
    mean = torch.where(have, value, 0.0).sum() / count  # no split with rows: 0 / 0
    dev = torch.where(have, value - mean, 0.0)
    std = ((dev * dev).sum() / count).sqrt()
    return split_log, mean.to(dtype), std.to(dtype)
