"""Token LCS length and ROUGE-L, functional API.

Not in the reference tree (docs/parity.md, "Not in the reference", has the definition).  Like
``token_edit_distance`` these take what an evaluation loop already holds on the device: padded integer
id rows with a length per row.  ROCm tensors run K30 (csrc/kernels/lcs.hip): a wave per pair updates a
table row as a bit vector, one AND, one addition and one OR per stream token; exact integers, no host
synchronisation outside ``config.validate``.  CPU tensors, non-contiguous rows and widths above
``ops.lcs.MAX_LEN`` run the ATen form below: one batched row recurrence per stream position, whose left
dependency a ``cummax`` resolves.
"""

from typing import Optional, Tuple

import torch

from torcheval_amd.metrics.functional.text.token_edit_distance import Lengths, _rows, _token_check
from torcheval_amd.ops import lcs as _k30

__all__ = ["token_lcs_length", "token_rouge_l"]

MEASURES = ("precision", "recall", "fmeasure")
Totals = Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]


@torch.inference_mode()
def token_lcs_length(input: torch.Tensor, target: torch.Tensor, input_lengths: Lengths = None,
                     target_lengths: Lengths = None, *, ignore_index: Optional[int] = None) -> torch.Tensor:
    """Length of the longest common subsequence of the token-id rows of ``input`` and ``target``.

    Rows, lengths and ``ignore_index`` are those of ``token_edit_distance``: row ``b`` of a side is its
    first ``lengths[b]`` entries (the whole row without lengths) without the entries equal to
    ``ignore_index``, and tokens compare as integers at full width.

    Args:
        input: integer ``[B, Li]`` predicted ids (a 1-D tensor is one pair).
        target: integer ``[B, Lt]`` reference ids; the two widths may differ.
        input_lengths: integer ``[B]``, or None.  Lengths outside ``[0, width]`` raise ``ValueError``
            under ``config.validate`` (one host read) and are clamped to it otherwise.
        target_lengths: likewise.
        ignore_index: the id to remove from both sides, or None.

    Returns the ``[B]`` int64 lengths.
    """
    x, t, il, tl = _token_check(input, target, input_lengths, target_lengths, ignore_index)
    return _lcs_update(x, t, il, tl, ignore_index)[0]


@torch.inference_mode()
def token_rouge_l(input: torch.Tensor, target: torch.Tensor, input_lengths: Lengths = None,
                  target_lengths: Lengths = None, *, ignore_index: Optional[int] = None,
                  measure: str = "fmeasure") -> torch.Tensor:
    """ROUGE-L over the token-id pairs of one batch; see ``token_lcs_length`` for the rows.

    Per pair, with ``lcs`` its LCS length: precision ``P = lcs / len(input)``, recall
    ``R = lcs / len(target)`` and F-measure ``F = 2 P R / (P + R)``, each 0 where its denominator is 0,
    the lengths taken after removal of ``ignore_index``.  The result is the mean of ``measure`` over the
    pairs (per sample, then averaged, as the usual ROUGE scorers do).  Class version: ``TokenROUGEL``.

    Returns a 0-d float64 tensor, NaN for an empty batch.
    """
    _measure_check(measure)
    x, t, il, tl = _token_check(input, target, input_lengths, target_lengths, ignore_index)
    return _rouge_l_compute(*_lcs_update(x, t, il, tl, ignore_index)[1], measure)


def _measure_check(measure: str) -> None:
    if measure not in MEASURES:
        raise ValueError(f"measure should be one of {MEASURES}, got {measure!r}.")


def _lcs_update(x: torch.Tensor, t: torch.Tensor, il: Lengths, tl: Lengths,
                ignore_index: Optional[int]) -> Tuple[torch.Tensor, Totals]:
    """The ``[B]`` int64 LCS lengths of checked rows and the four float64 totals of the batch: the sums of
    precision, recall and F-measure, and the pairs."""
    if x.shape[0] > 0 and _k30.supported(x, t):
        totals = torch.empty(4, dtype=torch.float64, device=x.device).unbind(0)
        return _k30.lcs(x, t, il, tl, ignore_index, totals, False), totals
    lcs, n, m = _aten_lcs(x, t, il, tl, ignore_index)
    zero = torch.zeros((), dtype=torch.float64, device=x.device)
    p, r = torch.where(n > 0, lcs.double() / n, zero), torch.where(m > 0, lcs.double() / m, zero)
    f = torch.where(p + r > 0, 2.0 * p * r / (p + r), zero)
    return lcs, (p.sum(), r.sum(), f.sum(), torch.tensor(float(x.shape[0]), dtype=torch.float64, device=x.device))


def _rouge_l_compute(precision_sum: torch.Tensor, recall_sum: torch.Tensor, fmeasure_sum: torch.Tensor,
                     pairs: torch.Tensor, measure: str) -> torch.Tensor:
    return (precision_sum, recall_sum, fmeasure_sum)[MEASURES.index(measure)] / pairs


def _aten_lcs(x: torch.Tensor, t: torch.Tensor, il: Lengths, tl: Lengths,
              ignore_index: Optional[int]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The ATen form: LCS lengths and kept lengths, all ``[B]`` int64.  Row ``i`` of the table from row
    ``i - 1`` for every pair at once: ``t_j = max(up_j, diag_j + (a_i == b_j))``, then the left
    dependency ``cur_j = max(t_j, cur_{j-1})`` is ``cummax(t)``.  The loop runs over the narrower side."""
    sides = [_rows(x, il, ignore_index), _rows(t, tl, ignore_index)]
    (a, n), (b, m) = sorted(sides, key=lambda side: side[0].shape[1])  # the LCS is symmetric
    prev = torch.zeros(a.shape[0], b.shape[1] + 1, dtype=torch.int64, device=a.device)
    col = m[:, None]
    lcs = torch.zeros_like(m)
    for i in range(1, a.shape[1] + 1):
        step = torch.maximum(prev[:, 1:], prev[:, :-1] + (a[:, i - 1:i] == b))
        prev = torch.cat([torch.zeros_like(col), torch.cummax(step, dim=1).values], dim=1)
        lcs = torch.where(n == i, prev.gather(1, col)[:, 0], lcs)
    return lcs, sides[0][1], sides[1][1]
