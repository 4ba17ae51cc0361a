"""Token edit distance and token error rates, functional API.

Not in the reference tree (docs/parity.md, "Not in the reference", has the definition).  The word-level
metrics of this family take Python strings; these take what an ASR, OCR or translation evaluation loop
already holds on the device: padded integer id rows with a length per row.  ROCm tensors run K29
(csrc/kernels/edit_distance.hip): a systolic wave over strips of 64 table columns, exact integers, no
host synchronisation outside ``config.validate``.  CPU tensors, non-contiguous rows and widths above
``ops.edit_distance.MAX_LEN`` run the ATen form below: one batched row recurrence per stream position,
whose left dependency a ``cummin`` resolves.
"""

from typing import Optional, Tuple

import torch

from torcheval_amd.config import config
from torcheval_amd.metrics.functional.text.word_error_rate import _word_error_rate_compute
from torcheval_amd.metrics.functional.text.word_information_lost import _wil_compute
from torcheval_amd.metrics.functional.text.word_information_preserved import _word_information_preserved_compute
from torcheval_amd.ops import edit_distance as _k29
from torcheval_amd.ops.segmentation import LABEL_DTYPES

__all__ = ["token_edit_distance", "token_error_rate"]

MEASURES = ("wer", "mer", "wil", "wip")
Lengths = Optional[torch.Tensor]
Totals = Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]


@torch.inference_mode()
def token_edit_distance(input: torch.Tensor, target: torch.Tensor, input_lengths: Lengths = None,
                        target_lengths: Lengths = None, *, ignore_index: Optional[int] = None) -> torch.Tensor:
    """Unit-cost Levenshtein distance between the token-id rows of ``input`` and ``target``.

    Row ``b`` of a side is its first ``lengths[b]`` entries (the whole row without lengths); every
    entry equal to ``ignore_index`` is then removed, wherever it stands.  Tokens compare as integers
    at full width: a negative id or an int64 id of 2^31 or above is a token like any other.

    Args:
        input: integer ``[B, Li]`` predicted ids (a 1-D tensor is one pair).
        target: integer ``[B, Lt]`` reference ids; the two widths may differ.
        input_lengths: integer ``[B]``, or None.  Lengths outside ``[0, width]`` raise ``ValueError``
            under ``config.validate`` (one host read) and are clamped to it otherwise.
        target_lengths: likewise.
        ignore_index: the id to remove from both sides (padding, a CTC blank), or None.

    Returns the ``[B]`` int64 distances.
    """
    x, t, il, tl = _token_check(input, target, input_lengths, target_lengths, ignore_index)
    return _token_update(x, t, il, tl, ignore_index)[0]


@torch.inference_mode()
def token_error_rate(input: torch.Tensor, target: torch.Tensor, input_lengths: Lengths = None,
                     target_lengths: Lengths = None, *, ignore_index: Optional[int] = None,
                     measure: str = "wer") -> torch.Tensor:
    """An error rate over the token-id pairs of one batch; see ``token_edit_distance`` for the rows.

    With ``errors`` the sum of the distances and ``input_total``, ``target_total`` and ``max_total``
    the sums of the row lengths (after removal) and of the longer of each pair: ``"wer"`` is
    ``errors / target_total``, ``"mer"`` is ``errors / max_total``, ``"wil"`` and ``"wip"`` are word
    information lost and preserved with ``max_total - errors`` hits, exactly as the word-level
    metrics of this package compute them.  Class version: ``TokenErrorRate``.

    Returns a 0-d float64 tensor.
    """
    _measure_check(measure)
    x, t, il, tl = _token_check(input, target, input_lengths, target_lengths, ignore_index)
    return _token_error_rate_compute(*_token_update(x, t, il, tl, ignore_index)[1], measure)


def _measure_check(measure: str) -> None:
    if measure not in MEASURES:
        raise ValueError(f"measure should be one of {MEASURES}, got {measure!r}.")


def _ignore_index_check(ignore_index: Optional[int]) -> None:
    if ignore_index is not None and (isinstance(ignore_index, bool) or not isinstance(ignore_index, int)
                                     or not -2**63 <= ignore_index < 2**63):
        raise ValueError(f"ignore_index should be an int64 value or None, got {ignore_index!r}.")


def _token_check(input: torch.Tensor, target: torch.Tensor, input_lengths: Lengths, target_lengths: Lengths,
                 ignore_index: Optional[int]) -> Tuple[torch.Tensor, torch.Tensor, Lengths, Lengths]:
    """Host checks without a synchronisation (one host read under ``config.validate``); the two sides
    as ``[B, L]`` and their lengths."""
    for name, x in (("input", input), ("target", target)):
        if not isinstance(x, torch.Tensor) or x.dtype not in LABEL_DTYPES:
            raise ValueError(f"{name} should be an integer tensor of token ids, got {getattr(x, 'dtype', type(x))}.")
    if input.ndim not in (1, 2) or target.ndim != input.ndim:
        raise ValueError(f"input and target should both be (num_pairs, length) or both (length,), got shapes "
                         f"{input.shape} and {target.shape}.")
    if input.ndim == 1:
        input, target = input.unsqueeze(0), target.unsqueeze(0)
    if input.shape[0] != target.shape[0]:
        raise ValueError(f"input and target should hold the same number of rows, got {input.shape[0]} and "
                         f"{target.shape[0]}.")
    if input.device != target.device:
        raise ValueError(f"input and target should be on one device, got {input.device} and {target.device}.")
    _ignore_index_check(ignore_index)
    bad = None
    for name, n, x in (("input_lengths", input_lengths, input), ("target_lengths", target_lengths, target)):
        if n is None:
            continue
        if not isinstance(n, torch.Tensor) or n.dtype not in LABEL_DTYPES or n.shape != (x.shape[0],):
            raise ValueError(f"{name} should be an integer tensor of shape ({x.shape[0]},), got "
                             f"{getattr(n, 'dtype', type(n))} {tuple(getattr(n, 'shape', ()))}.")
        if n.device != x.device:
            raise ValueError(f"{name} should be on the device of the ids, got {n.device} and {x.device}.")
        if config.validate:
            out = ((n < 0) | (n > x.shape[1])).any()
            bad = out if bad is None else bad | out
    if bad is not None and bool(bad):
        raise ValueError(f"lengths should lie in [0, width] (widths {input.shape[1]} and {target.shape[1]}).")
    return input, target, input_lengths, target_lengths


def _token_update(x: torch.Tensor, t: torch.Tensor, il: Lengths, tl: Lengths,
                  ignore_index: Optional[int]) -> Tuple[torch.Tensor, Totals]:
    """The ``[B]`` int64 distances of checked rows and the four float64 totals of the batch."""
    if x.shape[0] > 0 and _k29.supported(x, t):
        totals = torch.empty(4, dtype=torch.float64, device=x.device).unbind(0)
        return _k29.edit_distance(x, t, il, tl, ignore_index, totals, False), totals
    d, n, m = _aten_distances(x, t, il, tl, ignore_index)
    return d, tuple(v.sum().double() for v in (d, n, m, torch.maximum(n, m)))


def _token_error_rate_compute(errors: torch.Tensor, input_total: torch.Tensor, target_total: torch.Tensor,
                              max_total: torch.Tensor, measure: str) -> torch.Tensor:
    if measure == "wer":
        return _word_error_rate_compute(errors, target_total)
    if measure == "mer":
        return _word_error_rate_compute(errors, max_total)
    if measure == "wil":
        return _wil_compute(errors - max_total, target_total, input_total)
    return _word_information_preserved_compute(max_total - errors, target_total, input_total)


def _rows(x: torch.Tensor, lengths: Lengths, ignore_index: Optional[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """int64 rows with the kept tokens first, and the kept lengths."""
    x = x.long()
    b, width = x.shape
    n = torch.full((b,), width, device=x.device) if lengths is None else lengths.long().clamp(0, width)
    if ignore_index is None:
        return x, n
    drop = (x == ignore_index) | (torch.arange(width, device=x.device) >= n[:, None])
    order = torch.argsort(drop, dim=1, stable=True)
    return x.gather(1, order), width - drop.sum(1)


def _aten_distances(x: torch.Tensor, t: torch.Tensor, il: Lengths, tl: Lengths,
                    ignore_index: Optional[int]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The ATen form: distances and kept lengths, all ``[B]`` int64.  Row ``i`` of the table from row
    ``i - 1`` for every pair at once: ``t_j = min(up + 1, diag + (a_i != b_j))``, then the left
    dependency ``cur_j = min(t_j, cur_{j-1} + 1)`` is ``cummin(t - j) + j``."""
    (a, n), (b, m) = _rows(x, il, ignore_index), _rows(t, tl, ignore_index)
    j = torch.arange(b.shape[1] + 1, device=a.device)
    prev = j.expand(a.shape[0], -1)
    col = m[:, None]
    d = torch.where(n == 0, m, torch.zeros_like(m))
    for i in range(1, a.shape[1] + 1):
        step = torch.minimum(prev[:, 1:] + 1, prev[:, :-1] + (a[:, i - 1:i] != b))
        step = torch.cat([torch.full_like(col, i), step], dim=1)
        prev = torch.cummin(step - j, dim=1).values + j
        d = torch.where(n == i, prev.gather(1, col)[:, 0], d)
    return d, n, m
