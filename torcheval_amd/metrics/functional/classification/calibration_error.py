"""Multiclass calibration error (ECE, MCE and the RMS form), functional API.

Not in the reference tree (docs/parity.md, "Not in the reference").  ROCm tensors of native dtypes
run K15 (csrc/kernels/calibration.hip: one pass over the scores and a finish launch); CPU tensors,
float64 and other dtypes, a non-unit column stride and more bins than the kernel holds in LDS run
the ATen form below, which is the definition written with ``softmax`` / ``max`` / ``bucketize`` on
the float32 edge table.
"""

from typing import Optional, Tuple

import torch

import torcheval_amd.ops as _ops
from torcheval_amd.ops import calibration as _k15
from torcheval_amd.ops.hostread import read_int

__all__ = ["multiclass_calibration_error"]

_BAD_TARGET = "multiclass calibration error: `target` holds a label outside [0, num_classes)"
_BAD_CONFIDENCE = (
    "multiclass calibration error: a row's confidence is not in [0, 1] "
    "(a NaN or +inf score, a row of -inf logits, or a probability above 1)"
)


def multiclass_calibration_error(
    input: torch.Tensor,
    target: torch.Tensor,
    *,
    n_bins: int = 15,
    norm: str = "l1",
    from_logits: bool = False,
) -> torch.Tensor:
    """Calibration error of ``[N, C]`` scores against ``[N]`` labels over ``n_bins`` equal-width
    confidence bins.

    A row's prediction is ``torch.argmax``'s (the lowest index among the maxima) and its
    confidence, a float32, is the row maximum (``from_logits=False``) or
    ``1 / sum_j exp(x_j - max)`` formed in FP32, ``-inf`` logits contributing 0
    (``from_logits=True``).  The edges are ``e[b] = float32(b / n_bins)``; a row lies in bin ``b``
    when ``e[b] < conf <= e[b + 1]``, and ``conf == 0`` in bin 0.  With ``bin_count``,
    ``correct_sum`` and ``conf_sum`` per bin in FP64, ``d_b = correct_sum[b] - conf_sum[b]`` and
    ``N = sum(bin_count)``, over the bins that hold a row:

    * ``norm="l1"`` (ECE): ``sum |d_b| / N``
    * ``norm="max"`` (MCE): ``max |d_b| / bin_count[b]``
    * ``norm="l2"``: ``sqrt(sum d_b^2 / (bin_count[b] N))``

    Class version: ``MulticlassCalibrationError``.

    Args:
        input: scores ``[N, C]``: probabilities, or logits with ``from_logits=True``.
        target: integer labels ``[N]`` in ``[0, C)``.  A label outside it, or a row whose confidence
            is not in ``[0, 1]`` (a NaN or ``+inf`` score, a row of ``-inf`` logits, a
            "probability" above 1), raises on CPU; on ROCm the value is NaN and the call raises
            only under ``config.validate``.
        n_bins: number of bins, ``>= 1``.
        norm: ``"l1"``, ``"max"`` or ``"l2"``.
        from_logits: take the softmax of ``input`` first.

    Returns a float32 scalar (float64 input is binned on FP64 edges); NaN for ``N == 0``.
    """
    _calibration_param_check(n_bins, norm)
    _calibration_input_check(input, target)
    if _ops.compiling():
        return _calibration_error(input, target, n_bins, norm, from_logits)
    with torch.inference_mode():
        return _calibration_error(input, target, n_bins, norm, from_logits)


def _calibration_param_check(n_bins: int, norm: str) -> None:
    if not isinstance(n_bins, int) or isinstance(n_bins, bool) or n_bins < 1:
        raise ValueError(f"`n_bins` should be a positive integer, got {n_bins}.")
    if norm not in _k15.NORMS:
        raise ValueError(f"`norm` should be one of {_k15.NORMS}, got {norm!r}.")


def _calibration_input_check(input: torch.Tensor, target: torch.Tensor) -> None:
    if input.ndim != 2:
        raise ValueError(
            f"input should be a two-dimensional tensor (num_sample, num_classes), got shape {input.shape}."
        )
    if target.ndim != 1:
        raise ValueError(f"target should be a one-dimensional tensor, got shape {target.shape}.")
    if target.shape[0] != input.shape[0]:
        raise ValueError(
            "The `input` and `target` should have the same first dimension, "
            f"got shapes {input.shape} and {target.shape}."
        )
    if target.is_floating_point() or target.is_complex() or target.dtype == torch.bool:
        raise ValueError(f"target should hold integer labels, got dtype {target.dtype}.")
    if input.shape[0] > 0 and input.shape[1] == 0:
        raise ValueError(f"input should have at least one class, got shape {input.shape}.")


def _bad_rows_message(code: int) -> str:
    return "; ".join(m for bit, m in ((1, _BAD_TARGET), (2, _BAD_CONFIDENCE)) if code & bit)


def _raise_on_bad_rows(err: Optional[torch.Tensor]) -> None:
    """Surface (and clear) the device flag of bad rows: bit 0 the target, bit 1 the confidence."""
    if err is None:
        return
    code = read_int(err)
    if code != 0:
        err.zero_()
        raise ValueError(_bad_rows_message(code) + " (such rows made the value NaN).")


def _calibration_error(input: torch.Tensor, target: torch.Tensor, n_bins: int, norm: str,
                       from_logits: bool) -> torch.Tensor:
    from torcheval_amd.config import config

    if input.shape[0] == 0:
        return torch.full((), torch.nan, dtype=torch.float32, device=input.device)
    err = torch.zeros(1, dtype=torch.int32, device=input.device) if input.is_cuda and config.validate else None
    if _k15.supported(input, target, n_bins):
        out = _k15.calibration_error(input, target, n_bins, from_logits, norm, err)
    else:
        states = _calibration_update(input, target, n_bins, from_logits, err)
        out = _calibration_value(*states, norm)
    _raise_on_bad_rows(err)
    return out


def _bin_edges(n_bins: int, dtype: torch.dtype, device: torch.device) -> torch.Tensor:
    """``b / n_bins`` for ``b = 0 .. n_bins``: the quotient in FP64, then rounded to ``dtype``."""
    return (torch.arange(n_bins + 1, dtype=torch.float64) / n_bins).to(dtype).to(device)


def _calibration_update(input: torch.Tensor, target: torch.Tensor, n_bins: int, from_logits: bool,
                        err: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The ATen form of one batch, exactly as defined: float64 ``[n_bins]`` (bin_count,
    correct_sum, conf_sum) of checked inputs with ``N >= 1``.  Confidences are float32, float64
    (on FP64 edges) only for float64 input.  Bad rows raise on CPU; on ROCm they add NaN to
    ``conf_sum[0]``, are counted nowhere else and set their bits of ``err`` (when given)."""
    x = input if input.dtype in (torch.float32, torch.float64) else input.float()
    pred = x.argmax(dim=1)
    conf = torch.softmax(x, dim=1).max(dim=1).values if from_logits else x.max(dim=1).values
    bad_target = (target < 0) | (target >= input.shape[1])
    bad_conf = ~((conf >= 0) & (conf <= 1))
    bad = bad_target | bad_conf
    if not input.is_cuda:
        code = int(bad_target.any()) | (int(bad_conf.any()) << 1)
        if code != 0:
            raise ValueError(_bad_rows_message(code) + ".")
    elif err is not None:
        err.bitwise_or_((bad_target.any().to(err.dtype) | (bad_conf.any().to(err.dtype) << 1)))
    edges = _bin_edges(n_bins, x.dtype, x.device)
    # bucketize (right=False): the i with edges[i - 1] < conf <= edges[i]; 0 only for conf == 0
    bins = (torch.bucketize(torch.where(bad, 0, conf), edges) - 1).clamp_(0, n_bins - 1)
    zeros = torch.zeros(n_bins, dtype=torch.float64, device=x.device)
    bin_count = zeros.scatter_add(0, bins, (~bad).double())
    correct_sum = zeros.scatter_add(0, bins, ((pred == target) & ~bad).double())
    conf_sum = zeros.scatter_add(0, bins, torch.where(bad, 0, conf).double())
    conf_sum[0] += torch.where(bad.any(), torch.nan, 0.0)
    return bin_count, correct_sum, conf_sum


def _calibration_value(bin_count: torch.Tensor, correct_sum: torch.Tensor, conf_sum: torch.Tensor,
                       norm: str) -> torch.Tensor:
    """The value of three float64 ``[n_bins]`` states as a float32 scalar: FP64 over the bins that
    hold a row; NaN without rows or with a NaN in ``conf_sum[0]`` (a bad row)."""
    total = bin_count.sum()
    filled = bin_count > 0
    d = torch.where(filled, (correct_sum - conf_sum).abs(), 0.0)
    rows = torch.where(filled, bin_count, 1.0)
    if norm == "l1":
        value = d.sum() / total
    elif norm == "max":
        value = (d / rows).max()
    else:
        value = torch.sqrt((d * d / (rows * total)).sum())
    defined = (total > 0) & ~conf_sum[0].isnan()
    return torch.where(defined, value, torch.nan).float()
