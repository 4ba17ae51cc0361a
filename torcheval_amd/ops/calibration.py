"""K15 wrapper (csrc/kernels/calibration.hip): multiclass calibration error of [N, C] scores.

Two launches per call and no host synchronisation: the row launch (a wave per row above
``THREAD_ARM_MAX_COLUMNS`` columns, a thread per row up to there) writes one partial triple of bin
counts, correct counts and confidence sums per block; the finish launch adds them in block order
into the class states, or into a scratch triple whose value it evaluates.  ``compute()`` of the
class is the single-wave ``calibration_value`` launch.  Native inputs are float32 / float16 /
bfloat16 scores with a unit column stride and any row stride, int64 / int32 targets and
``n_bins <= max_bins()``; everything else is the caller's ATen form.  The ops are dispatcher ops
only (``torch.ops.torcheval_amd_calibration``), so eager and compiled calls take the same route.
"""

from typing import Optional

import torch

from torcheval_amd.ops import use_native

_SCORE_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_TARGET_DTYPES = (torch.int64, torch.int32)
NORMS = ("l1", "max", "l2")  # the kernels' norm codes are the positions

# kCalibMaxBins, kCalibNarrowMaxC and the rows one row launch covers before it grid-strides
# (kCalibMaxBlocks blocks of 4 waves or 256 threads), csrc/include/tea_kernels.h; held equal by
# tests/metrics/classification/test_calibration_error.py
MAX_BINS = 256
THREAD_ARM_MAX_COLUMNS = 32
WAVE_ARM_ROWS_PER_LAUNCH = 1024 * 4
THREAD_ARM_ROWS_PER_LAUNCH = 1024 * 256


def max_bins() -> int:
    """The most bins K15 takes: four wave-private bin sets of a block in LDS, 17 KiB at the cap,
    which leaves room for the eight blocks a CU holds at full occupancy."""
    return MAX_BINS


def rows_per_launch(num_columns: int) -> int:
    """Rows the row launch covers with one row per wave (thread) before it grid-strides."""
    return WAVE_ARM_ROWS_PER_LAUNCH if num_columns > THREAD_ARM_MAX_COLUMNS else THREAD_ARM_ROWS_PER_LAUNCH


def supported(input: torch.Tensor, target: torch.Tensor, n_bins: int) -> bool:
    """Whether the call runs K15: ROCm tensors on one device, native dtypes, ``[N >= 1, C >= 1]``
    scores with a unit column stride, ``[N]`` targets and ``n_bins <= max_bins()``.  Raises on a
    GPU without the extension (``use_native``)."""
    if not use_native(input) or target.device != input.device:
        return False
    if input.dtype not in _SCORE_DTYPES or target.dtype not in _TARGET_DTYPES:
        return False
    if input.dim() != 2 or target.dim() != 1 or target.shape[0] != input.shape[0]:
        return False
    n, c = input.shape
    if n < 1 or c < 1 or c >= 2**31 or not 1 <= n_bins <= MAX_BINS:
        return False
    return c == 1 or input.stride(1) == 1


def calibration_update(input: torch.Tensor, target: torch.Tensor, n_bins: int, from_logits: bool,
                       bin_count: torch.Tensor, correct_sum: torch.Tensor, conf_sum: torch.Tensor,
                       err: Optional[torch.Tensor]) -> None:
    """The three float64 ``[n_bins]`` states += the batch's bin counts, correct counts and sums of
    confidences.  A bad row adds NaN to ``conf_sum[0]`` only and sets bit 0 (target outside
    ``[0, C)``) or bit 1 (confidence outside ``[0, 1]``) of ``err``."""
    torch.ops.torcheval_amd_calibration.calibration_update(input, target, n_bins, from_logits, bin_count,
                                                           correct_sum, conf_sum, err)


def calibration_error(input: torch.Tensor, target: torch.Tensor, n_bins: int, from_logits: bool, norm: str,
                      err: Optional[torch.Tensor]) -> torch.Tensor:
    """The float32 scalar value of one batch (``norm`` one of ``NORMS``)."""
    out = torch.empty((), dtype=torch.float32, device=input.device)
    torch.ops.torcheval_amd_calibration.calibration_error(input, target, n_bins, from_logits, NORMS.index(norm), out,
                                                          err)
    return out


def calibration_value(bin_count: torch.Tensor, correct_sum: torch.Tensor, conf_sum: torch.Tensor,
                      norm: str) -> torch.Tensor:
    """The float32 scalar value of three float64 ``[n_bins]`` ROCm states."""
    out = torch.empty((), dtype=torch.float32, device=bin_count.device)
    torch.ops.torcheval_amd_calibration.calibration_value(bin_count, correct_sum, conf_sum, NORMS.index(norm), out)
    return out
