"""K21 wrapper (csrc/kernels/inception_score.hip): the Inception Score's sufficient statistics of
``[N, C]`` logits and the value of the statistics.

``inception_update`` is two launches: the row launch reads every row once (a wave per row, the row in
registers) and stores one FP64 ``[C + 2]`` partial per block, the finish launch adds the partials
in block order into the three float64 states.  ``inception_value`` is one launch.  No atomic, no
host synchronisation, results bit-identical from run to run.  Native inputs are ROCm float32 /
float16 / bfloat16 logits with unit stride along ``C``, any non-negative row stride and any element
alignment, ``1 <= C <= max_columns()``, ``1 <= S <= max_splits()`` and ``N < 2^31``, with contiguous
float64 states; everything else is the caller's ATen form.  The ops are dispatcher ops only
(``torch.ops.torcheval_amd_inception``), so eager and compiled calls take the same route.
"""

from typing import Tuple

import torch

from torcheval_amd.ops import use_native

_DTYPES = (torch.float32, torch.float16, torch.bfloat16)

# The constants of csrc/include/tea_kernels.h (kInception*), held equal by
# tests/metrics/image/test_inception_score.py.
MAX_COLUMNS = 2048
MAX_SPLITS = 64
MAX_BLOCKS = 1024  # grid cap of the row launch: splits x blocks per split
WAVES_PER_BLOCK = 4
NARROW_COLUMNS = 256
ROWS_PER_WAVE_NARROW = 32
ROWS_PER_WAVE_WIDE = 8


def max_columns() -> int:
    return MAX_COLUMNS


def max_splits() -> int:
    return MAX_SPLITS


def blocks_per_split(n: int, splits: int, c: int) -> int:
    """``inception_blocks`` of the kernel unit: a wave aims at 32 (``C <= 256``) or 8 rows of the
    largest split, until ``splits x blocks`` reaches ``MAX_BLOCKS``."""
    rows = (n + splits - 1) // splits
    per_block = WAVES_PER_BLOCK * (ROWS_PER_WAVE_NARROW if c <= NARROW_COLUMNS else ROWS_PER_WAVE_WIDE)
    return max(1, min((rows + per_block - 1) // per_block, MAX_BLOCKS // splits))


def _states_ok(ref: torch.Tensor, *states: torch.Tensor) -> bool:
    return all(t.dtype == torch.float64 and t.device == ref.device and t.is_contiguous() for t in states)


def supported(logits: torch.Tensor, prob_sum: torch.Tensor, neg_entropy_sum: torch.Tensor,
              num_rows: torch.Tensor) -> bool:
    """Whether the checked update runs K21.  Raises on a GPU without the extension
    (``use_native``)."""
    if not use_native(logits) or logits.dtype not in _DTYPES or logits.dim() != 2:
        return False
    n, c = logits.shape
    if not 1 <= n < 2**31 or not 1 <= c <= MAX_COLUMNS or not 1 <= prob_sum.shape[0] <= MAX_SPLITS:
        return False
    if (c > 1 and logits.stride(1) != 1) or (n > 1 and logits.stride(0) < 0):
        return False
    return _states_ok(logits, prob_sum, neg_entropy_sum, num_rows)


def value_supported(prob_sum: torch.Tensor, neg_entropy_sum: torch.Tensor, num_rows: torch.Tensor) -> bool:
    """Whether the value of these states is K21's value launch."""
    if not use_native(prob_sum) or not 1 <= prob_sum.shape[0] <= MAX_SPLITS or prob_sum.shape[1] < 1:
        return False
    return _states_ok(prob_sum, prob_sum, neg_entropy_sum, num_rows)


def inception_update(logits: torch.Tensor, first_split: int, prob_sum: torch.Tensor, neg_entropy_sum: torch.Tensor,
                     num_rows: torch.Tensor) -> None:
    """The three states += the statistics of the rows of ``logits``, row ``i`` into split
    ``(first_split + i) mod S``."""
    torch.ops.torcheval_amd_inception.inception_update(logits, first_split, prob_sum, neg_entropy_sum, num_rows)


def inception_value(prob_sum: torch.Tensor, neg_entropy_sum: torch.Tensor,
                    num_rows: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(split_log, out)``: float64 ``[S]`` (NaN for a split without rows) and float32 ``[2]``, the
    mean and the population standard deviation of ``exp(split_log)`` over the splits with rows."""
    split_log = torch.empty(prob_sum.shape[0], dtype=torch.float64, device=prob_sum.device)
    out = torch.empty(2, dtype=torch.float32, device=prob_sum.device)
    torch.ops.torcheval_amd_inception.inception_value(prob_sum, neg_entropy_sum, num_rows, split_log, out)
    return split_log, out
