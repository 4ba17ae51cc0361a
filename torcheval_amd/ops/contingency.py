"""K25 wrapper (csrc/kernels/contingency.hip): the int64 ``[R, C]`` contingency table of two label
vectors, and the pair-counting and information indices of such a table.

``contingency_update`` is one launch and one read of both label vectors per slice of the table;
``contingency_values`` is ``compute()``: ``contingency_stats`` (two launches: one read of the table
for the marginals, the exact u64 pair sums and the FP64 ``sum n log n`` partials, then the marginals'
own terms), ``contingency_emi`` when the expected mutual information is asked for, and the
single-wave ``contingency_values`` launch, which leaves every index in one float64 vector (``INDEX``).
No host synchronisation and no float atomics anywhere.  All ops are dispatcher ops only
(``torch.ops.torcheval_amd_contingency``), so eager and compiled calls take the same route.
"""

from typing import Dict, Optional, Tuple

import torch

from torcheval_amd.ops import use_native

# kCtgSliceSmall, kCtgSliceLarge, kCtgBlockSmall, kCtgBlockLarge, kCtgUnit, kCtgMaxBlocks, kCtgMaxCells,
# kCtgStatsBlocks, kCtgMarginBlocks, kCtgEmiBlocks, kCtgEmiMaxParts, kCtgInts and kCtgValues of
# csrc/include/tea_kernels.h (held equal by tests/metrics/clustering/test_contingency.py)
SLICE_SMALL = 4096
SLICE_LARGE = 32768
BLOCK_SMALL = 256
BLOCK_LARGE = 1024
UNIT = 4
MAX_BLOCKS = 1024
MAX_CELLS = 1 << 22
STATS_BLOCKS = 1024
MARGIN_BLOCKS = 256
EMI_BLOCKS = 2048
EMI_MAX_PARTS = 64
INTS = 6
VALUES = 21

# the kernels' own constants, which only size grids (kRows, kStatBlock, kEmiTargetItems of the kernel file)
_ROWS = 16
_STAT_BLOCK = 256
_EMI_TARGET_ITEMS = 4096

# pairs of an update from which the large slice is taken for a table the small one would hold (plan)
LARGE_FROM_PAIRS = 10**6

# steps of kCtgUnit pairs a thread should have before another sample group pays for its block
_STEPS_PER_THREAD = 4

# positions in the values vector; the four averages in the order of AVERAGE_METHODS
AVERAGE_METHODS = ("min", "geometric", "arithmetic", "max")
INDEX = {
    "rand": 0, "adjusted_rand": 1, "fowlkes_mallows": 2, "entropy_true": 3, "entropy_pred": 4,
    "mutual_info": 5, "expected_mutual_info": 6, "normalizer": 7, "normalized_mutual_info": 11,
    "adjusted_mutual_info": 15, "homogeneity": 19, "completeness": 20,
}

_LABEL_DTYPES = (torch.int64, torch.int32)


def plan(n: int, cells: int, slice_size: int = 0) -> Tuple[int, int]:
    """``(slice, groups)`` of an update of ``n`` pairs into a table of ``cells`` cells.

    A block holds one slice of the table in LDS and every slice re-reads all labels, so the label
    traffic is ``ceil(cells / slice)`` reads: a table that the small slice (16 KiB: eight blocks of 256
    threads per CU) does not hold takes the large one (128 KiB: one block of 1024 threads per CU), which
    re-reads the labels an eighth as often (measured at 10^7 pairs: 2.4 x and 7 x faster at 1000 x 1000
    and 2000 x 2000).  Where either slice holds the whole table the benchmark decides
    (profiles/clustering_indices_r39.json, ``slice_sweep``, 10 x 10 and 64 x 64): the large slice is 14 to 33 %
    faster at 10^6 and 10^7 pairs, the small one 8 to 18 % at 10^5, and at 10^4 both are within 1 us of
    the launch; so the large slice from ``LARGE_FROM_PAIRS`` = 10^6 pairs on.  Where between 10^5 and 10^6
    the two cross was not measured.  ``groups`` gives a thread about ``_STEPS_PER_THREAD`` steps, within the
    ``MAX_BLOCKS`` blocks of the persistent grid: a model, no other group count was timed.
    ``slice_size`` forces a slice (tests, the benchmark).
    """
    if slice_size == 0:
        slice_size = SLICE_SMALL if cells <= SLICE_SMALL and n < LARGE_FROM_PAIRS else SLICE_LARGE
    block = BLOCK_SMALL if slice_size == SLICE_SMALL else BLOCK_LARGE
    slices = -(-cells // slice_size)
    want = -(-n // (block * UNIT * _STEPS_PER_THREAD))
    return slice_size, max(1, min(MAX_BLOCKS // slices, want))


def stats_blocks(r: int, c: int) -> int:
    """Blocks of the cell pass (contingency_stats_blocks): length of ``cell_partials``."""
    items = -(-r // _ROWS) * -(-c // 64)
    return max(1, min(STATS_BLOCKS, -(-items // (_STAT_BLOCK // 64))))


def margin_blocks(r: int, c: int) -> int:
    """Blocks of the marginal pass (contingency_margin_blocks): half the length of ``margin_partials``."""
    return max(1, min(MARGIN_BLOCKS, -(-(r + c) // _STAT_BLOCK)))


def emi_parts(r: int, c: int) -> int:
    """Wave-items a pair's n-range is cut into (contingency_emi_parts): more when the pairs alone
    would not fill the device."""
    return max(1, min(EMI_MAX_PARTS, -(-_EMI_TARGET_ITEMS // (r * c))))


def emi_blocks(r: int, c: int) -> int:
    """Blocks of the EMI launch (contingency_emi_blocks): half the length of ``emi_partials``."""
    return max(1, min(EMI_BLOCKS, -(-(r * c * emi_parts(r, c)) // (_STAT_BLOCK // 64))))


def supported_table(table: torch.Tensor) -> bool:
    """Whether ``compute()`` of the int64 ``[R, C]`` table runs K25 as far as the shape decides: a
    contiguous ROCm table of at most ``MAX_CELLS`` cells.  (A total of 2^32 or more is the caller's
    to route to the ATen form: ``contingency_values`` returns the total beside the values.)  Raises on a GPU without
    the extension (``use_native``)."""
    if not use_native(table):
        return False
    return (table.dtype == torch.int64 and table.dim() == 2 and table.is_contiguous()
            and table.shape[0] >= 1 and table.shape[1] >= 1 and table.numel() <= MAX_CELLS)


def supported(labels_true: torch.Tensor, labels_pred: torch.Tensor, table: torch.Tensor) -> bool:
    """Whether the update runs K25: contiguous int64 / int32 label vectors of fewer than 2^31 pairs
    on the device of a ``supported_table``."""
    if not supported_table(table):
        return False
    for t in (labels_true, labels_pred):
        if t.device != table.device or t.dtype not in _LABEL_DTYPES or t.dim() != 1 or not t.is_contiguous():
            return False
    return labels_true.shape[0] == labels_pred.shape[0] and labels_true.shape[0] < 2**31


def contingency_update(labels_true: torch.Tensor, labels_pred: torch.Tensor, table: torch.Tensor,
                       err: Optional[torch.Tensor] = None, slice_size: int = 0) -> None:
    """``table`` += the counts of one ``supported`` batch.  A pair with a label outside its range is
    counted nowhere and sets bit 0 of ``err`` (int32 ``[1]``).  ``slice_size`` forces the slice
    instantiation (tests; 0: the rule of ``plan``)."""
    s, g = plan(labels_true.shape[0], table.numel(), slice_size)
    torch.ops.torcheval_amd_contingency.contingency_update(labels_true, labels_pred, s, g, table, err)


def contingency_stats(table: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The statistics of a ``supported_table``, two launches: int64 ``marginals`` ``[R + C + INTS]`` (row
    sums, column sums, then the exact sums of ``n (n - 1) / 2`` over the cells, the rows and the columns,
    the total, and the numbers of non-empty rows and columns), and float64 ``cell_partials``,
    ``margin_partials`` (the per-block sums of ``n log n``) and ``margin_logs`` (EMI's tables)."""
    r, c = table.shape
    dev = table.device

    def f64(n):
        return torch.empty(n, dtype=torch.float64, device=dev)

    out = {
        "marginals": torch.zeros(r + c + INTS, dtype=torch.int64, device=dev),
        "cell_partials": f64(stats_blocks(r, c)),
        "margin_partials": f64(2 * margin_blocks(r, c)),
        "margin_logs": f64(2 * (r + c)),
    }
    torch.ops.torcheval_amd_contingency.contingency_stats(table, out["marginals"], out["cell_partials"],
                                                          out["margin_partials"], out["margin_logs"])
    return out


def contingency_emi(stats: Dict[str, torch.Tensor], r: int, c: int) -> torch.Tensor:
    """float64 ``[2, emi_blocks(r, c)]``: per block the sum of the terms of the expected mutual
    information of ``contingency_stats``' marginals, and the sum of their magnitudes."""
    partials = torch.empty(2, emi_blocks(r, c), dtype=torch.float64, device=stats["marginals"].device)
    torch.ops.torcheval_amd_contingency.contingency_emi(stats["marginals"], stats["margin_logs"], r, c, partials)
    return partials


def contingency_values(table: torch.Tensor, emi: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """The float64 ``[VALUES]`` vector (``INDEX``) of a ``supported_table``, and the table's total as an
    int64 scalar on the device.  The values hold for a total below 2^32; the total is exact for any
    table, so the caller can tell.  Without ``emi`` the expected mutual information is not evaluated
    and it and AMI are NaN."""
    r, c = table.shape
    stats = contingency_stats(table)
    emi_partials = contingency_emi(stats, r, c) if emi else None
    values = torch.empty(VALUES, dtype=torch.float64, device=table.device)
    torch.ops.torcheval_amd_contingency.contingency_values(stats["marginals"], stats["cell_partials"],
                                                           stats["margin_partials"], emi_partials, values)
    return values, stats["marginals"][r + c + 3]
