"""K30 wrapper (csrc/kernels/lcs.hip): length of the longest common subsequence of padded token-id rows
``[B, Li]`` against ``[B, Lt]`` on ROCm, and the ROUGE-L sums of the batch.

One to three launches per call of the op and no host synchronisation: the prep launch (only with
``ignore_index``) compacts the kept tokens of every row into a workspace, as K29's does; the main launch,
a wave per pair, keeps the narrower side (by padded width, ``input`` on a tie) stationary in ``chunks``
registers of 64 columns, runs the other side past it one token at a time as a bit-vector update of a
table row, and writes the ``[B]`` int64 lengths; the finish launch (only with ``totals``) adds the pairs'
precision, recall and F-measure and their number into four 0-d float64 totals.  ``pick_chunks`` is the
instance rule.  Native inputs are contiguous integer tensors (narrow dtypes are widened to int32, a mixed
pair to int64) on one device with both widths at most ``MAX_LEN``; everything else is the caller's ATen
form.  Lengths are clamped to ``[0, width]`` on the device.  The op is a dispatcher op only
(``torch.ops.torcheval_amd_lcs``), so eager and compiled calls take the same route.
"""

from typing import Optional, Sequence

import torch

from torcheval_amd.ops import use_native
from torcheval_amd.ops.segmentation import LABEL_DTYPES

# kLcsMaxLen, kLcsMaxChunks and kLcsPairsPerWg of csrc/include/tea_kernels.h
MAX_LEN = 4096
MAX_CHUNKS = 64
PAIRS_PER_WG = 4


def supported(input: torch.Tensor, target: torch.Tensor) -> bool:
    """Whether the (checked) ``[B, Li]`` / ``[B, Lt]`` pair runs K30: the twin of ``lcs_geometry_ok``.
    Raises on a GPU without the extension (``use_native``)."""
    if not use_native(input) or target.device != input.device:
        return False
    if input.dtype not in LABEL_DTYPES or target.dtype not in LABEL_DTYPES:
        return False
    if not (input.is_contiguous() and target.is_contiguous()):
        return False
    return 1 <= input.shape[0] < 2**30 and input.shape[1] <= MAX_LEN and target.shape[1] <= MAX_LEN


def pick_chunks(input_width: int, target_width: int) -> int:
    """The smallest instance that holds the stationary (narrower) side: ``pow2ceil(ceil(width / 64))``,
    the twin of ``lcs_chunks``."""
    need = (min(input_width, target_width) + 63) // 64
    return 1 if need <= 1 else 1 << (need - 1).bit_length()


def lcs(input: torch.Tensor, target: torch.Tensor, input_lengths: Optional[torch.Tensor],
        target_lengths: Optional[torch.Tensor], ignore_index: Optional[int],
        totals: Optional[Sequence[torch.Tensor]] = None, accumulate: bool = False,
        chunks: Optional[int] = None) -> torch.Tensor:
    """The ``[B]`` int64 LCS lengths of ``supported`` rows.  ``totals``, four 0-d float64 tensors (the sums of
    precision, recall and F-measure, and the pairs), take the batch (``accumulate``: +=).  ``chunks`` forces a
    larger instance than ``pick_chunks`` gives."""
    b, dev = input.shape[0], input.device
    wide = torch.int64 if torch.int64 in (input.dtype, target.dtype) else torch.int32
    x, t = input.to(wide), target.to(wide)
    lengths = [None if n is None else n.to(torch.int64).contiguous() for n in (input_lengths, target_lengths)]
    ws_tokens = ws_lengths = None
    if ignore_index is not None:
        ws_tokens = torch.empty(max(1, b * (x.shape[1] + t.shape[1])), dtype=wide, device=dev)
        ws_lengths = torch.empty(2 * b, dtype=torch.int64, device=dev)
    out = torch.empty(b, dtype=torch.int64, device=dev)
    if chunks is None:
        chunks = pick_chunks(x.shape[1], t.shape[1])
    torch.ops.torcheval_amd_lcs.lcs(x, t, lengths[0], lengths[1], ignore_index, ws_tokens, ws_lengths, chunks, out,
                                    *(totals or (None,) * 4), accumulate)
    return out
