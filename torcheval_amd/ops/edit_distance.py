"""K29 wrapper (csrc/kernels/edit_distance.hip): unit-cost Levenshtein distance of padded token-id
rows ``[B, Li]`` against ``[B, Lt]`` on ROCm.

One to three launches per call of the op and no host synchronisation: the prep launch (only with
``ignore_index``) compacts the kept tokens of every row into a workspace; the walk, a systolic wave
over strips of 64 table columns, writes the ``[B]`` int64 distances; the finish launch (only with
``totals``) adds them and the lengths into the four 0-d float64 totals.  The walk has two arms:
``ARM_WAVE`` (a wave per pair, for many short pairs) and ``ARM_BLOCK`` (a workgroup of ``BLOCK_WAVES``
waves per pair, its strips skewed by two 64-step macro steps, for few long pairs); ``pick_arm`` is the
dispatch rule.  Native inputs are contiguous integer tensors (narrow dtypes are widened to int32, a
mixed pair to int64) on one device with both widths at most ``MAX_LEN``, the capacity of the 16-bit
edge column in LDS; everything else is the caller's ATen form.  Lengths are clamped to
``[0, width]`` on the device.  The op is a dispatcher op only (``torch.ops.torcheval_amd_editdist``),
so eager and compiled calls take the same route.
"""

from typing import Optional, Sequence

import torch

from torcheval_amd.ops import use_native
from torcheval_amd.ops.segmentation import LABEL_DTYPES

# kEditMaxLen, kEditArm*, kEditPairsPerWg and kEditBlockWaves of csrc/include/tea_kernels.h
MAX_LEN = 4096
ARM_WAVE, ARM_BLOCK = 0, 1
PAIRS_PER_WG = 4
BLOCK_WAVES = 8
# The block arm takes over for at most BLOCK_MAX_PAIRS pairs whose narrower side is at least
# BLOCK_MIN_WIDTH wide.  Measured on MI355X (profiles/token_edit_distance_r44.json), rows as long as the
# widths: the wave arm takes 5.7x the block arm's time at 32 pairs of 2048 tokens, 2.8x at 256 x 512,
# 1.2-1.3x at 1024 x 256, and 0.5-0.6x (the block arm is slower) at 2048 x 128.  The rule sees the padded
# widths only, because the lengths are on the device: a batch of at most 1024 short rows padded to 256 or
# more columns also takes the block arm, where seven of its eight waves idle through at least 14 barrier
# steps.  That case was not measured; by the 2048 x 128 figure it is probably the slower choice there.
BLOCK_MAX_PAIRS = 1024
BLOCK_MIN_WIDTH = 256


def supported(input: torch.Tensor, target: torch.Tensor) -> bool:
    """Whether the (checked) ``[B, Li]`` / ``[B, Lt]`` pair runs K29: the twin of
    ``edit_distance_geometry_ok``.  Raises on a GPU without the extension (``use_native``)."""
    if not use_native(input) or target.device != input.device:
        return False
    if input.dtype not in LABEL_DTYPES or target.dtype not in LABEL_DTYPES:
        return False
    if not (input.is_contiguous() and target.is_contiguous()):
        return False
    return 1 <= input.shape[0] < 2**30 and input.shape[1] <= MAX_LEN and target.shape[1] <= MAX_LEN


def pick_arm(pairs: int, input_width: int, target_width: int) -> int:
    if pairs <= BLOCK_MAX_PAIRS and min(input_width, target_width) >= BLOCK_MIN_WIDTH:
        return ARM_BLOCK
    return ARM_WAVE


def edit_distance(input: torch.Tensor, target: torch.Tensor, input_lengths: Optional[torch.Tensor],
                  target_lengths: Optional[torch.Tensor], ignore_index: Optional[int],
                  totals: Optional[Sequence[torch.Tensor]] = None, accumulate: bool = False,
                  arm: Optional[int] = None) -> torch.Tensor:
    """The ``[B]`` int64 distances of ``supported`` rows.  ``totals``, four 0-d float64 tensors
    (errors, input_total, target_total, max_total), take the batch (``accumulate``: +=).  ``arm``
    forces ``ARM_WAVE`` or ``ARM_BLOCK``."""
    b, dev = input.shape[0], input.device
    wide = torch.int64 if torch.int64 in (input.dtype, target.dtype) else torch.int32
    x, t = input.to(wide), target.to(wide)
    lengths = [None if n is None else n.to(torch.int64).contiguous() for n in (input_lengths, target_lengths)]
    ws_tokens = ws_lengths = None
    if ignore_index is not None:
        ws_tokens = torch.empty(max(1, b * (x.shape[1] + t.shape[1])), dtype=wide, device=dev)
        ws_lengths = torch.empty(2 * b, dtype=torch.int64, device=dev)
    out = torch.empty(b, dtype=torch.int64, device=dev)
    if arm is None:
        arm = pick_arm(b, x.shape[1], t.shape[1])
    torch.ops.torcheval_amd_editdist.edit_distance(x, t, lengths[0], lengths[1], ignore_index, ws_tokens, ws_lengths,
                                                   arm, out, *(totals or (None,) * 4), accumulate)
    return out
