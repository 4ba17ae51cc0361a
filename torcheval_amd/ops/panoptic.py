"""K28 wrapper (csrc/kernels/panoptic.hip): panoptic quality of ``(category, instance)`` map pairs
``[N, P, 2]`` on ROCm.

Three launches per call of the op and no host synchronisation: the pairs launch (a persistent grid of
at most ``MAX_BLOCKS`` blocks, each owning ``SPAN`` pixels of one image at a time) interns the span's
segments and co-occurring pairs in LDS tables and emits them into the span's region of a workspace;
the match launch, one workgroup per image, merges the regions and applies the matching rules; the
finish launch adds the per-image partials in image order into the four ``[K]`` float64 states, or into
a scratch quadruple whose PQ / SQ / RQ it evaluates.  ``compute()`` of the class is the single-wave
``panoptic_value`` launch.  Native inputs are contiguous integer maps (narrow dtypes are widened to
int32, a mixed pair to int64) on one device with at most ``MAX_CLASSES`` classes and fewer than 2^31
pixels per image; everything else is the caller's ATen form.  An image with more than ``MAX_SEGMENTS``
segments a side (void included) or ``MAX_PAIRS`` co-occurring pairs, or a thing instance id outside
``[0, 2^32)``, sets a bit of the flag word, which the caller reads.  A batch whose workspace exceeds
``WORKSPACE_CAP`` bytes runs in chunks of whole images.  The ops are dispatcher ops only
(``torch.ops.torcheval_amd_panoptic``), so eager and compiled calls take the same route.
"""

from typing import Optional, Sequence

import torch

from torcheval_amd.ops import use_native
from torcheval_amd.ops.segmentation import LABEL_DTYPES

# kPanSpan, kPanMaxBlocks, kPanMaxClasses, kPanMaxSegments and kPanMaxPairs of csrc/include/tea_kernels.h:
# the edges at which the GPU tests place their shapes
SPAN = 1024
MAX_BLOCKS = 1024
MAX_CLASSES = 1024
MAX_SEGMENTS = 1024
MAX_PAIRS = 4096
FLAG_UNKNOWN, FLAG_CAPACITY, FLAG_INSTANCE = 1, 2, 4  # kPanFlag*
WORKSPACE_CAP = 256 << 20  # bytes of span regions per call of the op
_PIXEL_BYTES = 20  # of a region per pixel of its span: two u64 keys and a u32 count


def supported(input: torch.Tensor, target: torch.Tensor, num_classes: int) -> bool:
    """Whether the (checked) pair of maps runs K28.  Raises on a GPU without the extension
    (``use_native``)."""
    if not use_native(input) or target.device != input.device:
        return False
    if input.dtype not in LABEL_DTYPES or target.dtype not in LABEL_DTYPES:
        return False
    if not (input.is_contiguous() and target.is_contiguous()) or input.numel() == 0:
        return False
    return 1 <= num_classes <= MAX_CLASSES and input.numel() // (2 * input.shape[0]) < 2**31


def images_per_call(pixels: int) -> int:
    """The most whole images whose span regions stay within ``WORKSPACE_CAP`` (at least one)."""
    return max(1, WORKSPACE_CAP // (-(-pixels // SPAN) * SPAN * _PIXEL_BYTES))


def panoptic_quality(input: torch.Tensor, target: torch.Tensor, table: torch.Tensor, allow_unknown: bool,
                     flag: torch.Tensor, states: Sequence[torch.Tensor], accumulate: bool, per_class: bool = False,
                     out: Optional[torch.Tensor] = None) -> None:
    """The four ``[K]`` float64 ``states`` (iou_sum, tp, fp, fn) take the images of ``supported`` maps
    (``accumulate``: +=); ``out`` (float32 ``[3]``, or ``[K, 3]`` for ``per_class``) the PQ / SQ / RQ of
    the states after them.  ``table`` is the ``[2, K]`` int64 class table: the category ids ascending,
    then 1 for a thing class and 0 for stuff."""
    n = input.shape[0]
    wide = torch.int64 if torch.int64 in (input.dtype, target.dtype) else torch.int32
    x, t = input.reshape(n, -1, 2).to(wide), target.reshape(n, -1, 2).to(wide)
    p, k, dev = x.shape[1], table.shape[1], x.device
    step = min(n, images_per_call(p))
    spans = step * -(-p // SPAN)
    ws_keys = torch.empty(spans * 2 * SPAN, dtype=torch.int64, device=dev)
    ws_counts = torch.empty(spans * SPAN, dtype=torch.int32, device=dev)
    ws_heads = torch.empty(spans, dtype=torch.int32, device=dev)
    part_iou = torch.empty(step * k, dtype=torch.int64, device=dev)
    part_counts = torch.empty(step * 3 * k, dtype=torch.int32, device=dev)
    for i in range(0, n, step):
        torch.ops.torcheval_amd_panoptic.panoptic_quality(
            x[i:i + step], t[i:i + step], table, allow_unknown, ws_keys, ws_counts, ws_heads, part_iou, part_counts,
            flag, *states, accumulate or i > 0, per_class, out if i + step >= n else None)


def panoptic_value(states: Sequence[torch.Tensor], per_class: bool) -> torch.Tensor:
    """The float32 (PQ, SQ, RQ) of four float64 ``[K]`` ROCm states: ``[3]``, or ``[K, 3]``."""
    k = states[0].numel()
    out = torch.empty((k, 3) if per_class else (3,), dtype=torch.float32, device=states[0].device)
    torch.ops.torcheval_amd_panoptic.panoptic_value(*states, per_class, out)
    return out
