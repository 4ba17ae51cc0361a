"""K17 wrapper (csrc/kernels/segmentation.hip): per-class intersection, predicted and target pixel
counts of segmentation scores ``[N, C, *spatial]`` (or a predicted label map ``[N, *spatial]``)
against a label map ``[N, *spatial]``, and mean IoU / Dice from them.

Two launches per call and no host synchronisation: the count launch (a persistent grid of at most
``max_blocks()`` blocks, each owning ``SPAN`` pixels of one image at a time) writes one ``[3, C]``
u32 partial per block; the finish launch adds them in block order into the class states, or into a
scratch triple whose value it evaluates.  ``compute()`` of the classes is the single-wave
``segmentation_value`` launch.  Native inputs are float32 / float16 / bfloat16 scores whose spatial
dims flatten to one stride (``arm``), integer label maps and ``num_classes <= max_classes()``;
everything else is the caller's ATen form.  The ops are dispatcher ops only
(``torch.ops.torcheval_amd_segmentation``), so eager and compiled calls take the same route.
"""

from typing import Optional, Tuple

import torch

from torcheval_amd.ops import use_native

_SCORE_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
LABEL_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)
ARMS = ("plane", "element", "label")  # the kernels' arm codes are the positions
AVERAGES = ("macro", "micro", "none")  # likewise

# kSegSpan, kSegMaxBlocks and kSegMaxClasses of csrc/include/tea_kernels.h (held equal by
# tests/metrics/classification/test_mean_iou.py): the edges at which the GPU tests place their shapes
SPAN = 2048
MAX_BLOCKS = 1024
MAX_CLASSES = 1024


def max_blocks() -> int:
    """The persistent grid's cap: more spans than this and a block loops over several."""
    return MAX_BLOCKS


def max_classes() -> int:
    """The most classes K17 takes: a block's three u32 histograms in LDS are 12 KiB at the cap, so
    the 8 blocks of 256 threads a CU can hold need 96 KiB of its 160 KiB."""
    return MAX_CLASSES


def _flat_stride(sizes, strides) -> Optional[int]:
    """The one stride the dims flatten to (``1`` for at most one element), or ``None``."""
    dims = [(n, s) for n, s in zip(sizes, strides) if n != 1]
    for (_, s), (n1, s1) in zip(dims, dims[1:]):
        if s != s1 * n1:
            return None
    return dims[-1][1] if dims else 1


def arm(input: torch.Tensor) -> str:
    """``"label"`` for an integer map; for scores ``"plane"`` (unit pixel stride, and for 16-bit
    scores a class stride of whole 16-byte units, so that every class plane of an image is aligned
    alike), ``"element"`` (any other layout whose spatial dims flatten to one stride:
    ``channels_last``, 16-bit planes of an odd size) or ``""`` (a cropped view: no arm)."""
    if input.dtype in LABEL_DTYPES:
        return "label"
    stride_p = _flat_stride(input.shape[2:], input.stride()[2:])
    if stride_p is None:
        return ""
    if stride_p == 1 and (input.dtype == torch.float32 or input.shape[1] == 1 or input.stride(1) % 8 == 0):
        return "plane"
    return "element"


def supported(input: torch.Tensor, target: torch.Tensor, num_classes: int) -> bool:
    """Whether the (checked) pair runs K17: ROCm tensors on one device, native dtypes, at least one
    pixel, ``num_classes <= max_classes()``, a layout an arm takes, and fewer than 2^32 pixels per
    block of the grid.  Raises on a GPU without the extension (``use_native``)."""
    if not use_native(input) or target.device != input.device:
        return False
    if input.dtype not in _SCORE_DTYPES + LABEL_DTYPES or target.dtype not in LABEL_DTYPES:
        return False
    if not 1 <= num_classes <= MAX_CLASSES or target.numel() == 0:
        return False
    spans = target.shape[0] * -(-(target.numel() // target.shape[0]) // SPAN)
    if -(-spans // min(spans, MAX_BLOCKS)) >= 2**32 // SPAN:  # a block's u32 counts
        return False
    return arm(input) != ""


def _maps(input: torch.Tensor, target: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``[N, C, P]`` scores (a view) or an ``[N, P]`` label map, and the ``[N, P]`` target."""
    n = target.shape[0]
    if input.dtype in LABEL_DTYPES:
        return input.reshape(n, -1), target.reshape(n, -1)
    p = target.numel() // n
    stride_p = _flat_stride(input.shape[2:], input.stride()[2:])
    return input.as_strided((n, input.shape[1], p), (input.stride(0), input.stride(1), stride_p)), target.reshape(n, -1)


def segmentation_update(input: torch.Tensor, target: torch.Tensor, num_classes: int, ignore_index: Optional[int],
                        intersection: torch.Tensor, pred_count: torch.Tensor, target_count: torch.Tensor,
                        err: Optional[torch.Tensor]) -> None:
    """The three float64 ``[num_classes]`` states += the counts of one ``supported`` batch.  A
    counted pixel whose target (bit 0 of ``err``) or label-map prediction (bit 1) lies outside
    ``[0, num_classes)`` is counted nowhere."""
    x, t = _maps(input, target)
    torch.ops.torcheval_amd_segmentation.segmentation_update(x, t, num_classes, ARMS.index(arm(input)), ignore_index,
                                                             intersection, pred_count, target_count, err)


def segmentation_batch(input: torch.Tensor, target: torch.Tensor, num_classes: int, ignore_index: Optional[int],
                       dice: bool, average: str, err: Optional[torch.Tensor]) -> torch.Tensor:
    """The float32 value of one ``supported`` batch: a scalar, or ``[num_classes]`` for
    ``average="none"`` (``average`` one of ``AVERAGES``)."""
    x, t = _maps(input, target)
    out = torch.empty((num_classes,) if average == "none" else (), dtype=torch.float32, device=input.device)
    torch.ops.torcheval_amd_segmentation.segmentation_batch(x, t, num_classes, ARMS.index(arm(input)), ignore_index,
                                                            dice, AVERAGES.index(average), out, err)
    return out


def segmentation_value(intersection: torch.Tensor, pred_count: torch.Tensor, target_count: torch.Tensor, dice: bool,
                       average: str) -> torch.Tensor:
    """The float32 value of three float64 ``[num_classes]`` ROCm states."""
    shape = (intersection.numel(),) if average == "none" else ()
    out = torch.empty(shape, dtype=torch.float32, device=intersection.device)
    torch.ops.torcheval_amd_segmentation.segmentation_value(intersection, pred_count, target_count, dice,
                                                            AVERAGES.index(average), out)
    return out
