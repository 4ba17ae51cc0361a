"""Segmentation mean IoU (Jaccard index) and Dice score, functional API.

Not in the reference tree (docs/parity.md, "Not in the reference").  ROCm tensors of native dtypes
run K17 (csrc/kernels/segmentation.hip: one pass over the scores with the class axis strided, and
a finish launch); CPU tensors, float64 scores, more classes than the kernel holds in LDS and
layouts whose spatial dims do not flatten to one stride run the ATen form below, which is the
definition written with ``argmax``, a mask and int64 ``bincount``s.
"""

from typing import Optional, Tuple

import torch

import torcheval_amd.ops as _ops
from torcheval_amd.ops import segmentation as _k17
from torcheval_amd.ops.hostread import read_int

__all__ = ["dice_score", "mean_iou"]

_BAD_TARGET = "segmentation metric: `target` holds a counted label outside [0, num_classes)"
_BAD_PREDICTION = "segmentation metric: the label-map `input` holds a counted label outside [0, num_classes)"


def mean_iou(
    input: torch.Tensor,
    target: torch.Tensor,
    *,
    num_classes: int,
    ignore_index: Optional[int] = None,
    average: Optional[str] = "macro",
) -> torch.Tensor:
    """Intersection over union of a predicted segmentation against a label map.

    With ``intersection[c]``, ``pred_count[c]`` and ``target_count[c]`` the numbers of counted
    pixels predicted and labelled ``c``, predicted ``c`` and labelled ``c``:
    ``iou_c = intersection[c] / (pred_count[c] + target_count[c] - intersection[c])`` in FP64, NaN
    for a class absent from both maps.  The counts are over all pixels of the call, at dataset
    level: the value is not a mean of per-image values.

    * ``average="macro"``: the mean over the classes present in either map (the mmseg /
      ``nanmean`` convention behind published mIoU numbers).
    * ``average="micro"``: ``sum(intersection) / sum(union)``.
    * ``average=None`` or ``"none"``: the ``[num_classes]`` vector.

    Class version: ``MeanIoU``.

    Args:
        input: scores ``[N, C, *spatial]`` with ``C == num_classes`` (float32, float16, bfloat16 or
            float64), whose prediction is ``torch.argmax(input, dim=1)`` (the lowest class among
            the maxima; NaN is the maximum), or integer labels ``[N, *spatial]`` already predicted.
        target: integer labels ``[N, *spatial]``.  A counted label outside ``[0, num_classes)``,
            in ``target`` or in a label-map ``input``, raises on CPU; on ROCm the pixel is counted
            nowhere and the call raises only under ``config.validate``.
        num_classes: number of classes, ``>= 1``.
        ignore_index: a pixel with ``target == ignore_index`` is counted nowhere.  Any integer:
            255, -1, -100, or a class.
        average: ``"macro"``, ``"micro"``, ``"none"`` or ``None``.

    Returns a float32 tensor (float64 for float64 scores); NaN when no pixel was counted.
    """
    return _segmentation_metric(input, target, num_classes, ignore_index, average, False)


def dice_score(
    input: torch.Tensor,
    target: torch.Tensor,
    *,
    num_classes: int,
    ignore_index: Optional[int] = None,
    average: Optional[str] = "macro",
) -> torch.Tensor:
    """Dice score (F1 over pixels) of a predicted segmentation against a label map:
    ``dice_c = 2 intersection[c] / (pred_count[c] + target_count[c])``, NaN for a class absent
    from both maps; ``average="micro"`` is ``2 sum(intersection) / sum(pred_count + target_count)``.
    Everything else, the dataset-level counting included, as ``mean_iou``.

    Class version: ``DiceScore``.
    """
    return _segmentation_metric(input, target, num_classes, ignore_index, average, True)


def _segmentation_metric(input: torch.Tensor, target: torch.Tensor, num_classes: int, ignore_index: Optional[int],
                         average: Optional[str], dice: bool) -> torch.Tensor:
    average = _segmentation_param_check(num_classes, ignore_index, average)
    _segmentation_input_check(input, target, num_classes)
    if _ops.compiling():
        return _segmentation_batch(input, target, num_classes, ignore_index, average, dice)
    with torch.inference_mode():
        return _segmentation_batch(input, target, num_classes, ignore_index, average, dice)


def _segmentation_param_check(num_classes: int, ignore_index: Optional[int], average: Optional[str]) -> str:
    """Checks the parameters; returns ``average`` with ``None`` spelled ``"none"``."""
    if not isinstance(num_classes, int) or isinstance(num_classes, bool) or num_classes < 1:
        raise ValueError(f"`num_classes` should be a positive integer, got {num_classes}.")
    if ignore_index is not None and (not isinstance(ignore_index, int) or isinstance(ignore_index, bool)):
        raise ValueError(f"`ignore_index` should be an integer or None, got {ignore_index!r}.")
    if average is None:
        return "none"
    if average not in _k17.AVERAGES:
        raise ValueError(f"`average` should be one of {_k17.AVERAGES} or None, got {average!r}.")
    return average


def _segmentation_input_check(input: torch.Tensor, target: torch.Tensor, num_classes: int) -> None:
    if target.is_floating_point() or target.is_complex() or target.dtype == torch.bool:
        raise ValueError(f"target should hold integer labels, got dtype {target.dtype}.")
    if target.ndim < 1:
        raise ValueError(f"target should be (num_sample, *spatial), got shape {target.shape}.")
    if input.is_complex() or input.dtype == torch.bool:
        raise ValueError(f"input should hold scores or integer labels, got dtype {input.dtype}.")
    if not input.is_floating_point():
        if input.shape != target.shape:
            raise ValueError(
                f"A label-map `input` should have the shape of `target`, got shapes {input.shape} and {target.shape}."
            )
        return
    if input.ndim != target.ndim + 1:
        raise ValueError(
            "input should be scores (num_sample, num_classes, *spatial) for a target (num_sample, *spatial), "
            f"got shapes {input.shape} and {target.shape}."
        )
    if input.shape[1] != num_classes:
        raise ValueError(f"input should have num_classes={num_classes} entries along dim 1, got shape {input.shape}.")
    if input.shape[0] != target.shape[0] or input.shape[2:] != target.shape[1:]:
        raise ValueError(
            "The `input` and `target` should agree in num_sample and in the spatial shape, "
            f"got shapes {input.shape} and {target.shape}."
        )


def _bad_labels_message(code: int) -> str:
    return "; ".join(m for bit, m in ((1, _BAD_TARGET), (2, _BAD_PREDICTION)) if code & bit)


def _raise_on_bad_labels(err: Optional[torch.Tensor]) -> None:
    """Surface (and clear) the device flag of bad labels: bit 0 the target, bit 1 the prediction."""
    if err is None:
        return
    code = read_int(err)
    if code != 0:
        err.zero_()
        raise ValueError(_bad_labels_message(code) + " (such pixels were counted nowhere).")


def _segmentation_batch(input: torch.Tensor, target: torch.Tensor, num_classes: int, ignore_index: Optional[int],
                        average: str, dice: bool) -> torch.Tensor:
    from torcheval_amd.config import config

    dtype = torch.float64 if input.dtype == torch.float64 else torch.float32
    if target.numel() == 0:
        return torch.full((num_classes,) if average == "none" else (), torch.nan, dtype=dtype, device=input.device)
    err = torch.zeros(1, dtype=torch.int32, device=input.device) if input.is_cuda and config.validate else None
    if _k17.supported(input, target, num_classes):
        out = _k17.segmentation_batch(input, target, num_classes, ignore_index, dice, average, err)
    else:
        states = _segmentation_update(input, target, num_classes, ignore_index, err)
        out = _segmentation_value(*states, dice, average, dtype)
    _raise_on_bad_labels(err)
    return out


def _segmentation_update(input: torch.Tensor, target: torch.Tensor, num_classes: int, ignore_index: Optional[int],
                         err: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The ATen form of one batch, exactly as defined: float64 ``[num_classes]`` (intersection,
    pred_count, target_count) of checked inputs with at least one pixel.  Labels are widened to
    int64 before they meet ``ignore_index``, so an index outside the target dtype's range ignores
    nothing.  Bad labels raise on CPU; on ROCm their pixels are counted nowhere and set their bits
    of ``err`` (when given)."""
    if input.is_floating_point():
        x = input.float() if not input.is_cuda and input.dtype in (torch.float16, torch.bfloat16) else input
        pred = x.argmax(dim=1).reshape(-1)
    else:
        pred = input.reshape(-1).long()
    t = target.reshape(-1).long()
    counted = torch.ones_like(t, dtype=torch.bool) if ignore_index is None else t != ignore_index
    bad_target = counted & ((t < 0) | (t >= num_classes))
    bad_pred = counted & ((pred < 0) | (pred >= num_classes))
    if not input.is_cuda:
        code = int(bad_target.any()) | (int(bad_pred.any()) << 1)
        if code != 0:
            raise ValueError(_bad_labels_message(code) + ".")
    elif err is not None:
        err.bitwise_or_(bad_target.any().to(err.dtype) | (bad_pred.any().to(err.dtype) << 1))
    keep = counted & ~bad_target & ~bad_pred
    t, pred = t[keep], pred[keep]
    intersection = torch.bincount(t[t == pred], minlength=num_classes)
    pred_count = torch.bincount(pred, minlength=num_classes)
    target_count = torch.bincount(t, minlength=num_classes)
    return intersection.double(), pred_count.double(), target_count.double()


def _segmentation_value(intersection: torch.Tensor, pred_count: torch.Tensor, target_count: torch.Tensor, dice: bool,
                        average: str, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """The value of three float64 ``[num_classes]`` states as ``dtype``: FP64 per class, NaN for a
    class absent from both maps, which the macro mean leaves out; NaN without a counted pixel."""
    both = pred_count + target_count
    union = both - intersection
    top, bottom = (2.0 * intersection, both) if dice else (intersection, union)
    if average == "none":
        return (top / bottom).to(dtype)
    if average == "micro":
        return (top.sum() / bottom.sum()).to(dtype)
    present = union > 0
    per_class = torch.where(present, top / torch.where(present, bottom, 1.0), 0.0)
    return (per_class.sum() / present.sum()).to(dtype)
