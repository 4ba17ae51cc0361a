"""Panoptic quality (PQ, with its factors SQ and RQ), functional API.

Not in the reference tree (docs/parity.md, "Not in the reference", has the definition: COCO
``panopticapi``'s rule set).  ROCm maps of integer dtypes run K28 (csrc/kernels/panoptic.hip): one read
of both maps into LDS tables of the co-occurring segment pairs, a match launch per batch and a finish
launch, with no host synchronisation before the flag word is read.  CPU tensors, non-contiguous maps,
more classes than the kernel's table holds, and calls whose flag word reports an image above the
kernel's capacities or an instance id outside ``[0, 2^32)`` run the ATen form below, which is the
definition written per image with ``unique(dim=0, return_inverse=True)`` and ``bincount``.
"""

import functools
from typing import Collection, Optional, Tuple

import torch

import torcheval_amd.ops as _ops
from torcheval_amd.ops import panoptic as _k28
from torcheval_amd.ops.hostread import read_int

__all__ = ["panoptic_quality"]

_UNKNOWN = "panoptic_quality: `input` holds a category that is in neither `things` nor `stuffs`"
_LIMITS = (
    f"panoptic_quality: an image has more than {_k28.MAX_SEGMENTS} segments on one side (void included) or "
    f"more than {_k28.MAX_PAIRS} co-occurring segment pairs, or a thing instance id lies outside [0, 2^32)"
)


def panoptic_quality(
    input: torch.Tensor,
    target: torch.Tensor,
    *,
    things: Collection[int],
    stuffs: Collection[int],
    allow_unknown_preds_category: bool = False,
    return_sq_and_rq: bool = False,
    return_per_class: bool = False,
) -> torch.Tensor:
    """Panoptic quality of predicted against true panoptic segmentations (Kirillov et al., 2019).

    A pixel is ``(category_id, instance_id)``.  Its segment is ``(class, instance)`` for a thing
    class, ``(class, 0)`` for a stuff class (the instance id is ignored) and *void* for any other
    category.  Per image, a predicted and a true segment of one class match when
    ``iou = inter / (area_p - pvoid_p + area_t - inter) > 1/2`` (an integer test; ``pvoid_p`` the
    predicted segment's pixels on void ground truth); a match adds 1 to ``tp[class]`` and ``iou`` to
    ``iou_sum[class]``.  An unmatched true segment of which at most half is predicted void adds 1 to
    ``fn[class]``; an unmatched predicted segment of which at most half lies on void adds 1 to
    ``fp[class]``.  Per class ``PQ = iou_sum / (tp + fp/2 + fn/2)``, ``SQ = iou_sum / tp`` and
    ``RQ = tp / (tp + fp/2 + fn/2)``; the reported value is the mean over the classes whose
    denominator is not zero, NaN when there is none.

    Class version: ``PanopticQuality``.

    Args:
        input: integer ``[N, *spatial, 2]``, the last axis ``(category_id, instance_id)``.
        target: likewise, of the same shape.  An unknown category is void.
        things: the category ids with instances.
        stuffs: the category ids without; disjoint from ``things``.  The classes are the union of
            both, ascending.
        allow_unknown_preds_category: an unknown category in ``input`` is void; otherwise it raises
            ``ValueError``.
        return_sq_and_rq: return ``(PQ, SQ, RQ)`` along a last axis of 3.
        return_per_class: return the per-class values, ``[K]`` (NaN for a class with a zero
            denominator), and not their mean.

    Returns a float32 tensor: a scalar, ``[3]``, ``[K]`` or ``[K, 3]``.
    """
    classes = _panoptic_classes(things, stuffs)
    _panoptic_input_check(input, target)
    if _ops.compiling():
        values = _panoptic_batch(input, target, classes, bool(allow_unknown_preds_category), bool(return_per_class))
    else:
        with torch.inference_mode():
            values = _panoptic_batch(input, target, classes, bool(allow_unknown_preds_category),
                                     bool(return_per_class))
    return values if return_sq_and_rq else values[..., 0]


def _panoptic_classes(things: Collection[int], stuffs: Collection[int]) -> Tuple[Tuple[int, ...], Tuple[bool, ...]]:
    """Checks the two collections; the category ids ascending and whether each is a thing class."""
    for name, ids in (("things", things), ("stuffs", stuffs)):
        if isinstance(ids, (str, torch.Tensor)) or not all(isinstance(c, int) and not isinstance(c, bool)
                                                           and -2**63 <= c < 2**63 for c in ids):
            raise ValueError(f"`{name}` should be a collection of integer category ids, got {ids!r}.")
    things, stuffs = set(things), set(stuffs)
    if things & stuffs:
        raise ValueError(f"`things` and `stuffs` should be disjoint, both hold {sorted(things & stuffs)}.")
    if not things | stuffs:
        raise ValueError("`things` and `stuffs` should name at least one category.")
    cats = tuple(sorted(things | stuffs))
    return cats, tuple(c in things for c in cats)


def _panoptic_input_check(input: torch.Tensor, target: torch.Tensor) -> None:
    for name, x in (("input", input), ("target", target)):
        if x.is_floating_point() or x.is_complex() or x.dtype == torch.bool:
            raise ValueError(f"{name} should hold integer (category_id, instance_id) pairs, got dtype {x.dtype}.")
    if input.ndim < 2 or input.shape[-1] != 2:
        raise ValueError(f"input should be (num_sample, *spatial, 2), got shape {input.shape}.")
    if input.shape != target.shape:
        raise ValueError(f"The `input` and `target` should have one shape, got {input.shape} and {target.shape}.")


@functools.lru_cache(maxsize=16)
def _class_table(classes: Tuple[Tuple[int, ...], Tuple[bool, ...]], device: torch.device) -> torch.Tensor:
    """``[2, K]`` int64 on ``device``: the category ids ascending, then 1 for a thing class."""
    return torch.tensor([classes[0], [int(t) for t in classes[1]]], dtype=torch.int64).to(device)


def _raise_on_flags(flag: Optional[torch.Tensor]) -> None:
    """Surface (and clear) the device flag word of a class: once per ``compute()``."""
    if flag is None:
        return
    code = read_int(flag)
    if code != 0:
        flag.zero_()
        if code & (_k28.FLAG_CAPACITY | _k28.FLAG_INSTANCE):
            raise RuntimeError(_LIMITS + " (the image's segments were counted nowhere or under a wrong id; "
                               "such images take the functional, or CPU tensors).")
        raise ValueError(_UNKNOWN + " (it was taken as void).")


def _panoptic_batch(input: torch.Tensor, target: torch.Tensor, classes, allow_unknown: bool,
                    per_class: bool) -> torch.Tensor:
    """``(PQ, SQ, RQ)`` of one checked batch, float32: ``[3]``, or ``[K, 3]``."""
    k = len(classes[0])
    table = _class_table(classes, input.device)
    if input.numel() == 0:
        return torch.full((k, 3) if per_class else (3,), torch.nan, device=input.device)
    if _k28.supported(input, target, k):
        dev = input.device
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        states = torch.empty((4, k), dtype=torch.float64, device=dev)
        out = torch.empty((k, 3) if per_class else (3,), dtype=torch.float32, device=dev)
        _k28.panoptic_quality(input, target, table, allow_unknown, flag, states.unbind(0), False, per_class, out)
        code = 0 if _ops.compiling() else read_int(flag)
        if code == 0:
            return out
        if code == _k28.FLAG_UNKNOWN:
            raise ValueError(_UNKNOWN + ".")
        # above a capacity or an instance id outside the key: the ATen form (which raises on an unknown category)
    return _panoptic_value(*_panoptic_update(input, target, table, allow_unknown), per_class)


def _canonical(x: torch.Tensor, table: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``[P, 2]`` raw pixels to canonical ``(class, instance)`` rows, void ``(K, 0)``; and whether
    every category is known."""
    k = table.shape[1]
    cat, inst = x[:, 0], x[:, 1]
    idx = torch.searchsorted(table[0], cat.contiguous()).clamp(max=k - 1)
    known = table[0][idx] == cat
    cls = torch.where(known, idx, k)
    inst = torch.where(known & (table[1][idx] != 0), inst, 0)
    return torch.stack([cls, inst], dim=1), known.all()


def _panoptic_update(input: torch.Tensor, target: torch.Tensor, table: torch.Tensor,
                     allow_unknown: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The ATen form of one batch, exactly as defined: float64 ``[K]`` (iou_sum, tp, fp, fn)."""
    n, k, dev = input.shape[0], table.shape[1], input.device
    x, t = input.reshape(n, -1, 2).long(), target.reshape(n, -1, 2).long()
    iou_sum = torch.zeros(k, dtype=torch.float64, device=dev)
    counts = torch.zeros((3, k), dtype=torch.int64, device=dev)
    for i in range(n):
        pkeys, known = _canonical(x[i], table)
        if not allow_unknown and not bool(known):
            raise ValueError(_UNKNOWN + ".")
        tkeys, _ = _canonical(t[i], table)
        pairs, inverse = torch.unique(torch.cat([pkeys, tkeys], dim=1), dim=0, return_inverse=True)
        inter = torch.bincount(inverse, minlength=pairs.shape[0])
        psegs, ps = torch.unique(pairs[:, :2], dim=0, return_inverse=True)
        tsegs, ts = torch.unique(pairs[:, 2:], dim=0, return_inverse=True)
        zeros_p, zeros_t = inter.new_zeros(psegs.shape[0]), inter.new_zeros(tsegs.shape[0])
        area_p, area_t = zeros_p.index_add(0, ps, inter), zeros_t.index_add(0, ts, inter)
        pvoid = zeros_p.index_add(0, ps, inter * (pairs[:, 2] == k))
        tvoid = zeros_t.index_add(0, ts, inter * (pairs[:, 0] == k))
        union = area_p[ps] - pvoid[ps] + area_t[ts] - inter
        match = (pairs[:, 0] == pairs[:, 2]) & (pairs[:, 0] < k) & (2 * inter > union)
        cls = pairs[match, 0]
        iou_sum.index_add_(0, cls, inter[match].double() / union[match].double())
        counts[0] += torch.bincount(cls, minlength=k)
        for row, segs, index, area, void in ((1, psegs, ps, area_p, pvoid), (2, tsegs, ts, area_t, tvoid)):
            unmatched = torch.ones_like(area, dtype=torch.bool)
            unmatched[index[match]] = False
            counted = unmatched & (segs[:, 0] < k) & (2 * void <= area)
            counts[row] += torch.bincount(segs[counted, 0], minlength=k)
    return iou_sum, counts[0].double(), counts[1].double(), counts[2].double()


def _panoptic_value(iou_sum: torch.Tensor, tp: torch.Tensor, fp: torch.Tensor, fn: torch.Tensor,
                    per_class: bool) -> torch.Tensor:
    """``(PQ, SQ, RQ)`` of four float64 ``[K]`` states, float32: ``[K, 3]`` with NaN where the
    denominator is zero, or ``[3]``, the means over the classes where it is not (NaN without one)."""
    den = tp + 0.5 * fp + 0.5 * fn
    values = torch.stack([iou_sum / den, iou_sum / tp, tp / den], dim=1)
    if per_class:
        return values.float()
    has = torch.stack([den, tp, den], dim=1) > 0
    return (torch.where(has, values, 0.0).sum(0) / has.sum(0)).float()
