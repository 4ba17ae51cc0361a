"""Hausdorff distance and average surface distance of segmentations, functional API.

Not in the reference tree (docs/parity.md, "Not in the reference", has the definition: the MONAI
convention).  ROCm label maps of native dtypes with unit spacing run K27
(csrc/kernels/surface_distance.hip): an exact integer nearest-surface search separated by axis, with no
host synchronisation.  CPU tensors, a ``spacing`` other than ones, non-contiguous maps and planes
larger than the kernel's limit run the ATen form below, which is the definition written with shifted
masks and a float64 ``torch.cdist``; it is not meant to be fast.
"""

import math
from typing import Optional, Sequence, Tuple

import torch

import torcheval_amd.ops as _ops
from torcheval_amd.ops import surface_distance as _k27

__all__ = ["average_surface_distance", "hausdorff_distance"]

# pairs of surface pixels per ``cdist`` call of the ATen form.  On ROCm a float64 ``cdist`` of 4096 x ~5000
# points (512 x 512 maps) returned wrong distances where the CPU and 2^22 pairs per call agree; supposed
# cause: its kernel takes a workgroup of 256 threads per pair, 2^32 threads at 2^24 pairs
_PAIRS = 1 << 22


def hausdorff_distance(
    input: torch.Tensor,
    target: torch.Tensor,
    *,
    num_classes: int,
    include_background: bool = False,
    percentile: Optional[float] = None,
    directed: bool = False,
    spacing: Optional[Sequence[float]] = None,
) -> torch.Tensor:
    """Hausdorff distance between the predicted and the true boundary, per image and class.

    For image ``n`` and class ``c`` let ``A = (pred == c)`` and ``B = (target == c)``.  The surface of
    a mask is the set of its pixels with a 4-neighbour outside it (outside the image counts as
    outside the mask), and ``d(a, surface(B))`` is the Euclidean distance, in units of ``spacing``, to
    the nearest pixel of ``B``'s surface.  The directed value ``h(A, B)`` is the maximum of
    ``d(a, surface(B))`` over ``A``'s surface, or with ``percentile=p`` the ``p``-th percentile of those
    distances (linear interpolation at position ``p / 100 * (m - 1)``, as ``numpy.percentile``; 95
    gives HD95).  The metric is ``h(A, B)`` when ``directed``, otherwise ``max(h(A, B), h(B, A))``.
    NaN when both surfaces are empty, ``+inf`` when exactly one is.

    Class version: ``HausdorffDistance``.

    Args:
        input: integer labels ``[N, H, W]``, or scores ``[N, C, H, W]`` with ``C == num_classes``
            whose prediction is ``torch.argmax(input, dim=1)``.
        target: integer labels ``[N, H, W]``.  A label outside ``[0, num_classes)`` belongs to no
            class.
        num_classes: number of classes.
        include_background: whether class 0 gets a column.
        percentile: ``None`` for the maximum, or a number in ``[0, 100]``.
        directed: only ``h(A, B)``.
        spacing: the pixel size along ``(H, W)``; ``None`` is ``(1, 1)``.

    Returns ``[N, K]`` float32 with ``K = num_classes``, or ``num_classes - 1`` without the background.
    """
    _surface_param_check(num_classes, include_background, spacing)
    if percentile is not None and (isinstance(percentile, bool) or not isinstance(percentile, (int, float))
                                   or not 0 <= percentile <= 100):
        raise ValueError(f"`percentile` should be None or a number in [0, 100], got {percentile!r}.")
    quantile = -1.0 if percentile is None else percentile / 100.0
    return _surface_metric(input, target, num_classes, include_background, 0, quantile, not directed, spacing)


def average_surface_distance(
    input: torch.Tensor,
    target: torch.Tensor,
    *,
    num_classes: int,
    include_background: bool = False,
    symmetric: bool = True,
    spacing: Optional[Sequence[float]] = None,
) -> torch.Tensor:
    """Average surface distance, per image and class: with the surfaces and ``d`` of
    ``hausdorff_distance``, the mean of ``d(a, surface(B))`` over ``A``'s surface when not ``symmetric``,
    otherwise the sum of the distances in both directions over the size of both surfaces (ASSD).  NaN
    when both surfaces are empty, ``+inf`` when exactly one is; everything else as
    ``hausdorff_distance``.

    Class version: ``AverageSurfaceDistance``.
    """
    _surface_param_check(num_classes, include_background, spacing)
    return _surface_metric(input, target, num_classes, include_background, 1, -1.0, bool(symmetric), spacing)


def _surface_param_check(num_classes: int, include_background: bool, spacing: Optional[Sequence[float]]) -> None:
    least = 1 if include_background else 2
    if not isinstance(num_classes, int) or isinstance(num_classes, bool) or num_classes < least:
        raise ValueError(
            f"`num_classes` should be an integer of at least {least} (include_background={include_background}), "
            f"got {num_classes}."
        )
    if spacing is not None:
        ok = not isinstance(spacing, (str, torch.Tensor)) and len(spacing) == 2
        if not ok or not all(isinstance(s, (int, float)) and math.isfinite(s) and s > 0 for s in spacing):
            raise ValueError(f"`spacing` should be None or two positive numbers for (H, W), got {spacing!r}.")


def _surface_average_check(average: Optional[str]) -> str:
    if average is None:
        return "none"
    if average not in ("macro", "none"):
        raise ValueError(f"`average` should be 'macro', 'none' or None, got {average!r}.")
    return average


def _surface_input_check(input: torch.Tensor, target: torch.Tensor, num_classes: int) -> None:
    if target.is_floating_point() or target.is_complex() or target.dtype == torch.bool:
        raise ValueError(f"target should hold integer labels, got dtype {target.dtype}.")
    if target.ndim != 3:
        raise ValueError(f"target should be a (num_sample, H, W) label map, got shape {target.shape}.")
    if input.is_complex() or input.dtype == torch.bool:
        raise ValueError(f"input should hold scores or integer labels, got dtype {input.dtype}.")
    if not input.is_floating_point():
        if input.shape != target.shape:
            raise ValueError(
                f"A label-map `input` should have the shape of `target`, got shapes {input.shape} and {target.shape}."
            )
        return
    if input.ndim != 4 or input.shape[1] != num_classes:
        raise ValueError(
            f"Scores should be (num_sample, num_classes={num_classes}, H, W), got shape {input.shape}."
        )
    if input.shape[0] != target.shape[0] or input.shape[2:] != target.shape[1:]:
        raise ValueError(
            "The `input` and `target` should agree in num_sample and in the spatial shape, "
            f"got shapes {input.shape} and {target.shape}."
        )


def _surface_metric(input: torch.Tensor, target: torch.Tensor, num_classes: int, include_background: bool, mode: int,
                    quantile: float, both: bool, spacing: Optional[Sequence[float]]) -> torch.Tensor:
    _surface_input_check(input, target, num_classes)
    if _ops.compiling():
        return _surface_batch(input, target, num_classes, include_background, mode, quantile, both, spacing)
    with torch.inference_mode():
        return _surface_batch(input, target, num_classes, include_background, mode, quantile, both, spacing)


def _label_map(input: torch.Tensor) -> torch.Tensor:
    """The predicted label map of scores (``argmax`` over the class axis, in ATen), or the map itself."""
    if not input.is_floating_point():
        return input
    x = input.float() if not input.is_cuda and input.dtype in (torch.float16, torch.bfloat16) else input
    return x.argmax(dim=1)


def _unit(spacing: Optional[Sequence[float]]) -> bool:
    return spacing is None or all(float(s) == 1.0 for s in spacing)


def _surface_batch(input: torch.Tensor, target: torch.Tensor, num_classes: int, include_background: bool, mode: int,
                   quantile: float, both: bool, spacing: Optional[Sequence[float]],
                   states: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None) -> Optional[torch.Tensor]:
    """The ``[N, K]`` float32 values of one checked batch; with ``states`` (the classes' update) the
    three ``[K]`` float64 states += the finite values, their number and the number of ``+inf``, and
    nothing is returned."""
    base = 0 if include_background else 1
    classes = num_classes - base
    pred = _label_map(input)
    n = target.shape[0]
    if target.numel() == 0:  # no image, or images without a pixel: both surfaces are empty
        return None if states is not None else torch.full((n, classes), torch.nan, device=input.device)
    native = _unit(spacing) and _k27.supported(pred, target, num_classes)
    if native and (states is None or states[0].device == pred.device):
        out = None if states is not None else torch.empty((n, classes), dtype=torch.float32, device=pred.device)
        _k27.surface_distance(pred, target, classes, base, mode, quantile, both, out, *(states or ()))
        return out
    values = _surface_values(pred, target, classes, base, mode, quantile, both, spacing)
    if states is None:
        return values
    finite = values.isfinite()
    states[0].add_(torch.where(finite, values, 0.0).sum(0, dtype=torch.float64).to(states[0].device))
    states[1].add_(finite.sum(0).double().to(states[1].device))
    states[2].add_(values.isinf().sum(0).double().to(states[2].device))
    return None


def _surface_points(mask: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """The float64 ``[m, 2]`` coordinates, in units of the spacing, of the surface of a bool ``[H, W]``
    mask: its pixels with a 4-neighbour outside it, by comparing the zero-padded mask with its shifts."""
    p = torch.nn.functional.pad(mask, (1, 1, 1, 1))
    inner = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return (mask & ~inner).nonzero().double() * scale


def _nearest(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """For every point of ``a`` the distance to the nearest point of ``b`` (both non-empty)."""
    rows = max(1, _PAIRS // b.shape[0])
    return torch.cat([
        torch.cdist(a[i:i + rows], b, compute_mode="donot_use_mm_for_euclid_dist").min(dim=1).values
        for i in range(0, a.shape[0], rows)
    ])


def _surface_values(pred: torch.Tensor, target: torch.Tensor, classes: int, base: int, mode: int, quantile: float,
                    both: bool, spacing: Optional[Sequence[float]]) -> torch.Tensor:
    """The ATen form, exactly as defined: ``[N, classes]`` float32 of integer label maps."""
    n = target.shape[0]
    scale = torch.tensor([1.0, 1.0] if spacing is None else [float(s) for s in spacing], dtype=torch.float64,
                         device=pred.device)
    out = torch.empty((n, classes), dtype=torch.float64, device=pred.device)
    for i in range(n):
        for k in range(classes):
            a = _surface_points(pred[i] == k + base, scale)
            b = _surface_points(target[i] == k + base, scale)
            if a.shape[0] == 0 or b.shape[0] == 0:
                out[i, k] = math.nan if a.shape[0] == b.shape[0] else math.inf
                continue
            dists = [_nearest(a, b)] + ([_nearest(b, a)] if both else [])
            if mode == 1:
                out[i, k] = sum(d.sum() for d in dists) / sum(d.numel() for d in dists)
            elif quantile < 0:
                out[i, k] = max(d.max() for d in dists)
            else:
                out[i, k] = max(torch.quantile(d, quantile) for d in dists)
    return out.float()
