"""Float64 CPU oracle of the surface-distance metrics (docs/parity.md, "Not in the reference"), as brute
force in numpy; it imports nothing from the package.  Surfaces come from shifted comparisons, distances
from all pairs of surface pixels, the values from ``min``, ``max``, ``np.percentile`` and ``sum``.
Cross-checked once, outside the suite, against scipy's ``binary_erosion`` (cross element, zero border)
and ``distance_transform_edt``.

Tolerance (``check``): under unit spacing a squared distance is an exact integer, so a value is one
correctly rounded FP64 square root, or an FP64 sum of fewer than 2^20 of them, rounded once to
float32: ``rtol = 2**-22`` (two float32 ulps), ``atol = 0``, NaN and ``+inf`` in place.
"""

import numpy as np
import torch

RTOL = 2.0 ** -22


def surface(mask):
    """Pixels of the bool ``[H, W]`` mask with a 4-neighbour outside it (the border is outside)."""
    p = np.pad(mask, 1)
    return mask & ~(p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:])


def directed(a, b, spacing):
    """For every surface pixel of mask ``a`` the distance to the nearest surface pixel of ``b``."""
    pa = np.argwhere(surface(a)).astype(np.float64) * spacing
    pb = np.argwhere(surface(b)).astype(np.float64) * spacing
    return np.sqrt(((pa[:, None, :] - pb[None, :, :]) ** 2).sum(-1)).min(1)


def oracle(pred, target, num_classes, include_background=False, metric="hausdorff", percentile=None, both=True,
           spacing=(1.0, 1.0)):
    """``[N, K]`` float64: ``metric`` "hausdorff" (``both`` False: directed) or "asd" (``both``: symmetric)."""
    pred, target = np.asarray(pred), np.asarray(target)
    classes = range(0 if include_background else 1, num_classes)
    out = np.empty((pred.shape[0], len(classes)))
    for i in range(pred.shape[0]):
        for k, c in enumerate(classes):
            a, b = pred[i] == c, target[i] == c
            if not a.any() or not b.any():
                out[i, k] = np.nan if a.any() == b.any() else np.inf
                continue
            d = [directed(a, b, spacing)] + ([directed(b, a, spacing)] if both else [])
            if metric == "asd":
                out[i, k] = sum(x.sum() for x in d) / sum(x.size for x in d)
            else:
                out[i, k] = max(x.max() if percentile is None else np.percentile(x, percentile) for x in d)
    return out


def check(got, want):
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    torch.testing.assert_close(got.double().cpu(), torch.from_numpy(want), rtol=RTOL, atol=0, equal_nan=True)


# ---------------------------------------------------------------- the cases both test files share
MAX_SIDE = 2048  # the native limit (kSurfMaxSide); tests/metrics/.../test_surface_distance.py holds it equal
MODES = {  # name -> (metric, percentile, both)
    "max": ("hausdorff", None, True), "p0": ("hausdorff", 0, True), "p50": ("hausdorff", 50, True),
    "p95": ("hausdorff", 95, True), "p100": ("hausdorff", 100, True), "directed": ("hausdorff", None, False),
    "assd": ("asd", None, True), "asd": ("asd", None, False),
}


def _hand():
    """(2, 5, 7), classes 0..3 with the background counted.  Image 0: class 0 fills the image but for
    the single pixels of class 1 (one in each map) and class 2 (target only: +inf); class 3 is nowhere
    (NaN).  Image 1: class 1 fills the prediction, so its surface is the image border, and the target
    but for a 3 x 3 block of class 3 (prediction absent: +inf); classes 0 and 2 are NaN."""
    p, t = torch.zeros(2, 5, 7, dtype=torch.int64), torch.zeros(2, 5, 7, dtype=torch.int64)
    p[0, 2, 3] = 1
    t[0, 1, 5], t[0, 4, 0] = 1, 2
    p[1], t[1] = 1, 1
    t[1, 1:4, 2:5] = 3
    return p, t, 4, True


def _far():
    """The longest search: it crosses two segment boundaries, over columns without any surface pixel."""
    p, t = torch.zeros(1, 70, 130, dtype=torch.int64), torch.zeros(1, 70, 130, dtype=torch.int64)
    p[0, 0, 0], t[0, 69, 129] = 1, 1
    return p, t, 2, False


def _random(w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 3, (2, 9, w), generator=g), torch.randint(0, 3, (2, 9, w), generator=g), 3, False


def _sparse(shape=(2, 37, 65), seed=7):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) < 0.02).long(), (torch.rand(shape, generator=g) < 0.02).long(), 2, False


def _rectangles():
    """Two filled 20 x 20 squares, the target's moved by (5, 10).  The farthest surface pixel of either
    is the corner pointing away from the other, and the nearest surface pixel of the other is its corner
    on the same diagonal, (5, 10) away: the Hausdorff distance is sqrt(125) in both directions."""
    p, t = torch.zeros(1, 40, 48, dtype=torch.int64), torch.zeros(1, 40, 48, dtype=torch.int64)
    p[0, 5:25, 6:26], t[0, 10:30, 16:36] = 1, 1
    return p, t, 2, False


def _too_wide():
    g = torch.Generator().manual_seed(9)
    shape = (1, 3, MAX_SIDE + 1)
    return torch.randint(0, 3, shape, generator=g), torch.randint(0, 3, shape, generator=g), 3, False


CASES = {
    "hand": _hand, "far": _far, "w63": lambda: _random(63, 1), "w64": lambda: _random(64, 2),
    "w65": lambda: _random(65, 3), "w129": lambda: _random(129, 4), "sparse": _sparse, "rectangles": _rectangles,
    "too_wide": _too_wide,
}
_cache = {}


def case(name, mode):
    """(input, target, num_classes, include_background, expected [N, K]) of a case, computed once."""
    if name not in _cache:
        _cache[name] = CASES[name]()
    if (name, mode) not in _cache:
        p, t, num_classes, background = _cache[name]
        metric, percentile, both = MODES[mode]
        _cache[name, mode] = oracle(p.numpy(), t.numpy(), num_classes, background, metric, percentile, both)
    return _cache[name] + (_cache[name, mode],)


def call(functional, mode):
    """(the package's functional for the mode, its keywords): ``functional`` is the module that has both."""
    metric, percentile, both = MODES[mode]
    if metric == "asd":
        return functional.average_surface_distance, {"symmetric": both}
    return functional.hausdorff_distance, {"percentile": percentile, "directed": not both}
