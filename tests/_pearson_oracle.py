"""The numpy FP64 oracle of Pearson and concordance correlation (docs/parity.md, "Not in the
reference"), shared by tests/metrics/regression/test_pearson.py and tests/gpu/test_k16_pearson.py.

It is the two-pass definition: subtract the FP64 mean, then sum.  Nothing of the metric's pivot
form or pairwise merge is in it.  ``floors`` is the a-priori error bound of any summation order of
each moment's own sum, ``n 2^-52 sum|term|``."""

import numpy as np

ROWS = ("n", "mean_x", "mean_y", "m2_x", "m2_y", "c_xy")


def _rows(v) -> np.ndarray:
    return np.atleast_2d(np.asarray(v, dtype=np.float64))


def moments(x, y) -> np.ndarray:
    """``[6, tasks]`` FP64 moments of ``[n]`` or ``[tasks, n]`` operands (zeros for ``n == 0``)."""
    x, y = _rows(x), _rows(y)
    tasks, n = x.shape
    out = np.zeros((6, tasks))
    if n == 0:
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        mx, my = x.sum(-1) / n, y.sum(-1) / n
        dx, dy = x - mx[:, None], y - my[:, None]
        out[:] = np.stack([np.full(tasks, float(n)), mx, my, (dx * dx).sum(-1), (dy * dy).sum(-1), (dx * dy).sum(-1)])
    # a constant operand has no spread, whatever the rounding of its mean
    out[3, (x == x[:, :1]).all(-1)] = 0.0
    out[4, (y == y[:, :1]).all(-1)] = 0.0
    return out


def floors(x, y) -> np.ndarray:
    """``[6, tasks]``: ``n 2^-52 sum|term|`` of each row's sum (means: of ``sum(v) / n``); 0 for n."""
    x, y = _rows(x), _rows(y)
    n = x.shape[1]
    m = moments(x, y)
    dx, dy = x - m[1][:, None], y - m[2][:, None]
    terms = np.stack([np.zeros(x.shape[0]), np.abs(x).sum(-1) / n, np.abs(y).sum(-1) / n, (dx * dx).sum(-1),
                      (dy * dy).sum(-1), np.abs(dx * dy).sum(-1)])
    return n * 2.0**-52 * terms


def _values(x, y, concordance: bool):
    x, y = _rows(x), _rows(y)
    n, mx, my, m2x, m2y, c = moments(x, y)
    with np.errstate(invalid="ignore", divide="ignore"):
        if concordance:
            num, den = 2.0 * c, m2x + m2y + n * (mx - my) ** 2
        else:
            num, den = c, np.sqrt(m2x * m2y)
        r = num / den
    if not concordance:
        r = np.clip(r, -1.0, 1.0)
    bad = (n < 2) | (den == 0) | ~np.isfinite(x).all(-1) | ~np.isfinite(y).all(-1)
    return np.where(bad, np.nan, r)


def pearson(x, y) -> np.ndarray:
    """FP64 ``[tasks]``; NaN for n < 2, a constant operand or a non-finite sample."""
    return _values(x, y, False)


def concordance(x, y) -> np.ndarray:
    return _values(x, y, True)
