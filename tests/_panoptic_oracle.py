"""Panoptic quality exactly as docs/parity.md defines it: a dict loop over the pixels of each image, ints
for the counts and ``fractions.Fraction`` for ``iou_sum``; and the named cases both test files share.

Tolerances.  The counts are equal exactly.  ``iou_sum``: each matched pair carries one FP64 division
(<= 2^-53) and one rounding to the 2^-52 fixed point (<= 2^-53), and the finish launch adds N per-image
partials, so ``|got - exact| <= (tp + N) * 2^-52`` per class.  The float32 values: ``rtol = 2^-22`` (the
FP64 value rounded once to float32, 2^-24, with room for the FP64 mean), NaN in place.
"""

import collections
from fractions import Fraction

import numpy as np
import torch

from torcheval_amd.ops import panoptic as K

THINGS, STUFFS = (1, 2, 7), (0, 5)  # the classes are 0, 1, 2, 5, 7; every other category is unknown
S = K.SPAN
Case = collections.namedtuple("Case", "input target allow route dtypes", defaults=(False, "native", ("int32", "int64")))


def oracle(input, target, things=THINGS, stuffs=STUFFS, allow=False):
    """``input`` / ``target``: integer arrays ``[N, ..., 2]``.  Returns ``(iou_sum, tp, fp, fn)``, lists over
    the ascending classes of Fractions and ints.  Raises ``ValueError`` on an unknown input category."""
    cats = sorted(set(things) | set(stuffs))
    k = len(cats)
    iou_sum, tp, fp, fn = [Fraction(0)] * k, [0] * k, [0] * k, [0] * k

    def segment(pixel, is_input):
        c, i = int(pixel[0]), int(pixel[1])
        if c not in cats:
            if is_input and not allow:
                raise ValueError("unknown input category")
            return None  # void
        return (cats.index(c), i if c in things else 0)

    n = input.shape[0]
    for x, y in zip(input.reshape(n, -1, 2), target.reshape(n, -1, 2)):
        inter = collections.Counter((segment(a, True), segment(b, False)) for a, b in zip(x, y))
        area_p, area_t, matched_p, matched_t = collections.Counter(), collections.Counter(), set(), set()
        for (p, t), c in inter.items():
            area_p[p] += c
            area_t[t] += c
        for (p, t), c in inter.items():
            if p is None or t is None or p[0] != t[0]:
                continue
            union = area_p[p] - inter[p, None] + area_t[t] - c
            if 2 * c > union:
                tp[p[0]] += 1
                iou_sum[p[0]] += Fraction(c, union)
                matched_p.add(p)
                matched_t.add(t)
        for t in area_t:
            if t is not None and t not in matched_t and 2 * inter[None, t] <= area_t[t]:
                fn[t[0]] += 1
        for p in area_p:
            if p is not None and p not in matched_p and 2 * inter[p, None] <= area_p[p]:
                fp[p[0]] += 1
    return iou_sum, tp, fp, fn


def values(states):
    """float64 ``([K, 3] per class, [3] means)`` of ``(PQ, SQ, RQ)`` from the oracle's states, NaN in place."""
    iou_sum, tp, fp, fn = states
    rows = []
    for s, a, b, c in zip(iou_sum, tp, fp, fn):
        den = Fraction(2 * a + b + c, 2)
        rows.append([float(s / den) if den else np.nan, float(s / a) if a else np.nan, float(a / den) if den else np.nan])
    per_class = np.array(rows, dtype=np.float64)
    has = ~np.isnan(per_class)
    with np.errstate(invalid="ignore"):  # 0 / 0: no class has a denominator
        return per_class, np.where(has, per_class, 0.0).sum(0) / has.sum(0)


def check_values(got, want):
    torch.testing.assert_close(got.cpu().double(), torch.from_numpy(np.asarray(want)), rtol=2.0**-22, atol=0,
                               equal_nan=True)


def check_states(metric, states, images):
    iou_sum, tp, fp, fn = states
    assert metric.true_positives.tolist() == tp and metric.false_positives.tolist() == fp
    assert metric.false_negatives.tolist() == fn
    for got, exact, n in zip(metric.iou_sum.tolist(), iou_sum, tp):
        assert abs(Fraction(got) - exact) <= (n + images) * Fraction(1, 2**52), (got, float(exact))


# ---------------------------------------------------------------- the cases
def _fill(rng, pixels):
    """``[pixels, 2]``: runs of 1 .. 40 pixels of one (category, instance); category 9 is unknown."""
    runs = rng.integers(1, 41, size=pixels)
    rows = np.stack([rng.choice([0, 1, 2, 5, 7, 9], size=pixels), rng.integers(0, 3, size=pixels)], axis=1)
    return np.repeat(rows, runs, axis=0)[:pixels]


def _blobs(seed, shape, straddle=False):
    """Target runs, and as the input the same runs moved by three pixels, unknown categories made stuff."""
    rng = np.random.default_rng(seed)
    n, pixels = shape[0], int(np.prod(shape[1:]))
    t = np.stack([_fill(rng, pixels) for _ in range(n)])
    x = np.roll(t, 3, axis=1)
    x[..., 0][x[..., 0] == 9] = 0
    if straddle:  # one thing segment pair across the span edge (where the image reaches it)
        x[:, S - 6:S + 1], t[:, S - 4:S + 1] = (1, 77), (1, 78)
    return Case(x.reshape(*shape, 2), t.reshape(*shape, 2))


def _fullest(step):
    """S pixels, each its own thing instance on both sides; odd target pixels are of another class."""
    ids = np.arange(S, dtype=np.int64) * step
    x = np.stack([np.ones(S, dtype=np.int64), ids], axis=1)
    t = np.stack([1 + np.arange(S, dtype=np.int64) % 2, ids], axis=1)
    return Case(x.reshape(1, 1, S, 2), t.reshape(1, 1, S, 2))


def _flat(rows_x, rows_t, **kw):
    """A 4 x 4 image from 16 (category, instance) rows a side."""
    return Case(np.array(rows_x, dtype=np.int64).reshape(1, 4, 4, 2), np.array(rows_t, dtype=np.int64).reshape(1, 4, 4, 2),
                **kw)


def _iou_threshold(more):
    """Thing segments of 6 and 6 (or 7) pixels sharing 4 (or 5): 2 * 4 == 8 does not match, 2 * 5 > 8 does."""
    x = [(1, 3)] * 6 + [(0, 0)] * 10
    t = [(0, 0)] * (1 if more else 2) + [(1, 4)] * (7 if more else 6) + [(0, 0)] * 8
    return _flat(x, t)


def _void_share(side, more):
    """An unmatched thing segment of 4 pixels, 2 (or 3) of them on the other side's void: counted at
    exactly a half, not above.  The other side's void is an unknown category, allowed in the input."""
    seg = [(2, 1)] * 4 + [(0, 0)] * 12
    other = [(9, 0)] * (3 if more else 2) + [(0, 0)] * (13 if more else 14)
    return _flat(seg, other) if side == "p" else _flat(other, seg, allow=True)


def _stuff():
    """Two stuff blobs with different instance ids against one: a match (IoU 1) only as one segment."""
    x = [(5, 9)] * 4 + [(1, 1)] * 8 + [(5, 9)] * 4
    t = [(5, 1)] * 4 + [(1, 1)] * 8 + [(5, 2)] * 4
    return _flat(x, t)


def _unknown_target():
    """8 predicted pixels, 4 on the true segment and 4 on void: union 4 and a match; 8 without ``pvoid``."""
    x = [(7, 1)] * 8 + [(0, 0)] * 8
    t = [(7, 5)] * 4 + [(-3, 0)] * 4 + [(0, 0)] * 8
    return _flat(x, t)


def _unknown_input(allow):
    x = [(9, 1)] * 3 + [(1, 2)] * 5 + [(0, 0)] * 8
    t = [(1, 2)] * 8 + [(0, 0)] * 8
    return _flat(x, t, allow=allow, route="native" if allow else "raises")


def _instance(value):
    """A thing instance id the 32-bit key field cannot hold."""
    x = [(1, value)] * 8 + [(0, 0)] * 8
    return _flat(x, x, route="rerun", dtypes=("int64",))


def _over_capacity():
    """One segment more than the per-side capacity, one id per pixel."""
    ids = np.arange(K.MAX_SEGMENTS + 1, dtype=np.int64)
    x = np.stack([np.ones_like(ids), ids], axis=1).reshape(1, 1, -1, 2)
    return Case(x, x.copy(), route="rerun")


CASES = {
    "px1": lambda: _blobs(1, (1, 1, 1)), "px63": lambda: _blobs(2, (1, 1, 63)), "px65": lambda: _blobs(3, (1, 1, 65)),
    "span_m1": lambda: _blobs(4, (1, 1, S - 1), True), "span": lambda: _blobs(5, (1, 1, S), True),
    "span_p1": lambda: _blobs(6, (1, 1, S + 1), True), "images": lambda: _blobs(7, (2, 1, S + 1), True),
    "fullest_1": lambda: _fullest(1), "fullest_4096": lambda: _fullest(4096), "fullest_65536": lambda: _fullest(2**16),
    "iou_half": lambda: _iou_threshold(False), "iou_above": lambda: _iou_threshold(True),
    "void_half_p": lambda: _void_share("p", False), "void_above_p": lambda: _void_share("p", True),
    "void_half_t": lambda: _void_share("t", False), "void_above_t": lambda: _void_share("t", True),
    "stuff": _stuff, "unknown_target": _unknown_target,
    "unknown_input": lambda: _unknown_input(False), "unknown_input_allowed": lambda: _unknown_input(True),
    "instance_2p32": lambda: _instance(2**32), "instance_neg": lambda: _instance(-1),
    "over_capacity": _over_capacity,
}
# a GPU test item is a group: its cases and their dtypes run inside it
GROUPS = {
    "pixel_edges": ("px1", "px63", "px65"), "span_edges": ("span_m1", "span", "span_p1"), "image_edges": ("images",),
    "fullest_span": ("fullest_1", "fullest_4096", "fullest_65536"),
    "thresholds": ("iou_half", "iou_above", "void_half_p", "void_above_p", "void_half_t", "void_above_t"),
    "stuff": ("stuff",), "unknown_target": ("unknown_target",),
    "unknown_input": ("unknown_input", "unknown_input_allowed"), "instance_edges": ("instance_2p32", "instance_neg"),
    "over_capacity": ("over_capacity",),
}
assert sorted(n for g in GROUPS.values() for n in g) == sorted(CASES)
_cache = {}


def case(name):
    """(the case, the oracle's states or ``None`` where the call raises), computed once."""
    if name not in _cache:
        c = CASES[name]()
        _cache[name] = c, (None if c.route == "raises" else oracle(c.input, c.target, allow=c.allow))
    return _cache[name]


def tensors(c, dtype="int64", device="cpu"):
    dt = getattr(torch, dtype)
    return torch.from_numpy(c.input).to(device, dt), torch.from_numpy(c.target).to(device, dt)
