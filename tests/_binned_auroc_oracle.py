"""The reference-default ``multiclass_binned_auroc`` (one value per sample) as the reference states it,
in numpy FP64, and the inputs on which the K4b kernel (csrc/kernels/binned_auroc.hip) and the ATen
form of ``_per_sample_binned_auroc`` are held to it.

Shared by tests/metrics/classification/test_per_sample_binned_auroc_oracle.py (the ATen form, CPU)
and tests/gpu/test_k4b_edges.py (the kernel).  Nothing here calls ``searchsorted`` or anything of
``torcheval_amd``: the oracle builds the [T, N, C] comparison the other two avoid.

Why the comparison is bit for bit.  tp is 0 or 1 and fp an integer below C, so the trapezoid is a
half-integer below 2^23 and the divisor ``tp_0 * fp_0`` an integer: both are exact in float32.  The
ATen form and the kernel divide them in float32, correctly rounded; the oracle divides in float64
and rounds to float32 once, and a float64 quotient of two float32 values rounded to float32 is the
correctly rounded float32 quotient (53 >= 2 * 24 + 2).  So all three give the same bits.

The scores lie on the grid of eighths from -1/8 to 9/8 and so do the thresholds, so that scores equal
thresholds all the time: that is where the direction of each comparison (``>=`` or ``>``) shows.
+inf, -inf, NaN and -0.0 are sprayed over the scores at a few percent each.
"""

import zlib
from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np
import torch

_BOOL_BUDGET = 1 << 24  # elements of the [T, rows, C] tensor of one chunk


def per_sample_binned_auroc_fp64(x, y, thr) -> torch.Tensor:
    """float32 [N]: reference binned_auroc.py:196-213 with ``average=None``.  ``x`` [N, C] scores,
    ``y`` [N] labels in [0, C), ``thr`` [T] ascending thresholds."""
    x = np.asarray(torch.as_tensor(x).detach().cpu().to(torch.float64).numpy())
    y = np.asarray(torch.as_tensor(y).detach().cpu().to(torch.int64).numpy())
    thr = np.asarray(torch.as_tensor(thr).detach().cpu().to(torch.float64).numpy())
    n, c = x.shape
    T = thr.shape[0]
    assert y.shape == (n,) and T >= 1 and (n == 0 or (y.min() >= 0 and y.max() < c))
    out = np.empty(n, dtype=np.float64)
    step = max(1, _BOOL_BUDGET // (T * c))
    for s in range(0, n, step):
        xs, ys = x[s:s + step], y[s:s + step]
        rows = xs.shape[0]
        with np.errstate(invalid="ignore"):
            ge = xs[None, :, :] >= thr[:, None, None]  # [T, rows, C]; NaN compares false
        true = np.arange(c)[None, :] == ys[:, None]  # the one-hot target
        tp = (ge & true[None]).sum(-1).astype(np.float64)  # [T, rows]
        fp = ge.sum(-1).astype(np.float64) - tp
        # descending thresholds behind a leading zero point, as rot90 + pad build it there
        zero = np.zeros((1, rows), dtype=np.float64)
        tpd = np.concatenate([zero, tp[::-1]], 0)
        fpd = np.concatenate([zero, fp[::-1]], 0)
        area = ((fpd[1:] - fpd[:-1]) * (tpd[1:] + tpd[:-1])).sum(0) / 2.0
        factor = tp[0] * fp[0]
        out[s:s + rows] = np.where(factor == 0, 0.5, area / np.where(factor == 0, 1.0, factor))
    return torch.from_numpy(out.astype(np.float32))


# ------------------------------------------------------------------ inputs
GRID = tuple(k / 8.0 for k in range(-1, 10))  # -1/8, 0, 1/8, ..., 9/8
SPRAY = ((float("inf"), 0.05), (float("-inf"), 0.03), (float("nan"), 0.03), (-0.0, 0.03))

THRESHOLDS: Dict[str, Tuple[float, ...]] = {
    "dup6": (0.0, 0.25, 0.25, 0.5, 0.875, 1.0),
    "dup5": (0.125, 0.5, 0.5, 0.5, 0.75),
    "zero": (0.0,),
    "one": (1.0,),
    "ends": (0.0, 1.0),
}
LINSPACE_T = (2, 3, 4, 9)  # the default thresholds, torch.linspace(0, 1, T)
THRESHOLD_SETS = tuple(THRESHOLDS) + tuple(f"lin{t}" for t in LINSPACE_T)


def thresholds(name: str) -> torch.Tensor:
    """float32 [T].  ``lin<T>`` is ``torch.linspace(0, 1, T)`` itself: exact eighths for T in {2, 3, 9};
    the two inner thresholds of T = 4 are thirds, which no score equals."""
    if name.startswith("lin"):
        t = torch.linspace(0, 1, int(name[3:]))
        if int(name[3:]) != 4:
            assert all(float(v) * 8 == round(float(v) * 8) for v in t), name
        return t
    return torch.tensor(THRESHOLDS[name], dtype=torch.float32)


def _gen(key: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(key.encode()))


def grid_scores(n: int, c: int, key: str, spray: bool = True) -> torch.Tensor:
    """float32 [n, c] on the grid of eighths, with the special values sprayed over it."""
    g = _gen("scores-" + key)
    grid = torch.tensor(GRID, dtype=torch.float32)
    x = grid[torch.randint(0, len(GRID), (n, c), generator=g)]
    if spray:
        u = torch.rand(n, c, generator=g)
        edge = 0.0
        for value, share in SPRAY:
            x[(u >= edge) & (u < edge + share)] = value
            edge += share
    return x


# widths at both edges of every G arm of launch_sample_binned_auroc (G lanes per sample, 4 columns
# per lane and pass); 5, 17, 33, 65, 129, 257: C % 4 == 1; 18: C % 4 == 2; 515: C % 4 == 3 on a third pass
ARMS: Dict[str, Tuple[int, ...]] = {
    "narrow": (2, 3),
    "g4": (4, 5, 16),
    "g8": (17, 18, 32),
    "g16": (33, 64),
    "g32": (65, 128),
    "g64": (129, 256, 257, 515),
}
WIDTHS = tuple(c for cs in ARMS.values() for c in cs)
NS = (1, 8, 9, 257)
# where the true class goes: anywhere, column 0, column C - 1, column C - 4 (the first column of the
# shifted tail load when C % 4 != 0, whose first 4 - C % 4 values repeat columns already counted)
PATTERNS = ("random", "first", "last", "tail")
LABEL_DTYPES = (torch.int64, torch.int32)
SMALL_LABEL_WIDTH = 18  # the one width that also runs int16 labels, through the wrapper's .long()


@dataclass(frozen=True)
class Case:
    id: str
    n: int
    c: int
    thr: str
    pattern: str
    label_dtype: torch.dtype

    def tensors(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """CPU ``x`` float32 [n, c], ``y`` [n] in the case's label dtype, ``thr`` float32 [T]."""
        x = grid_scores(self.n, self.c, self.id)
        if self.pattern == "random":
            y = torch.randint(0, self.c, (self.n,), generator=_gen("labels-" + self.id))
        else:
            col = {"first": 0, "last": self.c - 1, "tail": max(self.c - 4, 0)}[self.pattern]
            y = torch.full((self.n,), col, dtype=torch.int64)
        return x, y.to(self.label_dtype), thresholds(self.thr)


def cases_for(c: int) -> List[Case]:
    """Every n with every threshold set at width ``c``; the label pattern and dtype rotate over them
    (in steps of 5, coprime to the number of pairs) so that every (pattern, dtype) pair comes up and
    each n meets every pattern and every dtype."""
    dtypes = LABEL_DTYPES + ((torch.int16,) if c == SMALL_LABEL_WIDTH else ())
    pairs = [(p, d) for p in PATTERNS for d in dtypes]
    out = []
    for n in NS:
        for name in THRESHOLD_SETS:
            p, d = pairs[5 * len(out) % len(pairs)]
            dn = str(d).replace("torch.", "")
            out.append(Case(f"c{c}-n{n}-{name}-{p}-{dn}", n, c, name, p, d))
    return out


def all_cases() -> List[Case]:
    return [case for c in WIDTHS for case in cases_for(c)]


def mismatches(got: torch.Tensor, want: torch.Tensor) -> List[int]:
    """The rows whose float32 bits differ (no result is ever NaN)."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype == torch.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    return (got.view(torch.int32) != want.view(torch.int32)).nonzero().reshape(-1).tolist()


def describe(case_id: str, x: torch.Tensor, y: torch.Tensor, got: torch.Tensor, want: torch.Tensor) -> List[str]:
    """One line per mismatching row: the case, the row, both values and whether the row holds +inf."""
    out = []
    for r in mismatches(got, want):
        inf = bool((x[r] == float("inf")).any())
        out.append(f"{case_id} row {r} label {int(y[r])}: got {float(got[r])!r} want {float(want[r])!r}"
                   f"{' (+inf in row)' if inf else ''}")
    return out


def report(bad: List[str]) -> str:
    """What a failing comparison prints: the counts, then the first lines of ``describe``."""
    finite = [b for b in bad if not b.endswith("(+inf in row)")]
    return (f"{len(bad)} rows differ, {len(finite)} of them in rows without +inf; the first of those: {finite[:4]}; "
            f"the first of all: {bad[:4]}")
