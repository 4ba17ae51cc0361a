"""Inputs and the plain float64 oracle of K2 (multilabel / top-k multilabel counts).

Shared by tests/metrics/classification/test_k2_oracle.py (CPU) and tests/gpu/test_k2_multilabel.py.
Nothing here calls the package.

The top-k rule (docs/parity.md): scores rank by value with ``-0.0 == +0.0``; every NaN, of any sign
or payload, ranks above ``+inf`` and all NaNs are equal; among equal scores the lowest column index
wins.  That is the first ``k`` indices of a stable descending float64 sort, which ``topk_pred``
takes literally.  ``signed_zero_model_pred`` and ``highest_index_model_pred`` are two wrong rules
(the kernel before its zero fix, and ties to the highest index); they exist only to show that the
fixtures tell the rule from them.
"""

import torch

from tests._threshold_edges import CRITERIA, multilabel_targets

SCORE_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
TARGET_DTYPES = (torch.float32, torch.int64, torch.int32, torch.uint8, torch.bool)
N_ROWS = 13  # rows of the op-level fixtures: every target pattern of k2_targets is present

# 16-bit patterns: (quiet NaN, negative quiet NaN, signalling NaN, +inf, -inf, +0, -0, smallest
# denormal, largest finite); the float32 ones are those of the issue
_SPECIAL_BITS = {
    torch.float32: (0x7FC00000, 0xFFC00000, 0x7F800001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000,
                    0x00000001, 0x7F7FFFFF),
    torch.bfloat16: (0x7FC0, 0xFFC0, 0x7F81, 0x7F80, 0xFF80, 0x0000, 0x8000, 0x0001, 0x7F7F),
    torch.float16: (0x7E00, 0xFE00, 0x7C01, 0x7C00, 0xFC00, 0x0000, 0x8000, 0x0001, 0x7BFF),
}
_NAN_BITS = {dt: b[:3] for dt, b in _SPECIAL_BITS.items()}
# positive finite patterns of the 16-bit dtypes: 0 .. _MAX_FINITE16 (negatives: the same | 0x8000)
_MAX_FINITE16 = {torch.bfloat16: 0x7F7F, torch.float16: 0x7BFF}


def _from_bits(bits: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """int64 bit patterns -> ``dtype``, bit for bit (no arithmetic touches a signalling NaN)."""
    width, idt = (32, torch.int32) if dtype == torch.float32 else (16, torch.int16)
    bits = bits & ((1 << width) - 1)
    bits = torch.where(bits >= (1 << (width - 1)), bits - (1 << width), bits)  # two's complement
    return bits.to(idt).view(dtype)


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _row_perms(n: int, m: int, c: int, g: torch.Generator) -> torch.Tensor:
    """[n, c] int64: per row, the first c entries of a random permutation of range(m)."""
    return torch.rand(n, m, generator=g, dtype=torch.float64).argsort(dim=1)[:, :c]


# ------------------------------------------------------------------ the rule and the two wrong models
def _pred_from_order(key: torch.Tensor, k: int) -> torch.Tensor:
    idx = torch.sort(key, dim=-1, descending=True, stable=True).indices[:, :k]
    return torch.zeros(key.shape, dtype=torch.int64).scatter_(1, idx, 1)


def topk_pred(x: torch.Tensor, k: int) -> torch.Tensor:
    """The rule, as an int64 {0, 1} matrix [n, c] with k ones per row."""
    assert x.device.type == "cpu" and x.dim() == 2 and 1 <= k <= x.shape[1]
    return _pred_from_order(x.double(), k)


def signed_zero_model_pred(x: torch.Tensor, k: int) -> torch.Tensor:
    """The same sort with -0.0 ranked below +0.0 (above every negative value)."""
    d = x.double()
    neg_zero = (d == 0) & torch.signbit(d)
    # -1e-300 lies between -0.0 and the smallest negative denormal of every score dtype
    return _pred_from_order(torch.where(neg_zero, torch.full_like(d, -1e-300), d), k)


def highest_index_model_pred(x: torch.Tensor, k: int) -> torch.Tensor:
    """Ties go to the highest index: the rule applied to the columns in reverse order."""
    return _pred_from_order(x.double().flip(1), k).flip(1)


def counts(pred: torch.Tensor, target: torch.Tensor, criteria: str) -> int:
    """The correct count of ``_multilabel_update``, in float64, as a Python int."""
    p, t = pred.double(), target.double()
    if criteria == "hamming":
        return int((p == t).sum())
    if criteria == "exact_match":
        return int((p == t).all(dim=1).sum())
    if criteria == "overlap":
        both_pos = ((p == t) & (p == 1)).any(dim=1)
        both_empty = ((p == 0) & (t == 0)).all(dim=1)
        return int(both_pos.sum()) + int(both_empty.sum())
    if criteria == "contain":
        return int(((p - t) >= 0).all(dim=1).sum())
    if criteria == "belong":
        return int(((p - t) <= 0).all(dim=1).sum())
    raise ValueError(criteria)


def total(target: torch.Tensor, criteria: str) -> int:
    return target.numel() if criteria == "hamming" else target.shape[0]


def all_counts(pred: torch.Tensor, target: torch.Tensor) -> dict:
    return {crit: counts(pred, target, crit) for crit in CRITERIA}


def boundary_tied(x: torch.Tensor, k: int) -> torch.Tensor:
    """bool [n]: sorted[k-1] == sorted[k] (NaNs equal, zeros equal); all False at k == c."""
    if k >= x.shape[1]:
        return torch.zeros(x.shape[0], dtype=torch.bool)
    s = torch.sort(x.double(), dim=-1, descending=True, stable=True).values
    a, b = s[:, k - 1], s[:, k]
    return (a == b) | (a.isnan() & b.isnan())


# ------------------------------------------------------------------ scores
def tie_free_rows(dtype: torch.dtype, n: int, c: int, seed: int) -> torch.Tensor:
    """[n, c] scores, distinct within each row by construction.  float32: a per-row draw without
    replacement from 4c multiples of 0.375 that straddle zero.  bf16 / f16: a per-row draw without
    replacement from the dtype's finite bit patterns (denormals included, -0 left out).  Rows 1, 2
    and 3 get one NaN, one +inf and one -inf at a random column."""
    g = _gen(seed)
    if dtype == torch.float32:
        x = ((_row_perms(n, 4 * c, c, g) - 2 * c).double() * 0.375).to(dtype)
    else:
        npos = _MAX_FINITE16[dtype] + 1  # 0 .. max finite
        assert c <= 2 * npos - 1
        p = _row_perms(n, 2 * npos - 1, c, g)
        bits = torch.where(p < npos, p, (p - npos + 1) | 0x8000)  # negatives start at -denormal: no -0
        x = _from_bits(bits, dtype).clone()
    col = torch.randint(0, c, (3,), generator=g)
    nan, pinf, ninf = _SPECIAL_BITS[dtype][0], _SPECIAL_BITS[dtype][3], _SPECIAL_BITS[dtype][4]
    for row, bits in ((1, nan), (2, pinf), (3, ninf)):
        if row < n:
            x[row, col[row - 1]] = _from_bits(torch.tensor(bits), dtype)
    return x


def _tie_boundary(x: torch.Tensor, k: int, rows: torch.Tensor) -> torch.Tensor:
    """In ``rows``, raise the score of rank k to the score of rank k-1 (the order stays valid), so
    that the k-th and the (k+1)-th score are equal."""
    if k >= x.shape[1]:
        return x
    idx = torch.sort(x.double(), dim=-1, descending=True, stable=True).indices
    r = rows.nonzero().flatten()
    x = x.clone()
    x[r, idx[r, k]] = x[r, idx[r, k - 1]]
    return x


def tie_rows(dtype: torch.dtype, n: int, c: int, k: int, seed: int) -> torch.Tensor:
    """[n, c] scores drawn from {-1, 0, 1, 2}.  Three rows in four (all but row % 4 == 3) are tied
    across the rank-k boundary by construction; the rest are as drawn."""
    g = _gen(seed)
    x = (torch.randint(0, 4, (n, c), generator=g) - 1).to(dtype)
    return _tie_boundary(x, k, torch.arange(n) % 4 != 3)


def special_rows(dtype: torch.dtype, n: int, c: int, k: int, seed: int) -> torch.Tensor:
    """[n, c] rows of special values, by row % 13:
    0, 2   only +-0.0 in alternating order (starting with -0.0, with +0.0)
    1, 7   the special patterns (three NaN kinds, +-inf, +-0, smallest denormal, largest finite),
           tiled and shuffled
    3, 12  one repeated value (1.0, -0.0)
    4      NaNs only, of the three kinds
    5, 9   k - 1 NaNs (fewer than k), the rest from {-1, +-0, 1} tied across the boundary
    6, 11  min(k + 1, c) NaNs (more than k) of shuffled kinds, the rest distinct
    8      +-0.0 and +- the smallest denormal, shuffled
    10     the special patterns in their listed order, tiled
    """
    g = _gen(seed)
    sp = torch.tensor(_SPECIAL_BITS[dtype])
    nan = torch.tensor(_NAN_BITS[dtype])
    pz, nz, den = sp[5], sp[6], sp[7]
    sign = int(nz)
    bits = torch.zeros(n, c, dtype=torch.int64)
    cols = torch.arange(c)
    one = int(torch.ones((), dtype=dtype).view(torch.int32 if dtype == torch.float32 else torch.int16)) & 0xFFFFFFFF

    def shuffled(v):
        return v[torch.randperm(v.numel(), generator=g)]

    def tiled(v):
        return v.repeat(c // v.numel() + 1)[:c]

    for r in range(n):
        m = r % 13
        if m in (0, 2):
            bits[r] = torch.where(cols % 2 == (0 if m == 0 else 1), nz, pz)
        elif m in (1, 7):
            bits[r] = shuffled(tiled(sp))
        elif m == 3:
            bits[r] = one
        elif m == 12:
            bits[r] = nz
        elif m == 4:
            bits[r] = shuffled(tiled(nan))
        elif m in (5, 9):
            vals = torch.tensor([one | sign, int(pz), int(nz), one])  # -1, +0, -0, 1
            row = vals[torch.randint(0, 4, (c,), generator=g)]
            row[torch.randperm(c, generator=g)[: k - 1]] = shuffled(tiled(nan))[: k - 1]
            bits[r] = row
        elif m in (6, 11):
            row = one + 1 + torch.randperm(4 * c, generator=g)[:c]  # distinct values above 1.0
            m_nan = min(k + 1, c)
            row[torch.randperm(c, generator=g)[:m_nan]] = shuffled(tiled(nan))[:m_nan]
            bits[r] = row
        elif m == 8:
            bits[r] = shuffled(tiled(torch.stack([pz, nz, den, den | sign])))
        else:
            bits[r] = tiled(sp)
    x = _from_bits(bits, dtype).clone()
    tie = torch.tensor([r % 13 in (5, 9) for r in range(n)])
    if k > 1:  # rows 5, 9: tie the boundary below the NaNs (at k == 1 they hold no NaN at all)
        x = _tie_boundary(x, k, tie)
    return x


# ------------------------------------------------------------------ targets
def k2_targets(pred: torch.Tensor, seed: int, dtype: torch.dtype = torch.int64) -> torch.Tensor:
    """``multilabel_targets`` (rows equal to ``pred``, rows one label off, random rows) with three
    rows pinned so that no criterion is at its floor or ceiling: row 4 drops one predicted label
    (contain holds, belong fails), row 8 adds one label that was not predicted (belong holds,
    contain fails; impossible when every label is predicted), row 12 is the complement of
    ``pred`` (no overlap).  Rows 0, 2, 6, 10, ... equal ``pred`` and satisfy every criterion."""
    t = multilabel_targets(pred, seed, torch.int64)
    n, c = t.shape
    g = _gen(seed + 5000)
    pick = torch.rand(n, c, generator=g, dtype=torch.float64)
    if n > 4 and pred[4].any():
        t[4] = pred[4]
        t[4, (pick[4] * pred[4]).argmax()] = 0
    if n > 8 and not pred[8].all():
        t[8] = pred[8]
        t[8, (pick[8] * (1 - pred[8])).argmax()] = 1
    if n > 12:
        t[12] = 1 - pred[12]
    return t.to(dtype)


_ODD_VALUES = {
    torch.int64: [-1, 0, 1, 2],
    torch.int32: [-1, 0, 1, 2],
    torch.uint8: [0, 1, 2, 255],
    torch.float32: [0.0, 0.5, 1.0, -0.0, float("nan")],
}


def odd_targets(pred: torch.Tensor, seed: int, dtype: torch.dtype) -> torch.Tensor:
    """``k2_targets`` with values outside {0, 1}: in rows 1 and 3 (mod 4) half of the entries are
    drawn from the dtype's value set; row 2 turns one predicted label into the set's last value
    (2, 255, NaN) and row 6 one unpredicted label into its first non-binary one (-1, 2, 0.5)."""
    vals = torch.tensor(_ODD_VALUES[dtype], dtype=torch.float64)
    t = k2_targets(pred, seed, torch.int64).double()
    n, c = t.shape
    g = _gen(seed + 6000)
    draw = vals[torch.randint(0, vals.numel(), (n, c), generator=g)]
    swap = (torch.rand(n, c, generator=g, dtype=torch.float64) < 0.5) & (torch.arange(n) % 2 == 1)[:, None]
    t = torch.where(swap, draw, t)
    pick = torch.rand(n, c, generator=g, dtype=torch.float64)
    if n > 2 and pred[2].any():
        t[2, (pick[2] * pred[2]).argmax()] = vals[-1]
    if n > 6 and not pred[6].all():
        first = next(v for v in _ODD_VALUES[dtype] if v not in (0, 1))
        t[6, (pick[6] * (1 - pred[6])).argmax()] = first
    if dtype == torch.uint8:
        return t.to(torch.int64).to(dtype)
    return t.to(dtype)


# ------------------------------------------------------------------ the dispatch of launch_kinds
def topk_arm(c: int, vec: bool) -> str:
    """The top-k template arm that ``launch_kinds`` selects for ``c`` columns: ``topk_R<R>`` is
    ``ml_topk_kernel<.., R>``, ``topk_vec_RV<RV>`` is ``ml_topk_vec_kernel<.., RV>``."""
    if vec and c % 4 == 0 and c <= 2048:
        rv = -(-c // 256)
        return f"topk_vec_RV{1 if rv <= 1 else 2 if rv <= 2 else 4 if rv <= 4 else 8}"
    r = -(-c // 64)
    return f"topk_R{4 if r <= 4 else 8 if r <= 8 else 16 if r <= 16 else 32}"


def ks_for(c: int):
    """k from {1, 2, 3, c // 2, c - 1, c}, clipped to 1 <= k <= c, deduplicated, in order."""
    out = []
    for k in (1, 2, 3, c // 2, c - 1, c):
        k = min(max(k, 1), c)
        if k not in out:
            out.append(k)
    return out


# ------------------------------------------------------------------ the op-level top-k cases
# c of the scalar arms (R = 4, 8, 16, 32 values per lane), of the scalar arms reached through a
# misaligned view of a c % 4 == 0 row, and of the vectorised arms (RV = 1, 2, 4, 8)
SCALAR_C = (1, 3, 65, 255, 257, 511, 513, 1023, 1025, 2047)
VIEW_C = (256, 2048)
VEC_C = (4, 256, 260, 512, 516, 1024, 1028, 2048)
FIXTURES = ("tie_free", "tie", "special")


def fixture(kind: str, dtype: torch.dtype, c: int, k: int, n: int = N_ROWS) -> torch.Tensor:
    """The [n, c] scores of one op-level case; the seed depends on (c, k) only."""
    seed = 7919 * c + 31 * k
    if kind == "tie_free":
        return tie_free_rows(dtype, n, c, seed)
    if kind == "tie":
        return tie_rows(dtype, n, c, k, seed + 1)
    if kind == "special":
        return special_rows(dtype, n, c, k, seed + 2)
    raise ValueError(kind)
