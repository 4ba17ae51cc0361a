"""The definition of ``kl_divergence`` (docs/parity.md, "Not in the reference") in numpy FP64.

``scipy.special.logsumexp`` and ``rel_entr`` do the arithmetic of ordinary rows; every special-value
rule is written out here and decided before they are called, never inherited from them.
"""

import numpy as np
from scipy.special import logsumexp, rel_entr


def row_logits(x: np.ndarray, t: np.ndarray) -> float:
    """KL(softmax(t) || softmax(x)) of one row pair."""
    x, t = np.asarray(x, dtype=np.float64), np.asarray(t, dtype=np.float64)
    if np.isnan(x).any() or np.isnan(t).any() or (x == np.inf).any() or (t == np.inf).any():
        return np.nan  # a NaN or +inf in either operand
    if (t == -np.inf).all() or (x == -np.inf).all():
        return np.nan  # a row that is all masked entries
    on = t != -np.inf  # p_j > 0; a term with p_j == 0 is 0 whatever x_j is
    if (x[on] == -np.inf).any():
        return np.inf  # q_j == 0 under p_j > 0
    lp = t[on] - logsumexp(t[on])
    lq = x[on] - logsumexp(x[x != -np.inf])
    return float(np.sum(np.exp(lp) * (lp - lq)))


def row_probs(x: np.ndarray, t: np.ndarray) -> float:
    """KL(t / sum t || x / sum x) of one row pair of weights."""
    x, t = np.asarray(x, dtype=np.float64), np.asarray(t, dtype=np.float64)
    if not (np.isfinite(x).all() and np.isfinite(t).all()) or (x < 0).any() or (t < 0).any():
        return np.nan  # a negative, NaN or infinite entry, also opposite t_j == 0
    if t.sum() == 0 or x.sum() == 0:
        return np.nan
    on = t > 0
    if (x[on] == 0).any():
        return np.inf
    return float(np.sum(rel_entr(t[on] / t.sum(), x[on] / x.sum())))


def special_rows(from_logits: bool, c: int, at: int, seed: int = 9, low: float = float(np.finfo(np.float32).min)):
    """One float32 row pair of ``c`` columns per special-value rule of the definition, the special
    entry at column ``at``: ``(name, input row, target row, expected value)``.  The expected value
    is the oracle's, and where the definition names it, it is asserted here.  ``low`` is the most
    negative finite value of the dtype the rows will be cast to, the usual fill of masked vocabulary
    entries: it is an ordinary finite logit, so its rows are finite (one of them about ``p_j |low|``)."""
    rng = np.random.default_rng(seed)
    if from_logits:
        bx, bt = rng.normal(size=c).astype(np.float32), rng.normal(size=c).astype(np.float32)
        off, f = -np.inf, row_logits
    else:
        bx, bt = (rng.random(c) + 0.1).astype(np.float32), (rng.random(c) + 0.1).astype(np.float32)
        off, f = 0.0, row_probs
    nan, inf, neg = np.nan, np.inf, -0.5
    rules = [
        # name, (column, value) pairs for the input, for the target, the named result (None: finite)
        ("p = 0 against q = 0", [(at, off)], [(at, off)], None),
        ("p = 0 alone", [], [(at, off)], None),
        ("q = 0 under mass", [(at, off)], [], inf),
        ("nan in input", [(at, nan)], [], nan),
        ("nan in target", [], [(at, nan)], nan),
        ("nan in input opposite p = 0", [(at, nan)], [(at, off)], nan),
        ("+inf in input", [(at, inf)], [], nan),
        ("+inf in target", [], [(at, inf)], nan),
        ("target without mass", [], [(None, off)], nan),
        ("input without mass", [(None, off)], [], nan),
        ("neither with mass", [(None, off)], [(None, off)], nan),
        ("nan and q = 0 under mass", [(at, off), ((at + 1) % c, nan)], [], nan),
    ]
    if from_logits:
        rules += [
            ("lowest finite value in target", [], [(at, low)], None),
            ("lowest finite value in input", [(at, low)], [], None),
            ("lowest finite value in both", [(at, low)], [(at, low)], None),
        ]
    else:
        rules += [
            ("negative target", [], [(at, neg)], nan),
            ("negative input", [(at, neg)], [], nan),
            ("negative input opposite p = 0", [(at, neg)], [(at, off)], nan),
        ]
    out = []
    for name, ex, et, named in rules:
        x, t = bx.copy(), bt.copy()
        for row, edits in ((x, ex), (t, et)):
            for col, v in edits:
                if col is None:
                    row[:] = v
                else:
                    row[col] = v
        want = f(x, t)
        if named is None:
            assert np.isfinite(want), name
        else:
            assert (np.isnan(want) and np.isnan(named)) or want == named, (name, want, named)
        out.append((name, x, t, want))
    return out


def rows(x: np.ndarray, t: np.ndarray, from_logits: bool, mask=None) -> np.ndarray:
    """FP64 row values in shape ``[...]`` of ``[..., C]`` operands, 0 for uncounted rows, which are
    not read."""
    x, t = np.asarray(x, dtype=np.float64), np.asarray(t, dtype=np.float64)
    lead = x.shape[:-1]
    x2, t2 = x.reshape(-1, x.shape[-1]), t.reshape(-1, x.shape[-1])
    m = np.ones(len(x2), dtype=bool) if mask is None else np.asarray(mask, dtype=bool).reshape(-1)
    f = row_logits if from_logits else row_probs
    return np.array([f(x2[i], t2[i]) if m[i] else 0.0 for i in range(len(x2))], dtype=np.float64).reshape(lead)


def value(x: np.ndarray, t: np.ndarray, from_logits: bool, mask=None, reduction: str = "mean"):
    """The FP64 result: the row values, their sum over the counted rows, or that sum divided by the
    number of counted rows (NaN when there are none)."""
    r = rows(x, t, from_logits, mask)
    if reduction == "none":
        return r
    count = r.size if mask is None else int(np.asarray(mask, dtype=bool).sum())
    total = float(r.sum())
    if reduction == "sum":
        return total
    return total / count if count > 0 else float("nan")
