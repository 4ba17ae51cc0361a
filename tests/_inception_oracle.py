"""The definition of ``inception_score`` (docs/parity.md, "Not in the reference") in numpy FP64.

``scipy.special.logsumexp`` does the arithmetic of ordinary rows; every special-value rule is written
out here and decided before it is called.  The partition is ``np.add.at`` on ``(first + i) mod S``,
and the value is formed from the three states alone.

``dyadic`` builds cases whose states are exact by construction: rows of ``0`` / ``-inf`` with ``2^t``
zeros at seeded columns, so every probability is ``2^-t`` and every row's negative entropy
``-t log 2``; the expected states come from the construction, never from a softmax.
"""

import numpy as np
from scipy.special import logsumexp


def row(x: np.ndarray):
    """``(p [C], h)`` of one row of logits: its softmax and its negative entropy."""
    x = np.asarray(x, dtype=np.float64)
    c = x.shape[0]
    if np.isnan(x).any() or (x == np.inf).any():
        return np.full(c, np.nan), np.nan  # a NaN or +inf logit
    on = x != -np.inf  # -inf: a masked class, p = 0 and term 0
    if not on.any():
        return np.full(c, np.nan), np.nan  # a row that is all masked classes
    lp = np.full(c, -np.inf)
    lp[on] = x[on] - logsumexp(x[on])
    p = np.exp(lp)
    return p, float(np.sum(p[on] * lp[on]))


def stats(x: np.ndarray, splits: int, first: int = 0):
    """``(prob_sum [S, C], neg_entropy_sum [S], num_rows [S])`` of ``[N, C]`` logits, row ``i`` in
    split ``(first + i) mod S``."""
    x = np.asarray(x, dtype=np.float64)
    n, c = x.shape
    p, h = np.zeros((n, c)), np.zeros(n)
    for i in range(n):
        p[i], h[i] = row(x[i])
    split = (first + np.arange(n)) % splits
    prob_sum, neg, rows = np.zeros((splits, c)), np.zeros(splits), np.zeros(splits)
    np.add.at(prob_sum, split, p)
    np.add.at(neg, split, h)
    np.add.at(rows, split, 1.0)
    return prob_sum, neg, rows


def values(prob_sum: np.ndarray, neg: np.ndarray, rows: np.ndarray):
    """``(split_log [S], mean, std)`` of the three states: NaN for a split without rows, the mean
    and the population standard deviation over the others (0 with one, NaN with none)."""
    splits = rows.shape[0]
    split_log = np.full(splits, np.nan)
    for s in range(splits):
        if rows[s] > 0:
            q = prob_sum[s] / rows[s]
            cross = 0.0
            for qj in q:  # j ascending; q_j == 0 adds 0
                cross += 0.0 if qj == 0 else qj * np.log(qj)
            split_log[s] = neg[s] / rows[s] - cross
    have = rows > 0
    if not have.any():
        return split_log, np.nan, np.nan
    v = np.exp(split_log[have])
    return split_log, float(np.mean(v)), float(np.std(v, ddof=0))


def score(x: np.ndarray, splits: int, first: int = 0):
    """``(mean, std)`` of ``[N, C]`` logits."""
    return values(*stats(x, splits, first))[1:]


def dyadic(n: int, c: int, splits: int, first: int, seed: int):
    """``(logits [N, C] float32, prob_sum, neg_entropy_sum, num_rows)``: row ``i`` holds ``0`` at
    ``2^t`` seeded columns (``0 <= t``, ``2^t <= C``, ``t`` seeded per row) and ``-inf`` elsewhere.
    The expected states are sums of ``2^-t`` (exact in FP64: at most ``2^31`` terms of at most 12
    bits below 1), ``-sum t log 2`` and the row counts."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, int(np.floor(np.log2(c))) + 1, size=n)
    order = rng.random((n, c)).argsort(axis=1).argsort(axis=1)  # a seeded permutation per row
    zero = order < (2**t)[:, None]
    # every second row reaches the last column: one of its zeros moves there
    move = (np.arange(n) % 2 == 1) & ~zero[:, c - 1]
    zero[move, zero[move].argmax(axis=1)] = False
    zero[move, c - 1] = True
    assert (zero.sum(axis=1) == 2**t).all()
    x = np.where(zero, np.float32(0.0), np.float32(-np.inf)).astype(np.float32)
    split = (first + np.arange(n)) % splits
    prob_sum, rows, tsum = np.zeros((splits, c)), np.zeros(splits), np.zeros(splits)
    np.add.at(prob_sum, split, zero * (2.0**-t)[:, None])
    np.add.at(rows, split, 1.0)
    np.add.at(tsum, split, t.astype(np.float64))  # integers: exact
    return x, prob_sum, -tsum * np.log(2.0), rows
