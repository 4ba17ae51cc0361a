"""Oracles and error bounds shared by the K25 tests (tests/metrics/clustering/test_contingency.py,
tests/gpu/test_k25_contingency.py): the contingency table by ``np.add.at``, every index from Python
integers, ``Fraction`` and ``math.fsum``, and the expected mutual information from exact rational
hypergeometric probabilities.

Bounds, with ``U = 2^-53``, for the forms that K25 and the ATen form share:

* A sum ``S = sum x log x`` of ``k`` positive terms carries at most ``(k + 20) U S``: two roundings per
  term, one per addition of the longest chain (at most ``k``, whatever the grouping) and the wave
  butterfly; ``E(S)`` below.
* ``H = log N - S / N``: ``E(S) / N + 4 U log N``.
* ``MI = ((S_n - S_a) - S_b) / N + log N``: ``(E(S_n) + E(S_a) + E(S_b)) / N + 12 U log N`` (four operations
  on intermediates of at most ``3 log N``).  Absolute, so it also holds where MI is near 0.
* A quotient ``x / y`` with absolute errors ``e_x``, ``e_y``: ``(e_x + |x / y| e_y) / (|y| - e_y) + 2 U |x / y|``.
* Rand is one division of exact integers: ``4 U``.  ARI's numerator and denominator are exact integers
  converted with at most three roundings each: ``8 U`` absolute (``|ARI| <= 1``).  FMI is two quotients of
  converted integers, two square roots and a product: ``10 U``.

Every bound is doubled where the other side of a comparison is FP64 too.
"""

import math
from fractions import Fraction

import numpy as np

U = 2.0**-53
EPS = 2.0**-52
METHODS = ("min", "geometric", "arithmetic", "max")


def table_of(labels_true, labels_pred, r, c):
    """int64 [r, c] by np.add.at; pairs with a label outside its range are left out."""
    t, p = np.asarray(labels_true, dtype=np.int64), np.asarray(labels_pred, dtype=np.int64)
    ok = (t >= 0) & (t < r) & (p >= 0) & (p < c)
    out = np.zeros((r, c), dtype=np.int64)
    np.add.at(out, (t[ok], p[ok]), 1)
    return out


def pair_sums(table):
    """Python integers: sum n (n - 1) / 2 over the cells, the rows and the columns, and N."""
    rows = [[int(v) for v in row] for row in np.asarray(table)]
    a = [sum(row) for row in rows]
    b = [sum(col) for col in zip(*rows)]
    half = lambda xs: sum(x * (x - 1) // 2 for x in xs)  # noqa: E731
    return half([v for row in rows for v in row]), half(a), half(b), sum(a)


def pair_bounds_f64(table):
    """{rand, adjusted_rand, fowlkes_mallows: absolute bound} for the ATen form's FP64 pair sums (totals of
    2^32 or more).  With A = N (N - 1) / 2, a sum of k terms x (x - 1) / 2 carries (k + 4) U of itself (two
    roundings per term, one conversion, one per addition), so each of tp, fp, fn, tn is off by at most
    d = 4 (K + 4) U A with K the number of cells.  Rand = (tn + tp) / A: 2 d / A + 4 U.  ARI = 2 (tp tn -
    fn fp) / D with D the denominator: the numerator moves by at most 2 d A, D by at most 4 d A, and
    |ARI| <= 1: 12 d A / D + 8 U.  FMI = P / sqrt(Pa Pb): FMI (d / P + d / (2 Pa) + d / (2 Pb)) + 10 U."""
    P, Pa, Pb, N = pair_sums(table)
    A = N * (N - 1) // 2
    tp, fp, fn = P, Pb - P, Pa - P
    tn = A - tp - fp - fn
    D = (tp + fn) * (fn + tn) + (tp + fp) * (fp + tn)
    d = 4 * (np.asarray(table).size + 4) * U * A
    fmi = P / math.sqrt(Pa * Pb) if P else 0.0
    return {"rand": 2 * d / A + 4 * U,
            "adjusted_rand": (12 * d * A / D if D else 0.0) + 8 * U,
            "fowlkes_mallows": (fmi * (d / P + d / (2 * Pa) + d / (2 * Pb)) if P else 0.0) + 10 * U}


def emi_oracle(a, b):
    """(EMI, sum of |terms|) for marginals a, b (Python ints, one total): exact hypergeometric
    probabilities as Fractions (the first from math.comb, the rest by the exact ratio), the terms
    through math.fsum."""
    n_total = sum(a)
    assert n_total == sum(b)
    terms = []
    for ai in a:
        for bj in b:
            if ai == 0 or bj == 0:
                continue
            lo, hi = max(1, ai + bj - n_total), min(ai, bj)
            p = Fraction(math.comb(ai, lo) * math.comb(n_total - ai, bj - lo), math.comb(n_total, bj))
            for n in range(lo, hi + 1):
                weight = float(Fraction(n, n_total) * p)
                if weight != 0.0:
                    terms.append(weight * math.log(Fraction(n_total * n, ai * bj)))
                p *= Fraction((ai - n) * (bj - n), (n + 1) * (n_total - ai - bj + n + 1))
    return math.fsum(terms), math.fsum(abs(t) for t in terms)


def emi_ceiling(n_total):
    """The model's ceiling of |EMI - oracle| / sum |term|: nine lgammas of a few ulp each at the
    magnitude of lgamma(N + 1); never below a few roundings of the sum itself."""
    return 64 * U * max(1.0, math.lgamma(n_total + 1))


def emi_bound(n_total, mag):
    """Absolute bound of a computed EMI whose terms sum to `mag` in magnitude: the ceiling's share, and
    the roundings of the log factor ``log n + (log N - log a - log b)`` (three logs and three additions
    at the magnitude of log N: 6 U log N per term) times the terms' weights ``(n / N) p(n)``, which sum to
    ``sum_ij a_i b_j / N^2 <= 1``."""
    return emi_ceiling(n_total) * mag + 6 * U * math.log(max(n_total, 2))


def _xlogx(xs):
    return math.fsum(x * math.log(x) for x in xs if x > 0)


def values_oracle(table, emi=None):
    """{name: value} and {name: bound} of every index of the table, sklearn 1.7.2's conventions;
    NMI / AMI / normalizer as 4-lists in the order of METHODS.  `emi` = (value, absolute error) adds
    EMI and AMI."""
    t = np.asarray(table)
    cells = [int(v) for v in t.reshape(-1)]
    a = [int(v) for v in t.sum(axis=1)]
    b = [int(v) for v in t.sum(axis=0)]
    P, Pa, Pb, N = pair_sums(t)
    names = ["rand", "adjusted_rand", "fowlkes_mallows", "entropy_true", "entropy_pred", "mutual_info",
             "homogeneity", "completeness"]
    if N == 0:
        nan4 = [math.nan] * 4
        v = {k: math.nan for k in names}
        v.update(normalizer=nan4, normalized_mutual_info=nan4, adjusted_mutual_info=nan4,
                 expected_mutual_info=math.nan)
        return v, {k: ([0.0] * 4 if isinstance(x, list) else 0.0) for k, x in v.items()}
    T = N * (N - 1)
    tp, fp, fn = 2 * P, 2 * (Pb - P), 2 * (Pa - P)
    tn = T - tp - fp - fn
    v, e = {}, {}
    v["rand"] = 1.0 if (tn + tp == T or T == 0) else float(Fraction(tn + tp, T))
    e["rand"] = 4 * U
    if fn == 0 and fp == 0:
        v["adjusted_rand"] = 1.0
    else:
        v["adjusted_rand"] = float(Fraction(2 * (tp * tn - fn * fp), (tp + fn) * (fn + tn) + (tp + fp) * (fp + tn)))
    e["adjusted_rand"] = 8 * U
    v["fowlkes_mallows"] = math.sqrt(Fraction(P, Pb)) * math.sqrt(Fraction(P, Pa)) if P != 0 else 0.0
    e["fowlkes_mallows"] = 10 * U

    rows, cols = sum(x > 0 for x in a), sum(x > 0 for x in b)
    log_n = math.log(N)
    s_n, s_a, s_b = _xlogx(cells), _xlogx(a), _xlogx(b)

    def err_s(s, k):
        return (k + 20) * U * s

    e_n, e_a, e_b = err_s(s_n, len(cells)), err_s(s_a, len(a)), err_s(s_b, len(b))
    hu = 0.0 if rows <= 1 else -math.fsum(x / N * (math.log(x) - log_n) for x in a if x > 0)
    hv = 0.0 if cols <= 1 else -math.fsum(x / N * (math.log(x) - log_n) for x in b if x > 0)
    e_hu = 0.0 if rows <= 1 else e_a / N + 4 * U * log_n
    e_hv = 0.0 if cols <= 1 else e_b / N + 4 * U * log_n
    if rows > 1 and cols > 1:
        mi = math.fsum(t[i, j] / N * math.log(Fraction(int(t[i, j]) * N, a[i] * b[j]))
                       for i in range(len(a)) for j in range(len(b)) if t[i, j] > 0)
        mi = max(mi, 0.0)
        e_mi = (e_n + e_a + e_b) / N + 12 * U * log_n
    else:
        mi, e_mi = 0.0, 0.0
    v.update(entropy_true=hu, entropy_pred=hv, mutual_info=mi)
    e.update(entropy_true=e_hu, entropy_pred=e_hv, mutual_info=e_mi)

    def quotient(x, y, e_x, e_y):
        q = x / y
        return q, (e_x + abs(q) * e_y) / max(abs(y) - e_y, 1e-300) + 2 * U * abs(q)

    v["homogeneity"], e["homogeneity"] = quotient(mi, hu, e_mi, e_hu) if hu != 0.0 else (1.0, 0.0)
    v["completeness"], e["completeness"] = quotient(mi, hv, e_mi, e_hv) if hv != 0.0 else (1.0, 0.0)
    norms = [min(hu, hv), math.sqrt(hu * hv), 0.5 * (hu + hv), max(hu, hv)]
    # sqrt(hu hv) moves by half the sum of the relative errors (first order; 1 % on top), and is an
    # exact 0 when either entropy is
    e_geo = 0.505 * norms[1] * (e_hu / hu + e_hv / hv) + 2 * U * norms[1] if hu > 0 and hv > 0 else 0.0
    e_norms = [max(e_hu, e_hv), e_geo, e_hu + e_hv, max(e_hu, e_hv)]
    v["normalizer"], e["normalizer"] = norms, e_norms
    nmi, e_nmi, ami, e_ami = [], [], [], []
    for k in range(4):
        if rows == 1 and cols == 1:
            nmi.append(1.0), e_nmi.append(0.0), ami.append(1.0), e_ami.append(0.0)
            continue
        # a normalizer of 0 has a single cluster on one side, where MI is an exact 0 by rule
        q, eq = quotient(mi, norms[k], e_mi, e_norms[k]) if norms[k] != 0.0 else (0.0, 0.0)
        if norms[k] != 0.0 and abs(mi) <= 1e-15 + e_mi:
            # the convention's threshold is applied to a rounded MI: either side may have taken it
            q, eq = (0.0 if abs(mi) <= 1e-15 else q), max(eq, (abs(mi) + e_mi) / max(norms[k] - e_norms[k], 1e-300))
        nmi.append(q), e_nmi.append(eq)
        if rows == 1 or cols == 1:
            ami.append(0.0), e_ami.append(0.0)
        elif emi is not None:
            den, num = norms[k] - emi[0], mi - emi[0]
            den = min(den, -EPS) if den < 0 else max(den, EPS)
            num = min(num, -EPS) if num < 0 else max(num, EPS)
            q, eq = quotient(num, den, e_mi + emi[1] + EPS, e_norms[k] + emi[1] + EPS)
            ami.append(q), e_ami.append(eq)
        else:
            ami.append(math.nan), e_ami.append(0.0)
    v.update(normalized_mutual_info=nmi, adjusted_mutual_info=ami)
    e.update(normalized_mutual_info=e_nmi, adjusted_mutual_info=e_ami)
    v["expected_mutual_info"] = emi[0] if emi is not None else math.nan
    e["expected_mutual_info"] = emi[1] if emi is not None else 0.0
    return v, e


def fill(a, b):
    """A table with the marginals a, b (greedy)."""
    ra, cb = list(a), list(b)
    table = np.zeros((len(a), len(b)), dtype=np.int64)
    for i in range(len(a)):
        for j in range(len(b)):
            v = min(ra[i], cb[j])
            table[i, j] = v
            ra[i] -= v
            cb[j] -= v
    return table


# marginals of the expected-mutual-information cases (tests/gpu/test_k25_contingency.py; the benchmark
# records their accuracy)
EMI_CASES = {
    "2-2": ([2, 2], [2, 2]),
    "n-1": ([1], [1]),
    "lower-limit-above-1": ([7, 3], [8, 2]),
    "zero-marginal": ([0, 5, 2], [4, 0, 3]),
    "3x70": ([1000, 2000, 3000], [10 + (7 * j) % 150 for j in range(69)] + [None]),
    "2x2-20000": ([10000, 10000], [9000, 11000]),
}
EMI_CASES["3x70"][1][-1] = 6000 - sum(EMI_CASES["3x70"][1][:-1])
