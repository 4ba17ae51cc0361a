"""External clustering indices that compare two labelings, functional API.

Not in the reference tree (docs/parity.md, "Not in the reference").  Rand and adjusted Rand index,
Fowlkes-Mallows, mutual information, NMI, AMI, homogeneity, completeness and V-measure are all
functions of the rectangular contingency table ``n[i, j] = #{s : true[s] = i, pred[s] = j}``.  Contiguous
ROCm label vectors run K25 (csrc/kernels/contingency.hip): the table is counted in int64 through LDS
slices, the pair sums are exact u64, the entropies and AMI's expected mutual information are
fixed-order FP64 sums, and every value leaves one single-wave launch in one float64 vector.  CPU
tensors, non-contiguous labels, tables of more than 2^22 cells and totals of 2^32 or more run the ATen
form below, which is the definition: ``bincount`` of ``true * C + pred``, int64 pair sums (FP64 ones from a
total of 2^32 on, where int64 would wrap), FP64 entropies and the expected mutual information from ``lgamma`` over ``[R, C]`` with a loop over ``n``.

Conventions for degenerate inputs follow sklearn 1.7.2 and are listed in docs/parity.md.
"""

import math
from typing import Optional, Tuple

import torch

import torcheval_amd.ops as _ops
from torcheval_amd.ops import contingency as _k25
from torcheval_amd.ops.hostread import read_int

__all__ = [
    "adjusted_mutual_info_score",
    "adjusted_rand_score",
    "completeness_score",
    "contingency_matrix",
    "fowlkes_mallows_score",
    "homogeneity_score",
    "mutual_info_score",
    "normalized_mutual_info_score",
    "rand_score",
    "v_measure_score",
]

_BAD_LABEL = "contingency: a label lies outside [0, num_classes) or [0, num_clusters)"
_EPS = 2.220446049250313e-16
# the ATen form's EMI keeps its [chunk, R, C] float64 temporaries at or below this many elements
_ATEN_EMI_ELEMENTS = 1 << 20

_COMMON_ARGS = """
    Args:
        labels_true: ``[N]`` class ids, int64 or int32.
        labels_pred: ``[N]`` cluster ids, int64 or int32.
        num_classes: the class ids lie in ``[0, num_classes)``.
        num_clusters: the cluster ids lie in ``[0, num_clusters)``.  ``None`` for either range reads
            that vector's ``max()`` on the host; with both given there is no host synchronisation.

    Ids without a member do not change a value.  ``N = 0`` gives NaN (sklearn raises).  A label outside
    its range raises on CPU; on ROCm the pair is counted nowhere and the call raises only under
    ``config.validate``.  Returns a float64 scalar on the labels' device.
"""


def contingency_matrix(labels_true: torch.Tensor, labels_pred: torch.Tensor, *, num_classes: Optional[int] = None,
                       num_clusters: Optional[int] = None) -> torch.Tensor:
    """The int64 ``[num_classes, num_clusters]`` table ``n[i, j]``: how many samples have class ``i`` and
    cluster ``j`` (``sklearn.metrics.cluster.contingency_matrix`` without its relabelling, so a row or
    column of an id without a member stays, all zero).  Arguments as ``rand_score``."""
    return _checked(labels_true, labels_pred, num_classes, num_clusters)[0]


def rand_score(labels_true: torch.Tensor, labels_pred: torch.Tensor, *, num_classes: Optional[int] = None,
               num_clusters: Optional[int] = None) -> torch.Tensor:
    """Rand index: the share of sample pairs on which the two labelings agree (together in both or
    apart in both); 1 when there is no pair (``sklearn.metrics.rand_score``).  Class version: ``RandScore``.
    """
    return _value(labels_true, labels_pred, num_classes, num_clusters, "rand")


def adjusted_rand_score(labels_true: torch.Tensor, labels_pred: torch.Tensor, *, num_classes: Optional[int] = None,
                        num_clusters: Optional[int] = None) -> torch.Tensor:
    """Rand index adjusted for chance, ``2 (tp tn - fn fp) / ((tp + fn)(fn + tn) + (tp + fp)(fp + tn))``
    over the pair counts, 1 when ``fn = fp = 0`` (``sklearn.metrics.adjusted_rand_score``).  Class
    version: ``AdjustedRandScore``."""
    return _value(labels_true, labels_pred, num_classes, num_clusters, "adjusted_rand")


def fowlkes_mallows_score(labels_true: torch.Tensor, labels_pred: torch.Tensor, *, num_classes: Optional[int] = None,
                          num_clusters: Optional[int] = None) -> torch.Tensor:
    """Fowlkes-Mallows index: the geometric mean of pairwise precision and recall, 0 when no pair is
    together in both labelings (``sklearn.metrics.fowlkes_mallows_score``).  Class version:
    ``FowlkesMallowsScore``."""
    return _value(labels_true, labels_pred, num_classes, num_clusters, "fowlkes_mallows")


def mutual_info_score(labels_true: torch.Tensor, labels_pred: torch.Tensor, *, num_classes: Optional[int] = None,
                      num_clusters: Optional[int] = None) -> torch.Tensor:
    """Mutual information of the two labelings in nats, clipped at 0 (``sklearn.metrics.mutual_info_score``).
    Class version: ``MutualInfoScore``."""
    return _value(labels_true, labels_pred, num_classes, num_clusters, "mutual_info")


def normalized_mutual_info_score(labels_true: torch.Tensor, labels_pred: torch.Tensor, *,
                                 num_classes: Optional[int] = None, num_clusters: Optional[int] = None,
                                 average_method: str = "arithmetic") -> torch.Tensor:
    """Mutual information over the ``average_method`` (``"min"``, ``"geometric"``, ``"arithmetic"``,
    ``"max"``) mean of the two entropies; 1 when both labelings have one cluster, 0 when the mutual
    information is within 1e-15 of 0 (``sklearn.metrics.normalized_mutual_info_score``).  Class version:
    ``NormalizedMutualInfoScore``."""
    k = _average_index(average_method)
    return _value(labels_true, labels_pred, num_classes, num_clusters, "normalized_mutual_info", k)


def adjusted_mutual_info_score(labels_true: torch.Tensor, labels_pred: torch.Tensor, *,
                               num_classes: Optional[int] = None, num_clusters: Optional[int] = None,
                               average_method: str = "arithmetic") -> torch.Tensor:
    """Mutual information adjusted for chance, ``(MI - E[MI]) / (mean(H(U), H(V)) - E[MI])`` with the
    expectation over the hypergeometric model of random labelings with the same cluster sizes; 1
    when both labelings have one cluster, 0 when exactly one has, numerator and denominator kept
    ``eps`` away from 0 with their signs (``sklearn.metrics.adjusted_mutual_info_score``).  Class version:
    ``AdjustedMutualInfoScore``."""
    k = _average_index(average_method)
    return _value(labels_true, labels_pred, num_classes, num_clusters, "adjusted_mutual_info", k, emi=True)


def homogeneity_score(labels_true: torch.Tensor, labels_pred: torch.Tensor, *, num_classes: Optional[int] = None,
                      num_clusters: Optional[int] = None) -> torch.Tensor:
    """``MI / H(labels_true)``, 1 when that entropy is 0: every cluster holds members of one class
    (``sklearn.metrics.homogeneity_score``).  Class version: ``HomogeneityScore``."""
    return _value(labels_true, labels_pred, num_classes, num_clusters, "homogeneity")


def completeness_score(labels_true: torch.Tensor, labels_pred: torch.Tensor, *, num_classes: Optional[int] = None,
                       num_clusters: Optional[int] = None) -> torch.Tensor:
    """``MI / H(labels_pred)``, 1 when that entropy is 0: all members of a class are in one cluster
    (``sklearn.metrics.completeness_score``).  Class version: ``CompletenessScore``."""
    return _value(labels_true, labels_pred, num_classes, num_clusters, "completeness")


def v_measure_score(labels_true: torch.Tensor, labels_pred: torch.Tensor, *, num_classes: Optional[int] = None,
                    num_clusters: Optional[int] = None, beta: float = 1.0) -> torch.Tensor:
    """``(1 + beta) h c / (beta h + c)`` of homogeneity ``h`` and completeness ``c``, 0 when both are 0
    (``sklearn.metrics.v_measure_score``).  Class version: ``VMeasureScore``."""
    _beta_check(beta)
    values = _checked(labels_true, labels_pred, num_classes, num_clusters, values=True)[1]
    return _v_measure(values, beta)


for _f in (rand_score, adjusted_rand_score, fowlkes_mallows_score, mutual_info_score, normalized_mutual_info_score,
           adjusted_mutual_info_score, homogeneity_score, completeness_score, v_measure_score):
    _f.__doc__ = (_f.__doc__ or "").rstrip() + "\n" + _COMMON_ARGS
del _f


# ----------------------------------------------------------------------------- checks
def _range_check(value: Optional[int], name: str, required: bool = False) -> None:
    if value is None and not required:
        return
    if not isinstance(value, int) or isinstance(value, bool) or value < 1:
        raise ValueError(f"`{name}` should be a positive integer{'' if required else ' or None'}, got {value!r}.")


def _average_index(average_method: str) -> int:
    if average_method not in _k25.AVERAGE_METHODS:
        raise ValueError(f"`average_method` should be one of {list(_k25.AVERAGE_METHODS)}, got {average_method!r}.")
    return _k25.AVERAGE_METHODS.index(average_method)


def _beta_check(beta: float) -> None:
    if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not beta >= 0.0 or math.isinf(beta):
        raise ValueError(f"`beta` should be a finite non-negative number, got {beta!r}.")


def _labels_check(labels_true: torch.Tensor, labels_pred: torch.Tensor) -> None:
    for name, t in (("labels_true", labels_true), ("labels_pred", labels_pred)):
        if t.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"{name} should be int64 or int32 ids, got dtype {t.dtype}.")
        if t.dim() != 1:
            raise ValueError(f"{name} should be a [N] vector, got shape {tuple(t.shape)}.")
    if labels_true.shape[0] != labels_pred.shape[0]:
        raise ValueError(
            f"labels_true and labels_pred should have one length, got {labels_true.shape[0]} and {labels_pred.shape[0]}."
        )


def _v_measure(values: torch.Tensor, beta: float) -> torch.Tensor:
    h, c = values[_k25.INDEX["homogeneity"]], values[_k25.INDEX["completeness"]]
    return torch.where(h + c == 0.0, 0.0, (1.0 + beta) * h * c / (beta * h + c))


def _value(labels_true, labels_pred, num_classes, num_clusters, name: str, offset: int = 0,
           emi: bool = False) -> torch.Tensor:
    return _checked(labels_true, labels_pred, num_classes, num_clusters, values=True, emi=emi)[1][
        _k25.INDEX[name] + offset]


def _checked(labels_true: torch.Tensor, labels_pred: torch.Tensor, num_classes: Optional[int],
             num_clusters: Optional[int], values: bool = False,
             emi: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    _range_check(num_classes, "num_classes")
    _range_check(num_clusters, "num_clusters")
    _labels_check(labels_true, labels_pred)
    if _ops.compiling():
        return _validated(labels_true, labels_pred, num_classes, num_clusters, values, emi)
    with torch.inference_mode():
        return _validated(labels_true, labels_pred, num_classes, num_clusters, values, emi)


def _range_of(labels: torch.Tensor) -> int:
    """One host read; no sample, or only negative ids, leave one, empty, id."""
    return max(1, read_int(labels.max().to(torch.int64)) + 1) if labels.numel() else 1


def _validated(labels_true, labels_pred, num_classes, num_clusters, values: bool, emi: bool):
    """The table (and the values vector) with the bad-label flag surfaced as ``silhouette_score``
    surfaces its own: ROCm calls carry the device flag under ``config.validate`` only."""
    from torcheval_amd.config import config

    labels_pred = labels_pred.to(labels_true.device)
    r = _range_of(labels_true) if num_classes is None else num_classes
    c = _range_of(labels_pred) if num_clusters is None else num_clusters
    dev = labels_true.device
    err = torch.zeros(1, dtype=torch.int32, device=dev) if (not labels_true.is_cuda or config.validate) else None
    table = _contingency(labels_true, labels_pred, r, c, err=err)
    out = _values(table, emi) if values else None
    if err is not None and read_int(err) != 0:
        raise ValueError(_BAD_LABEL + ("." if not labels_true.is_cuda else " (such pairs were counted nowhere)."))
    return table, out


# ----------------------------------------------------------------------------- the two paths
def _contingency(labels_true: torch.Tensor, labels_pred: torch.Tensor, num_classes: int, num_clusters: int,
                 slice_size: int = 0, err: Optional[torch.Tensor] = None,
                 table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The int64 ``[R, C]`` table of checked label vectors, or ``table`` with their counts added, from
    whichever path the tensors take.  ``slice_size`` reaches K25 only (tests)."""
    if table is None:
        table = torch.zeros(num_classes, num_clusters, dtype=torch.int64, device=labels_true.device)
    if _k25.supported(labels_true, labels_pred, table):
        _k25.contingency_update(labels_true, labels_pred, table, err, slice_size)
    else:
        table += _contingency_aten(labels_true, labels_pred, num_classes, num_clusters, err).to(table.device)
    return table


def _values(table: torch.Tensor, emi: bool = True) -> torch.Tensor:
    """The float64 values vector (``ops.contingency.INDEX``) of a table whose total is below 2^32."""
    if _k25.supported_table(table):
        return _k25.contingency_values(table, emi)[0]
    return _values_aten(table, emi)


def _contingency_aten(labels_true: torch.Tensor, labels_pred: torch.Tensor, num_classes: int, num_clusters: int,
                      err: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``bincount(true * C + pred)``; a pair with a label outside its range goes to a cell past the
    table and sets ``err``."""
    r, c = num_classes, num_clusters
    t, p = labels_true.to(torch.int64), labels_pred.to(torch.int64)
    bad = (t < 0) | (t >= r) | (p < 0) | (p >= c)
    if err is not None:
        err.bitwise_or_(bad.any().to(err.dtype))
    cell = torch.where(bad, r * c, t * c + p)
    return torch.bincount(cell, minlength=r * c + 1)[: r * c].reshape(r, c)


def _expected_mutual_info_aten(a: torch.Tensor, b: torch.Tensor, total: torch.Tensor) -> torch.Tensor:
    """``sum_ij sum_n (n / N) log(N n / (a_i b_j)) p(n)`` with the hypergeometric ``p`` through ``lgamma``,
    vectorised over ``[R, C]`` and a block of ``n`` at a time.  Reads the largest ``n`` on the host."""
    dev = a.device
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    n_max = int(torch.minimum(a.max(), b.max()).item()) if a.numel() and b.numel() else 0
    if n_max < 1:
        return zero
    N = total.to(torch.float64)
    ai, bj = a.to(torch.float64)[None, :, None], b.to(torch.float64)[None, None, :]
    live = (ai > 0) & (bj > 0)
    lo, hi = torch.clamp(ai + bj - N, min=1.0), torch.minimum(ai, bj)
    g = (torch.lgamma(ai + 1) + torch.lgamma(N - ai + 1) + torch.lgamma(bj + 1) + torch.lgamma(N - bj + 1)
         - torch.lgamma(N + 1))
    k = torch.log(N) - torch.log(ai.clamp(min=1.0)) - torch.log(bj.clamp(min=1.0))
    step = max(1, _ATEN_EMI_ELEMENTS // max(1, a.numel() * b.numel()))
    emi = zero
    for n0 in range(1, n_max + 1, step):
        n = torch.arange(n0, min(n0 + step, n_max + 1), dtype=torch.float64, device=dev)[:, None, None]
        valid = live & (n >= lo) & (n <= hi)
        m = torch.where(valid, n, lo.expand_as(valid).clamp(max=hi.clamp(min=1.0)))  # any n inside the range
        logp = g - torch.lgamma(m + 1) - torch.lgamma(ai - m + 1) - torch.lgamma(bj - m + 1) - torch.lgamma(N - ai - bj + m + 1)
        term = m / N * (torch.log(m) + k) * torch.exp(logp)
        emi = emi + torch.where(valid, term, 0.0).sum()
    return emi


def _values_aten(table: torch.Tensor, emi: bool = True) -> torch.Tensor:
    """The definition in ATen: FP64 entropies and mutual information, sklearn 1.7.2's conventions by
    ``torch.where``, and the pair sums ``sum x (x - 1) / 2`` in int64 while the total is below 2^32, where
    none of them can wrap.  From a total of 2^32 on ``N (N - 1) / 2`` and the sums leave int64, so the pair
    sums are formed in FP64 instead: Rand, ARI and FMI then carry the roundings of those sums (relative
    ``(k + 4) 2^-53`` for a sum of ``k`` terms; tests/_contingency_oracle.py, ``pair_bounds_f64``) and are no
    longer exact to the last bit.  Same layout as K25's vector."""
    dev = table.device
    n = table.to(torch.int64)
    a, b = n.sum(dim=1), n.sum(dim=0)
    total = a.sum()

    def f64(x):
        return x.to(torch.float64)

    def half_product(x):  # x (x - 1) / 2 with the even factor halved first: no intermediate above the result
        return torch.where(x % 2 == 0, (x // 2) * (x - 1), x * ((x - 1) // 2))

    def pairs(x):  # exact below a total of 2^32; wraps above, where it is not used
        return half_product(x).sum()

    def pairs_f64(x):
        x = f64(x)
        return (x * (x - 1.0) * 0.5).sum()

    def xlogx(x):
        return torch.xlogy(f64(x), f64(x)).sum()

    exact = total < 2**32

    def pick(ints, floats):
        return torch.where(exact, f64(ints), floats)

    # halves of sklearn's pair confusion matrix (every index is a ratio of products of two of them)
    p, pa, pb = pairs(n), pairs(a), pairs(b)
    all_pairs = half_product(total)
    tn_i = all_pairs - p - (pb - p) - (pa - p)
    pf, paf, pbf = pairs_f64(n), pairs_f64(a), pairs_f64(b)
    all_f = f64(total) * (f64(total) - 1.0) * 0.5
    tp, fp, fn = pick(p, pf), pick(pb - p, pbf - pf), pick(pa - p, paf - pf)
    tn = pick(tn_i, ((all_f - pf) - (pbf - pf)) - (paf - pf))
    one = torch.ones((), dtype=torch.float64, device=dev)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    nan = torch.full((), torch.nan, dtype=torch.float64, device=dev)
    agree = (fn == 0) & (fp == 0)  # on the exact route: of integers below 2^63, whose conversion keeps a 0
    rand = torch.where(agree | (total <= 1), one, pick(tn_i + p, tn + tp) / pick(all_pairs, all_f))
    bottom = (pick(p + (pa - p), tp + fn) * pick((pa - p) + tn_i, fn + tn)
              + pick(p + (pb - p), tp + fp) * pick((pb - p) + tn_i, fp + tn))
    ari = torch.where(agree, one, 2.0 * (tp * tn - fn * fp) / bottom)
    fmi = torch.where(tp != 0, torch.sqrt(tp / pick(pb, pbf)) * torch.sqrt(tp / pick(pa, paf)), zero)

    N = f64(total)
    log_n = torch.log(N)
    rows, cols = (a > 0).sum(), (b > 0).sum()
    s_cell, s_a, s_b = xlogx(n), xlogx(a), xlogx(b)
    hu = torch.where(rows <= 1, zero, log_n - s_a / N)
    hv = torch.where(cols <= 1, zero, log_n - s_b / N)
    mi = torch.where((rows > 1) & (cols > 1), (((s_cell - s_a) - s_b) / N + log_n).clamp(min=0.0), zero)
    e = _expected_mutual_info_aten(a, b, total) if emi else nan
    norm = torch.stack([torch.minimum(hu, hv), torch.sqrt(hu * hv), 0.5 * (hu + hv), torch.maximum(hu, hv)])
    single = (rows == 1) & (cols == 1)
    nmi = torch.where(single, one, torch.where(mi.abs() <= 1e-15, zero, mi / norm))
    den, num = norm - e, mi - e
    den = torch.where(den < 0, den.clamp(max=-_EPS), den.clamp(min=_EPS))
    num = torch.where(num < 0, num.clamp(max=-_EPS), num.clamp(min=_EPS))
    ami = torch.where(single, one, torch.where((rows == 1) | (cols == 1), zero, num / den))
    ami = torch.where(torch.isnan(e), nan, ami)
    hom = torch.where(hu != 0, mi / hu, one)
    com = torch.where(hv != 0, mi / hv, one)
    out = torch.cat([torch.stack([rand, ari, fmi, hu, hv, mi, e]), norm, nmi, ami, torch.stack([hom, com])])
    return torch.where(total == 0, nan, out)
