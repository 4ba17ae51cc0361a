"""Edge inputs and the plain-ATen oracle of the thresholded binary / multilabel metrics.

Shared by tests/metrics/classification/test_threshold_dtype_oracle.py (CPU) and
tests/gpu/test_threshold_dtype_edges.py.  The oracle is ``torch.where(x < thr, 0, 1)`` on the CPU
tensor in its own dtype - ATen casts the Python threshold to the tensor's dtype (integer and bool
tensors promote to float32) - followed by int64 counts.  Nothing here calls the package.
"""

import torch

FLOAT_DTYPES = (torch.float32, torch.bfloat16, torch.float16, torch.float64)
INT_DTYPES = (torch.int64, torch.int32, torch.uint8, torch.bool)
THRESHOLDS = (0.5, 0.7, 0.9, 0.1, 0.3, 1 / 3, 1e-3, 0.0, 1.0, -0.25)
CRITERIA = ("exact_match", "hamming", "overlap", "contain", "belong")


def dtype_id(dtype: torch.dtype) -> str:
    return str(dtype).replace("torch.", "")


def _edges(dtype: torch.dtype, thr: float) -> torch.Tensor:
    up = torch.tensor(float("inf"), dtype=dtype)
    tv = torch.tensor(thr, dtype=dtype)  # the threshold as ATen sees it
    t32 = torch.tensor(thr, dtype=torch.float32).to(dtype)  # the threshold as a float32 compare sees it
    special = torch.tensor([0.0, -0.0, 1.0, float("nan"), float("inf"), float("-inf")], dtype=dtype)
    return torch.cat([
        torch.stack([tv, torch.nextafter(tv, up), torch.nextafter(tv, -up),
                     t32, torch.nextafter(t32, up), torch.nextafter(t32, -up)]),
        special,
    ])


def edge_scores(dtype: torch.dtype, thr: float, n: int, seed: int) -> torch.Tensor:
    """1-D CPU tensor of ``dtype`` and length ``n``: the threshold as ``dtype`` and as float32 with
    their neighbours, the special values and uniform filler, repeated and permuted (about half
    edges; every edge is present once n >= 24).  Integer / bool dtypes: seeded values of the whole
    range of the dtype, 0 and 1 among them."""
    g = torch.Generator().manual_seed(seed)
    if dtype.is_floating_point:
        e = _edges(dtype, thr)
        e = e.repeat(max(1, n // (2 * e.numel())))
        fill = torch.rand(max(n - e.numel(), 0), generator=g, dtype=torch.float64).to(dtype)
    else:
        if dtype == torch.bool:
            fill = torch.randint(0, 2, (n,), generator=g).to(dtype)
        else:
            info = torch.iinfo(dtype)
            # randint's upper bound is exclusive and must fit int64: the maximum goes in by hand
            fill = torch.randint(info.min, info.max, (n,), generator=g, dtype=torch.int64).to(dtype)
            fill[::7] = info.max
            fill[3::7] = info.min
        e = torch.tensor([0, 1], dtype=dtype).repeat(max(1, n // 8))
    v = torch.cat([e, fill])
    return v[torch.randperm(v.numel(), generator=g)][:n].contiguous()


def binary_targets(n: int, seed: int, dtype: torch.dtype = torch.int64) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed + 1000)
    return torch.randint(0, 2, (n,), generator=g).to(dtype)


def multilabel_targets(pred: torch.Tensor, seed: int, dtype: torch.dtype = torch.int64) -> torch.Tensor:
    """{0, 1} targets [n, c] tied to the oracle's decisions, so that one flipped decision moves
    every criterion: rows 0, 2 (mod 4) equal ``pred``, rows 1 differ in one label, rows 3 are
    random."""
    g = torch.Generator().manual_seed(seed + 2000)
    t = pred.clone()
    n, c = t.shape
    rows = torch.arange(n)
    col = torch.randint(0, c, (n,), generator=g)
    one = rows % 4 == 1
    t[rows[one], col[one]] ^= 1
    rnd = rows % 4 == 3
    t[rnd] = torch.randint(0, 2, (int(rnd.sum()), c), generator=g)
    return t.to(dtype)


def oracle_pred(x: torch.Tensor, thr: float) -> torch.Tensor:
    """int64 {0, 1} decisions of plain ATen on the CPU tensor in its own dtype."""
    assert x.device.type == "cpu"
    return torch.where(x < thr, 0, 1)


def float32_model_pred(x: torch.Tensor, thr: float) -> torch.Tensor:
    """The decision of a float32 compare (scores and threshold both rounded to float32): what the
    sensitivity check tells apart from the oracle."""
    return (~(x.float() < torch.tensor(thr, dtype=torch.float32))).long()


def oracle_counts(pred: torch.Tensor, target: torch.Tensor, weight=None, strict: bool = False) -> torch.Tensor:
    """[tp, fp, tn, fn] in float64 (exact: integer counts, or weights that are multiples of 1/4),
    by the documented contract of ``ops.classification.binary_counts``: with ``strict`` a target
    outside {0, 1} counts nowhere, otherwise it is a wrong prediction (fp when predicted
    positive, fn when predicted negative)."""
    t = target.double()
    t1, t0 = t == 1.0, t == 0.0
    other = ~(t1 | t0) if not strict else torch.zeros_like(t1)
    pos = pred.bool()
    w = torch.ones_like(t) if weight is None else weight.double()
    return torch.stack([
        (w * (pos & t1)).sum(),
        (w * (pos & (t0 | other))).sum(),
        (w * (~pos & t0)).sum(),
        (w * (~pos & (t1 | other))).sum(),
    ])


def binary_formulas(pred: torch.Tensor, target: torch.Tensor) -> dict:
    """The five binary metrics from int64 counts of (pred, target in {0, 1}), as float32 / int64
    CPU tensors.  Denominators are non-zero for the edge inputs (both decisions and both targets
    are always present at the sizes the tests use)."""
    tp = ((pred == 1) & (target == 1)).sum()
    fp = ((pred == 1) & (target == 0)).sum()
    tn = ((pred == 0) & (target == 0)).sum()
    fn = ((pred == 0) & (target == 1)).sum()
    for d in (tp + fp, tp + fn):
        assert int(d) > 0
    f = torch.float32
    return {
        "accuracy": (tp + tn).to(f) / (tp + fp + tn + fn).to(f),
        "precision": tp.to(f) / (tp + fp).to(f),
        "recall": tp.to(f) / (tp + fn).to(f),
        "f1_score": (2 * tp).to(f) / (2 * tp + fp + fn).to(f),
        "confusion_matrix": torch.stack([torch.stack([tn, fp]), torch.stack([fn, tp])]),
    }


def multilabel_formula(pred: torch.Tensor, target: torch.Tensor, criteria: str) -> torch.Tensor:
    """multilabel accuracy of int64 [n, c] decisions vs {0, 1} targets, float32."""
    p, t = pred.bool(), target.bool()
    if criteria == "hamming":
        return (p == t).sum().float() / t.numel()
    if criteria == "exact_match":
        ok = (p == t).all(dim=1)
    elif criteria == "overlap":
        ok = (p & t).any(dim=1) | (~p.any(dim=1) & ~t.any(dim=1))
    elif criteria == "contain":
        ok = (~t | p).all(dim=1)  # every target label is predicted
    elif criteria == "belong":
        ok = (~p | t).all(dim=1)  # every predicted label is a target label
    else:
        raise ValueError(criteria)
    return ok.sum().float() / t.shape[0]
