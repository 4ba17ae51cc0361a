"""Silhouette coefficient (Rousseeuw 1987) of features under cluster labels, functional API.

Not in the reference tree (docs/parity.md, "Not in the reference").  With ``d(i, j)`` the Euclidean
distance, ``a(i)`` the mean of ``d`` over the other members of ``i``'s cluster and ``b(i)`` the
smallest mean of ``d`` over another non-empty cluster, ``s(i) = (b - a) / max(a, b)``.  ROCm float32 /
float16 / bfloat16 features run K23 (csrc/kernels/silhouette.hip): 128 x 128 FP32-MFMA tiles of the
inner products whose epilogue takes the square roots and sums them per sample and cluster in FP64
registers, so neither a distance nor an ``[N, K]`` table is written to memory.  CPU tensors, float64
features and features whose inner stride is not 1 run the ATen form below, which evaluates the
definition in FP64 from direct differences, a bounded chunk of query rows at a time.
"""

from typing import Dict, Optional

import torch

import torcheval_amd.ops as _ops
from torcheval_amd.ops import silhouette as _k23
from torcheval_amd.ops.hostread import read_int

__all__ = ["silhouette_samples", "silhouette_score"]

# the ATen form keeps its [chunk, N] float64 distance block at or below this many bytes
_ATEN_CHUNK_BYTES = 1 << 28

_BAD_LABEL = "silhouette: `labels` holds a value outside [0, num_clusters)"


def silhouette_score(input: torch.Tensor, labels: torch.Tensor, *, num_clusters: Optional[int] = None) -> torch.Tensor:
    """Mean silhouette coefficient of ``[N, D]`` features under ``[N]`` cluster labels.

    ``s(i) = (b(i) - a(i)) / max(a(i), b(i))`` with ``a(i)`` the mean Euclidean distance from sample
    ``i`` to the other members of its cluster and ``b(i)`` the smallest mean distance to the members
    of another cluster; ``s(i) = 0`` for the only member of a cluster and where ``a = b = 0``.  The
    score is the mean of ``s`` (``sklearn.metrics.silhouette_score`` with the Euclidean metric).

    * Fewer than two non-empty clusters (``N < 2`` included) give NaN, where sklearn raises: raising
      would need a host read.  If every cluster is a singleton the score is 0.
    * A row with a NaN or an infinite feature has the distance NaN to every other row: the score is
      NaN, and so is the ``silhouette_samples`` entry of the row itself and of the other members
      of its cluster.  For every other sample the row's cluster simply is not a candidate for the
      nearest cluster (a NaN mean loses to a number), so their entries stay finite.
    * A label outside ``[0, num_clusters)`` raises on CPU.  On ROCm the sample belongs to no cluster:
      it enters no mean, its ``silhouette_samples`` entry is NaN, the score is the mean over the
      other samples, and the call raises only under ``config.validate``.

    Class version: ``SilhouetteScore``.

    Args:
        input: ``[N, D]`` features, float32, float16, bfloat16 or float64.
        labels: ``[N]`` cluster ids, int64 or int32.  Ids without a member are ignored.
        num_clusters: the ids lie in ``[0, num_clusters)``.  ``None`` reads ``labels.max()`` on the
            host, which is the call's only host synchronisation; with a value there is none.

    Returns a float32 scalar (float64 for float64 features) on the features' device.
    """
    out = _silhouette_checked(input, labels, num_clusters)
    return out["score64"][0] if input.dtype == torch.float64 else out["score"][0]


def silhouette_samples(input: torch.Tensor, labels: torch.Tensor, *, num_clusters: Optional[int] = None) -> torch.Tensor:
    """The silhouette coefficient ``s(i)`` of every sample: ``[N]``, float32 (float64 for float64
    features).  Definition, arguments and the handling of degenerate inputs as ``silhouette_score``;
    with fewer than two non-empty clusters every entry is NaN."""
    out = _silhouette_checked(input, labels, num_clusters)
    return out["s"] if input.dtype == torch.float64 else out["samples"]


def _silhouette_param_check(num_clusters: Optional[int]) -> None:
    if num_clusters is not None and (
        not isinstance(num_clusters, int) or isinstance(num_clusters, bool) or num_clusters < 1
    ):
        raise ValueError(f"`num_clusters` should be a positive integer or None, got {num_clusters!r}.")


def _silhouette_input_check(input: torch.Tensor, labels: torch.Tensor) -> None:
    if input.dim() != 2 or not input.is_floating_point() or input.shape[1] < 1:
        raise ValueError(f"input should be floating [N, D] features with D >= 1, got shape {tuple(input.shape)}.")
    if labels.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"labels should be int64 or int32 cluster ids, got dtype {labels.dtype}.")
    if labels.dim() != 1 or labels.shape[0] != input.shape[0]:
        raise ValueError(
            f"labels should be [N] for [N, D] features, got shapes {tuple(labels.shape)} and {tuple(input.shape)}."
        )


def _silhouette_checked(input: torch.Tensor, labels: torch.Tensor, num_clusters: Optional[int]) -> Dict[str, torch.Tensor]:
    _silhouette_param_check(num_clusters)
    _silhouette_input_check(input, labels)
    if _ops.compiling():
        # no inference mode inside a traced graph (as spearman_corrcoef)
        return _silhouette_validated(input, labels, num_clusters)
    with torch.inference_mode():
        return _silhouette_validated(input, labels, num_clusters)


def _silhouette_validated(input: torch.Tensor, labels: torch.Tensor, num_clusters: Optional[int]) -> Dict[str, torch.Tensor]:
    """``_silhouette`` with the bad-label flag surfaced as ``mean_iou`` surfaces its own: ROCm calls
    carry the device flag under ``config.validate`` only and read it after the kernels."""
    from torcheval_amd.config import config

    labels = labels.to(input.device)
    if num_clusters is None:
        # the call's one host read; -1 and below (or no sample) leave one, empty, cluster
        num_clusters = max(1, read_int(labels.max().to(torch.int64)) + 1) if labels.numel() else 1
    err = torch.zeros(1, dtype=torch.int32, device=input.device) if input.is_cuda and config.validate else None
    out = _silhouette(input, labels, num_clusters, err=err)
    if err is not None and read_int(err) != 0:
        raise ValueError(_BAD_LABEL + " (such samples belong to no cluster).")
    return out


def _silhouette(input: torch.Tensor, labels: torch.Tensor, num_clusters: int, groups: int = 0,
                err: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The statistics of checked inputs, from whichever path the tensors take: float64 ``a``, ``b``,
    ``s`` ``[N]``, float32 ``samples`` ``[N]``, ``score64`` ``[1]`` and float32 ``score`` ``[1]``.
    ``groups`` reaches K23 only (tests)."""
    if _k23.supported(input, labels, num_clusters):
        return _k23.silhouette(input, labels, num_clusters, groups, err)
    return _silhouette_aten(input, labels, num_clusters, err)


def _distance_block(q: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """``[len(q), len(r)]`` float64 Euclidean distances.  On CPU from direct differences (``cdist``
    without the matrix-multiply form), so equal rows are at distance 0 exactly.  On ROCm that ``cdist``
    kernel left every output past the first 2^24 of a call at 0 (torch 2.10: the scores of
    benchmarks/bench_silhouette.py came out halved), so there the block is the FP64 form
    ``(|q|^2 + |r|^2) - 2 q r^T`` that sklearn uses, clamped at 0: exact on integer data, and off by
    about ``1e-8 |x|`` for rows closer than that."""
    if not q.is_cuda:
        return torch.cdist(q, r, compute_mode="donot_use_mm_for_euclid_dist")
    d2 = ((q * q).sum(dim=1)[:, None] + (r * r).sum(dim=1)[None, :]) - 2.0 * torch.mm(q, r.T)
    return d2.clamp_(min=0.0).sqrt_()


def _silhouette_aten(input: torch.Tensor, labels: torch.Tensor, num_clusters: int,
                     err: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The definition in FP64 ATen.  Per chunk of query rows one ``[chunk, N]`` block of distances
    (``_distance_block``), NaN in the rows and columns of non-finite samples, 0 on the positional
    diagonal, and one ``[chunk, N] @ [N, K]`` product with the one-hot membership for the sums per
    cluster; no larger distance tensor exists."""
    x = input.double()
    n, k, dev = x.shape[0], num_clusters, x.device
    lab = labels.to(torch.int64)
    bad = (lab < 0) | (lab >= k)
    if not x.is_cuda:
        if bool(bad.any()):
            raise ValueError(_BAD_LABEL + ".")
    elif err is not None:
        err.bitwise_or_(bad.any().to(err.dtype))
    lab = torch.where(bad, k, lab)
    member = torch.zeros(n, k + 1, dtype=torch.float64, device=dev)
    member = member.scatter_(1, lab[:, None], 1.0)[:, :k]  # [N, K] one-hot; a bad label: no cluster
    counts = member.sum(dim=0)
    poisoned = ~torch.isfinite(x).all(dim=1)
    clean = torch.where(poisoned[:, None], 0.0, x)
    own = lab.clamp(max=k - 1)
    n_own = counts[own]
    nan = torch.full((), torch.nan, dtype=torch.float64, device=dev)
    clusters = torch.arange(k, device=dev)
    a_parts, b_parts = [], []
    step = max(1, _ATEN_CHUNK_BYTES // (8 * max(n, 1)))
    for lo in range(0, n, step):
        hi = min(lo + step, n)
        rows = torch.arange(lo, hi, device=dev)
        d = _distance_block(clean[lo:hi], clean)
        d = d.masked_fill(poisoned[None, :] | poisoned[lo:hi, None], torch.nan)
        d[rows - lo, rows] = 0.0
        # a NaN distance poisons its own cluster's sum only: sum the NaNs apart from the numbers
        isnan = torch.isnan(d)
        sums = torch.where(isnan, 0.0, d) @ member
        sums = torch.where((isnan.double() @ member) > 0, nan, sums)  # [chunk, K]
        mine = own[lo:hi, None] == clusters[None, :]
        a_parts.append(sums.gather(1, own[lo:hi, None])[:, 0] / (n_own[lo:hi] - 1.0).clamp(min=1.0))
        means = sums / counts[None, :]
        candidate = ~mine & (counts[None, :] > 0) & ~torch.isnan(means)
        best = torch.where(candidate, means, torch.inf).min(dim=1).values
        b_parts.append(torch.where(candidate.any(dim=1), best, nan))
    empty = torch.empty(0, dtype=torch.float64, device=dev)
    a = torch.cat(a_parts) if a_parts else empty
    b = torch.cat(b_parts) if b_parts else empty
    a = torch.where(n_own > 1, a, 0.0)
    top = torch.maximum(a, b)
    s = torch.where((n_own == 1) | (top == 0), 0.0, (b - a) / torch.where(top == 0, 1.0, top))
    s = torch.where(torch.isnan(a) | torch.isnan(b), nan, s)
    a, b, s = (torch.where(bad, nan, v) for v in (a, b, s))
    members = counts.sum()
    score = torch.where((counts > 0).sum() >= 2, torch.where(bad, 0.0, s).sum() / members, nan).reshape(1)
    return {"a": a, "b": b, "s": s, "samples": s.to(torch.float32), "score64": score,
            "score": score.to(torch.float32)}
