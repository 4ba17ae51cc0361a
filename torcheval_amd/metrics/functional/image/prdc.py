"""Improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020),
functional API.

Not in the reference tree (docs/parity.md, "Not in the reference").  Both pairs are k-nearest-
neighbour statistics of the squared distances between real and generated features.  ROCm float32 /
float16 / bfloat16 features with ``k <= 8`` run K22 (csrc/kernels/prdc.hip): 128 x 128 FP32-MFMA
tiles of the inner products whose epilogue keeps the k smallest distances or the ball counts of
every row in the block, so no distance is written to memory.  CPU tensors, float64 features,
features whose inner stride is not 1 and ``k > 8`` run the ATen form below, which evaluates the
definition in FP64 a bounded chunk of query rows at a time.
"""

from typing import Dict, Tuple

import torch

import torcheval_amd.ops as _ops
from torcheval_amd.ops import prdc as _k22

__all__ = ["density_coverage", "improved_precision_recall"]

# the ATen form keeps its [chunk, n_ref] float64 distance block at or below this many bytes
_ATEN_CHUNK_BYTES = 1 << 28


def improved_precision_recall(
    real_features: torch.Tensor, fake_features: torch.Tensor, *, k: int = 3
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Improved precision and recall of ``[M, D]`` generated against ``[N, D]`` real features.

    With ``d2(a, b) = max(0, (|a|^2 + |b|^2) - 2 <a, b>)`` and ``r_i^2`` (``s_j^2``) the k-th
    smallest ``d2`` from real row ``i`` (generated row ``j``) to the other rows of its own set
    (by position, so a duplicate row elsewhere counts at distance 0)::

        precision = #{j : d2(y_j, x_i) <= r_i^2 for some i} / M
        recall    = #{i : d2(x_i, y_j) <= s_j^2 for some j} / N

    Every comparison is ``<=`` (the paper's definition).  Class version:
    ``ImprovedPrecisionRecall``.

    Args:
        real_features, fake_features: ``[n, D]`` with the same ``D``; each ``n >= k + 1``.
        k: the neighbour that sets a row's radius, an integer ``>= 1``.

    Returns ``(precision, recall)``, float32 scalars on the features' device.
    """
    values = _prdc_checked(real_features, fake_features, k)["values"]
    return values[0], values[1]


def density_coverage(
    real_features: torch.Tensor, fake_features: torch.Tensor, *, k: int = 5
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Density and coverage of ``[M, D]`` generated against ``[N, D]`` real features.

    With ``d2`` and the real radii ``r_i^2`` of ``improved_precision_recall``::

        density  = sum_j #{i : d2(y_j, x_i) <= r_i^2} / (k M)
        coverage = #{i : min_j d2(x_i, y_j) <= r_i^2} / N

    Every comparison is ``<=``; the ``prdc`` package uses ``<``, which differs on exact ties only.
    Class version: ``DensityCoverage``.

    Args:
        real_features, fake_features: ``[n, D]`` with the same ``D``; each ``n >= k + 1``.
        k: the neighbour that sets a row's radius, an integer ``>= 1``.

    Returns ``(density, coverage)``, float32 scalars on the features' device.
    """
    values = _prdc_checked(real_features, fake_features, k)["values"]
    return values[2], values[3]


def _prdc_param_check(k: int) -> None:
    if not isinstance(k, int) or isinstance(k, bool) or k < 1:
        raise ValueError(f"`k` should be an integer greater than or equal to 1, but received {k}.")


def _prdc_input_check(real: torch.Tensor, fake: torch.Tensor, k: int) -> None:
    if real.dim() != 2 or fake.dim() != 2 or real.shape[1] != fake.shape[1] or real.shape[1] < 1:
        raise ValueError(
            "The features should be two-dimensional with the same, non-zero width, "
            f"got shapes {tuple(real.shape)} and {tuple(fake.shape)}."
        )
    if real.shape[0] < k + 1 or fake.shape[0] < k + 1:
        raise ValueError(
            f"`k` = {k} needs at least k + 1 rows on each side, "
            f"got {real.shape[0]} real and {fake.shape[0]} generated."
        )


def _prdc_checked(real: torch.Tensor, fake: torch.Tensor, k: int) -> Dict[str, torch.Tensor]:
    _prdc_param_check(k)
    _prdc_input_check(real, fake, k)
    if _ops.compiling():
        # no inference mode inside a traced graph (as spearman_corrcoef)
        return _prdc(real, fake, k)
    with torch.inference_mode():
        return _prdc(real, fake, k)


def _prdc(real: torch.Tensor, fake: torch.Tensor, k: int, groups: int = 0) -> Dict[str, torch.Tensor]:
    """The statistics of checked features, from whichever path the tensors take:

    ``radii_real`` ``[N]`` / ``radii_fake`` ``[M]`` (float64, squared), ``hits_real`` / ``hits_fake``
    (int32), ``nearest_real`` / ``nearest_fake`` (float64, squared), ``tallies`` (int64 ``[4]``:
    precise rows, recalled rows, total of ``hits_fake``, covered rows) and ``values`` (float32
    ``[4]``: precision, recall, density, coverage).  ``groups`` reaches K22 only (tests).
    """
    if _k22.supported(real, fake, k):
        return _k22.prdc(real, fake, k, groups)
    return _prdc_aten(real, fake, k)


def _d2_block(q: torch.Tensor, nq: torch.Tensor, r: torch.Tensor, nr: torch.Tensor) -> torch.Tensor:
    return ((nq[:, None] + nr[None, :]) - 2.0 * torch.mm(q, r.T)).clamp_(min=0.0)


def _prdc_aten(real: torch.Tensor, fake: torch.Tensor, k: int) -> Dict[str, torch.Tensor]:
    """The definition in FP64 ATen.  Per chunk of query rows one ``[chunk, n_ref]`` distance block
    (``mm``, the clamp, ``+inf`` on the positional diagonal for the self passes), ``topk`` for the
    radii, the compares and sums for the hits; no larger distance tensor exists."""
    x, y = real.double(), fake.double()
    nx, ny = (x * x).sum(dim=1), (y * y).sum(dim=1)

    def chunks(n_query: int, n_ref: int):
        step = max(1, _ATEN_CHUNK_BYTES // (8 * n_ref))
        return [(lo, min(lo + step, n_query)) for lo in range(0, n_query, step)]

    def radii(a: torch.Tensor, na: torch.Tensor) -> torch.Tensor:
        out = []
        for lo, hi in chunks(a.shape[0], a.shape[0]):
            d = _d2_block(a[lo:hi], na[lo:hi], a, na)
            rows = torch.arange(hi - lo, device=a.device)
            d[rows, rows + lo] = float("inf")
            out.append(torch.topk(d, k, dim=1, largest=False).values[:, k - 1])
        return torch.cat(out)

    def cross(q, nq, r, nr, rad) -> Tuple[torch.Tensor, torch.Tensor]:
        hits, nearest = [], []
        for lo, hi in chunks(q.shape[0], r.shape[0]):
            d = _d2_block(q[lo:hi], nq[lo:hi], r, nr)
            hits.append((d <= rad[None, :]).sum(dim=1))
            nearest.append(d.min(dim=1).values)
        return torch.cat(hits).to(torch.int32), torch.cat(nearest)

    radii_r, radii_f = radii(x, nx), radii(y, ny)
    hits_f, nearest_f = cross(y, ny, x, nx, radii_r)
    hits_r, nearest_r = cross(x, nx, y, ny, radii_f)
    tallies = torch.stack([
        (hits_f > 0).sum(), (hits_r > 0).sum(), hits_f.sum(dtype=torch.int64), (nearest_r <= radii_r).sum(),
    ]).to(torch.int64)
    n, m = x.shape[0], y.shape[0]
    divisors = torch.tensor([m, n, k * m, n], dtype=torch.float64, device=x.device)
    return {
        "radii_real": radii_r, "radii_fake": radii_f,
        "hits_real": hits_r, "hits_fake": hits_f,
        "nearest_real": nearest_r, "nearest_fake": nearest_f,
        "tallies": tallies,
        "values": (tallies.double() / divisors).to(torch.float32),
    }
