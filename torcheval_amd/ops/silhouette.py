"""K23 wrapper (csrc/kernels/silhouette.hip): the silhouette coefficient of ``[N, D]`` features under
``[N]`` cluster labels.

``plan`` is plumbing in ATen on the device: a stable argsort of the labels, the clusters' counts and
offsets by ``searchsorted`` (``bincount`` would read its output size on the host), every non-empty
cluster padded to whole 128-row panels, and from these the int32 lists the kernels walk.  No size
depends on a device value: the lists are ``max_panels = ceil(N / 128) + K`` panels long, which bounds
``sum_c ceil(n_c / 128)``, and the number of panels in use stays on the device.

Per call four launches on the current stream: ``silhouette_norms`` (FP64 row norms),
``silhouette_tile`` (128 x 128 FP32-MFMA tiles of inner products between a column tile of query
samples and a panel of one cluster's members; distances are formed, square-rooted and summed per
query sample in FP64 registers) and ``silhouette_finish`` (two launches: a thread per sample joins
the panel ranges' partial results into ``a``, ``b`` and ``s``, then one wave takes the mean).
No distance and no ``[N, K]`` table is written to memory; no host synchronisation, no atomics.
Native inputs are float32 features with unit stride along the feature axis and any row stride;
float16 / bfloat16 features are widened here (one exact copy); everything else is the caller's ATen
form.
"""

from typing import Dict, Optional

import torch

from torcheval_amd.ops import use_native

# kSilTile, kSilCUs, kSilMaxGroups, kSilBlockStages, kSilEpilogueStages and kSilStitchRows of
# csrc/include/tea_kernels.h (held equal by tests/metrics/clustering/test_silhouette.py)
TILE = 128
CUS = 256
MAX_GROUPS = 16
BLOCK_STAGES = 12
EPILOGUE_STAGES = 6
STITCH_ROWS = 256

_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def max_panels_for(n: int, num_clusters: int) -> int:
    """The host-side bound of the number of 128-row panels: ``sum_c ceil(n_c / 128) <= n // 128 + K``."""
    return (n + TILE - 1) // TILE + num_clusters


def groups_for(n: int, max_panels: int, d: int, groups: int = 0) -> int:
    """Panel groups ``G`` of a call (silhouette_groups of the kernel file, where the rule is
    explained): ``groups >= 1`` as given, clamped to ``max_panels``; 0 the ``G <= MAX_GROUPS`` with the
    smallest modelled time of the busiest CU."""
    cols = max(1, (n + TILE - 1) // TILE)
    panels = max(1, max_panels)
    if groups >= 1:
        return min(groups, panels)
    stages = max(1, (d + 31) // 32) + EPILOGUE_STAGES
    best, best_cost = 1, -1
    for g in range(1, min(panels, MAX_GROUPS) + 1):  # a plain loop: traced by torch.compile
        c, t = (cols * g + CUS - 1) // CUS, (panels + g - 1) // g
        cost = c * (t * stages + BLOCK_STAGES) * (4 if c == 1 else 3)
        if best_cost < 0 or cost < best_cost:  # the first of equal costs
            best, best_cost = g, cost
    return best


def stitch_blocks(n: int) -> int:
    """Blocks of the stitch launch (silhouette_stitch_blocks): length of ``block_sums``."""
    return (n + STITCH_ROWS - 1) // STITCH_ROWS


def supported(input: torch.Tensor, labels: torch.Tensor, num_clusters: int) -> bool:
    """Whether the call runs K23: ROCm ``[N >= 1, D >= 1]`` features of the native dtype family with
    unit stride along ``D`` and int64 / int32 labels on the same device.  Raises on a GPU without
    the extension (``use_native``)."""
    if not use_native(input) or labels.device != input.device:
        return False
    if input.dtype not in _DTYPES or labels.dtype not in (torch.int64, torch.int32):
        return False
    if input.dim() != 2 or labels.dim() != 1 or input.shape[0] != labels.shape[0]:
        return False
    n, d = input.shape
    if n < 1 or d < 1 or num_clusters < 1:
        return False
    if n >= 2**31 - TILE or d >= 2**31 - 64 or max_panels_for(n, num_clusters) * TILE >= 2**31:
        return False
    return d == 1 or input.stride(1) == 1


def plan(labels: torch.Tensor, num_clusters: int) -> Dict[str, torch.Tensor]:
    """The int32 lists of a call, all on the labels' device and without a host read:

    ``labels`` ``[N]`` (-1 for a label outside ``[0, K)``), ``counts`` ``[K]``, ``ref_index``
    ``[max_panels * 128]`` (the sample of every panel row in cluster order, -1 for padding),
    ``panel_cluster`` ``[max_panels]`` (-1 past the last panel in use) and ``num_panels`` ``[1]``.
    """
    n, k, dev = labels.shape[0], num_clusters, labels.device
    lab = labels.to(torch.int64)
    lab = torch.where((lab >= 0) & (lab < k), lab, k)  # a bad label sorts last, into no cluster
    order = torch.argsort(lab, stable=True)
    bounds = torch.searchsorted(lab[order], torch.arange(k + 1, device=dev))
    starts = bounds[:k]
    counts = bounds[1:] - starts
    panels = (counts + (TILE - 1)) // TILE
    ends = torch.cumsum(panels, 0)
    first = ends - panels
    max_panels = max_panels_for(n, k)
    t = torch.arange(max_panels, device=dev)
    used = t < ends[-1:]
    cluster = torch.searchsorted(ends, t, right=True).clamp_(max=k - 1)  # skips clusters without panels
    slot = torch.arange(max_panels * TILE, device=dev)
    ts = slot // TILE
    c = cluster[ts]
    pos = (ts - first[c]) * TILE + slot % TILE
    member = used[ts] & (pos < counts[c])
    sample = order[(starts[c] + pos).clamp_(0, n - 1)]
    return {
        "labels": torch.where(lab < k, lab, -1).to(torch.int32),
        "counts": counts.to(torch.int32),
        "ref_index": torch.where(member, sample, -1).to(torch.int32),
        "panel_cluster": torch.where(used, cluster, -1).to(torch.int32),
        "num_panels": ends[-1:].to(torch.int32),
    }


def silhouette(input: torch.Tensor, labels: torch.Tensor, num_clusters: int, groups: int = 0,
               err: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The statistics of a ``supported`` call: float64 ``a``, ``b``, ``s`` ``[N]``, float32
    ``samples`` ``[N]``, ``score64`` ``[1]`` and float32 ``score`` ``[1]``.  ``groups`` forces the
    number of panel groups (tests; 0: the rule of ``groups_for``).  ``err`` (int32 ``[1]``) gets bit 0
    set when a label lies outside ``[0, num_clusters)``.  All ops are dispatcher ops only
    (``torch.ops.torcheval_amd_silhouette``), so the call stays in a compiled graph."""
    if input.dtype != torch.float32:
        input = input.float()
    ops = torch.ops.torcheval_amd_silhouette
    dev = input.device
    n, d = input.shape
    p = plan(labels, num_clusters)
    if err is not None:
        err.bitwise_or_((p["labels"] < 0).any().to(err.dtype))

    def f64(*shape):
        return torch.empty(*shape, dtype=torch.float64, device=dev)

    norms = f64(n)
    ops.silhouette_norms(input, norms)
    edges = f64(groups_for(n, max_panels_for(n, num_clusters), d, groups), 4, n)
    ops.silhouette_tile(input, norms, p["labels"], p["ref_index"], p["panel_cluster"], p["counts"], p["num_panels"],
                        groups, edges)
    out = {
        "a": f64(n), "b": f64(n), "s": f64(n),
        "samples": torch.empty(n, dtype=torch.float32, device=dev),
        "score64": f64(1),
        "score": torch.empty(1, dtype=torch.float32, device=dev),
    }
    ops.silhouette_finish(edges, p["labels"], p["panel_cluster"], p["counts"], p["num_panels"], f64(stitch_blocks(n)),
                          out["a"], out["b"], out["s"], out["samples"], out["score64"], out["score"])
    return out
