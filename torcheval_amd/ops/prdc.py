"""K22 wrapper (csrc/kernels/prdc.hip): the k-nearest-neighbour statistics behind improved
precision / recall and density / coverage.

Per call nine launches on the current stream: ``prdc_norms`` (FP64 row norms of both sets),
``prdc_knn`` + ``prdc_radii`` per set (the k smallest squared distances of every row to the other
rows of its set, kept per block in LDS across 128 x 128 FP32-MFMA tiles, then merged into the k-th),
``prdc_cross`` in both directions (per row the number of rows of the other set whose ball holds it,
and the nearest of them) and ``prdc_finish`` (two launches: hits and nearest per row, then the four
integer tallies and the four values).
No distance is written to memory; no host synchronisation, no atomics.  Native inputs are float32
features with unit stride along the feature axis and any row stride, and ``1 <= k <= 8``; float16 /
bfloat16 features are widened here (one exact copy); everything else is the caller's ATen form.
"""

from typing import Dict

import torch

from torcheval_amd.ops import use_native

# kPrdcTile, kPrdcMaxK, kPrdcCUs, kPrdcMaxGroups, kPrdcBlockStages and kPrdcHitsRows of
# csrc/include/tea_kernels.h (held equal by tests/metrics/image/test_prdc.py): the side of one tile,
# at whose edges the GPU tests place their set sizes, the largest k, the three constants of the
# group rule and the rows per block of the hits launch
TILE = 128
MAX_K = 8
CUS = 256
MAX_GROUPS = 16
BLOCK_STAGES = 12
HITS_ROWS = 256

_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def groups_for(n_query: int, n_ref: int, d: int, groups: int = 0) -> int:
    """Column groups ``G`` of a pass of ``n_query`` rows of width ``d`` over ``n_ref`` columns
    (prdc_groups of the kernel file, where the rule is explained): ``groups >= 1`` as given, clamped
    to the number of column tiles; 0 the ``G <= MAX_GROUPS`` with the smallest modelled time of the
    busiest CU.  A pass writes ``2 G`` lists per row."""
    panels = max(1, (n_query + TILE - 1) // TILE)
    tiles = max(1, (n_ref + TILE - 1) // TILE)
    if groups >= 1:
        return min(groups, tiles)
    stages = max(1, (d + 31) // 32)
    best, best_cost = 1, -1
    for g in range(1, min(tiles, MAX_GROUPS) + 1):  # a plain loop: traced by torch.compile
        c, t = (panels * g + CUS - 1) // CUS, (tiles + g - 1) // g
        cost = c * (t * stages + BLOCK_STAGES) * (4 if c == 1 else 3)
        if best_cost < 0 or cost < best_cost:  # the first of equal costs
            best, best_cost = g, cost
    return best


def hits_blocks(n_r: int, n_f: int) -> int:
    """Blocks of the hits launch (prdc_hits_blocks): rows of ``block_tallies``."""
    return (n_r + HITS_ROWS - 1) // HITS_ROWS + (n_f + HITS_ROWS - 1) // HITS_ROWS


def supported(real: torch.Tensor, fake: torch.Tensor, k: int) -> bool:
    """Whether the call runs K22: ROCm ``[n, D]`` features of the native dtype family on one device
    with unit stride along ``D >= 1``, at least ``k + 1`` rows each and ``1 <= k <= MAX_K``.
    Raises on a GPU without the extension (``use_native``)."""
    if not use_native(real) or fake.device != real.device:
        return False
    if real.dtype not in _DTYPES or fake.dtype not in _DTYPES:
        return False
    if real.dim() != 2 or fake.dim() != 2 or real.shape[1] != fake.shape[1] or real.shape[1] < 1:
        return False
    if not 1 <= k <= MAX_K or min(real.shape[0], fake.shape[0]) < k + 1:
        return False
    if max(real.shape[0], fake.shape[0]) >= 2**31 - TILE or real.shape[1] >= 2**31 - 64:
        return False
    return real.shape[1] == 1 or (real.stride(1) == 1 and fake.stride(1) == 1)


def prdc(real: torch.Tensor, fake: torch.Tensor, k: int, groups: int = 0) -> Dict[str, torch.Tensor]:
    """The statistics of a ``supported`` call, as the dictionary that ``_prdc`` of
    ``metrics.functional.image.prdc`` describes.  ``groups`` forces the number of column groups of
    every pass (tests; 0: the rule of ``groups_for``); no result depends on it.  All ops are
    dispatcher ops only (``torch.ops.torcheval_amd_prdc``), so the call stays in a compiled graph."""
    if real.dtype != torch.float32:
        real = real.float()
    if fake.dtype != torch.float32:
        fake = fake.float()
    ops = torch.ops.torcheval_amd_prdc
    dev = real.device
    n, m, d = real.shape[0], fake.shape[0], real.shape[1]

    def f64(*shape):
        return torch.empty(*shape, dtype=torch.float64, device=dev)

    def i32(*shape):
        return torch.empty(*shape, dtype=torch.int32, device=dev)

    norms_r, norms_f = f64(n), f64(m)
    ops.prdc_norms(real, fake, norms_r, norms_f)
    radii = []
    for feats, norms in ((real, norms_r), (fake, norms_f)):
        rows = feats.shape[0]
        partial = f64(rows, 2 * groups_for(rows, rows, d, groups), k)
        ops.prdc_knn(feats, norms, k, groups, partial)
        radii.append(f64(rows))
        ops.prdc_radii(partial, radii[-1])
    radii_r, radii_f = radii
    lists_f, lists_r = 2 * groups_for(m, n, d, groups), 2 * groups_for(n, m, d, groups)
    counts_f, mins_f = i32(m, lists_f), f64(m, lists_f)
    counts_r, mins_r = i32(n, lists_r), f64(n, lists_r)
    ops.prdc_cross(fake, real, norms_f, norms_r, radii_r, groups, counts_f, mins_f)
    ops.prdc_cross(real, fake, norms_r, norms_f, radii_f, groups, counts_r, mins_r)
    out = {
        "radii_real": radii_r, "radii_fake": radii_f,
        "hits_real": i32(n), "hits_fake": i32(m),
        "nearest_real": f64(n), "nearest_fake": f64(m),
        "tallies": torch.empty(4, dtype=torch.int64, device=dev),
        "values": torch.empty(4, dtype=torch.float32, device=dev),
    }
    block_tallies = torch.empty(hits_blocks(n, m), 4, dtype=torch.int64, device=dev)
    ops.prdc_finish(counts_f, mins_f, counts_r, mins_r, radii_r, k, block_tallies, out["hits_real"], out["hits_fake"],
                    out["nearest_real"], out["nearest_fake"], out["tallies"], out["values"])
    return out
