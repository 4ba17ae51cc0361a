"""K25 (indices of a contingency table) on one MI355X: the HIP kernels against this package's ATen form.

``update``: one update of 10^7 uniformly random label pairs into an int64 ``[R, C]`` table at 10 x 10,
1000 x 1000 and 2000 x 2000, along three routes on the same tensors: K25 with the slice the rule of
``ops.contingency.plan`` picks, K25 with the other slice forced (the A/B of the rule), and the ATen form
(``bincount`` of ``true * C + pred``).  ``slice_sweep``: both slices forced at 10 x 10 and 64 x 64 (tables either slice holds whole) for 10^4 to
10^7 pairs, back-to-back calls.  ``compute``: AMI and ARI of a 1000 x 1000 table of 10^6 pairs, K25
(statistics, EMI, values) against the ATen form (``lgamma`` over ``[R, C]`` with a loop over ``n``).
``emi_accuracy``: ``|EMI - oracle| / sum |term|`` of the device EMI against the exact-rational oracle of
tests/_contingency_oracle.py on the cases of tests/gpu/test_k25_contingency.py; the largest is the
figure that test's bound is four times of.  Windows are device-synchronised and follow a warm-up;
medians over the rounds with their minimum and maximum.

    python benchmarks/bench_clustering_indices.py --out profiles/clustering_indices_r39.json
"""

import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.bench_spearman import _alternate, _window, _write  # noqa: E402
from torcheval_amd.metrics.functional.clustering.contingency import _contingency_aten, _values_aten  # noqa: E402
from torcheval_amd.ops import contingency as K  # noqa: E402

UPDATE_PAIRS = 10**7
UPDATE_SHAPES = ((10, 10), (1000, 1000), (2000, 2000))
COMPUTE_SHAPE, COMPUTE_PAIRS = (1000, 1000), 10**6
SWEEP_SHAPES, SWEEP_PAIRS = ((10, 10), (64, 64)), (10**4, 10**5, 10**6, 10**7)


def _labels(n, r, c, dev):
    g = torch.Generator(device=dev).manual_seed(n + r + c)
    return torch.randint(0, r, (n,), device=dev, generator=g), torch.randint(0, c, (n,), device=dev, generator=g)


def _median(windows):
    windows = sorted(windows)
    return {"ms": round(windows[len(windows) // 2], 5), "ms_min_max": [round(windows[0], 5), round(windows[-1], 5)]}


def _emi_accuracy(dev):
    from tests import _contingency_oracle as O

    out = {}
    for key, (a, b) in O.EMI_CASES.items():
        want, mag = O.emi_oracle(a, b)
        table = torch.from_numpy(O.fill(a, b)).to(dev)
        got = float(K.contingency_emi(K.contingency_stats(table), len(a), len(b)).sum(dim=1)[0])
        n = sum(a)
        out[key] = {"n": n, "emi": got, "oracle": want, "sum_abs_terms": mag,
                    "ratio": abs(got - want) / mag if mag > 0 else float(got != want),
                    "ceiling": 64 * O.U * math.lgamma(n + 1)}
    out["largest_ratio"] = max(v["ratio"] for v in out.values())
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-aten", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "update": {}, "slice_sweep": {}, "compute": {}}
    for r, c in UPDATE_SHAPES:
        t, p = _labels(UPDATE_PAIRS, r, c, dev)
        table = torch.zeros(r, c, dtype=torch.int64, device=dev)
        picked, groups = K.plan(UPDATE_PAIRS, r * c)
        other = K.SLICE_LARGE if picked == K.SLICE_SMALL else K.SLICE_SMALL
        fns = {"native": lambda: K.contingency_update(t, p, table),
               "native_other_slice": lambda: K.contingency_update(t, p, table, None, other)}
        entry = {"pairs": UPDATE_PAIRS, "slice": picked, "groups": groups, "other_slice": other,
                 "other_groups": K.plan(UPDATE_PAIRS, r * c, other)[1]}
        entry.update(_alternate(fns, {"native": 10, "native_other_slice": 10}, args.rounds))
        table.zero_()
        K.contingency_update(t, p, table)
        if not args.no_aten:
            ref = _contingency_aten(t, p, r, c)
            entry["equal_to_aten"] = bool(torch.equal(ref, table))
            entry["aten"] = _median([_window(lambda: _contingency_aten(t, p, r, c), 3) for _ in range(args.rounds)])
        res["update"][f"{r}x{c}"] = entry
        del t, p, table
        torch.cuda.empty_cache()

    # the two slices where both hold the whole table, over the update's length: what the rule of plan() rests on
    for (r, c), n in ((shape, n) for shape in SWEEP_SHAPES for n in SWEEP_PAIRS):
        t, p = _labels(n, r, c, dev)
        table = torch.zeros(r, c, dtype=torch.int64, device=dev)
        fns = {"small": lambda: K.contingency_update(t, p, table, None, K.SLICE_SMALL),
               "large": lambda: K.contingency_update(t, p, table, None, K.SLICE_LARGE)}
        entry = {"picked": K.plan(n, r * c)[0], "groups_small": K.plan(n, r * c, K.SLICE_SMALL)[1],
                 "groups_large": K.plan(n, r * c, K.SLICE_LARGE)[1]}
        entry.update(_alternate(fns, {"small": 50, "large": 50}, args.rounds))
        res["slice_sweep"][f"{r}x{c}/{n}"] = entry

    r, c = COMPUTE_SHAPE
    t, p = _labels(COMPUTE_PAIRS, r, c, dev)
    table = torch.zeros(r, c, dtype=torch.int64, device=dev)
    K.contingency_update(t, p, table)
    ami, ari = K.INDEX["adjusted_mutual_info"] + 2, K.INDEX["adjusted_rand"]
    fns = {"ami_native": lambda: K.contingency_values(table, True)[0][ami],
           "ari_native": lambda: K.contingency_values(table, False)[0][ari]}
    entry = {"pairs": COMPUTE_PAIRS, "emi_parts": K.emi_parts(r, c), "emi_blocks": K.emi_blocks(r, c)}
    entry.update(_alternate(fns, {"ami_native": 10, "ari_native": 20}, args.rounds))
    native = K.contingency_values(table, True)[0]
    entry["ami"], entry["ari"] = float(native[ami]), float(native[ari])
    if not args.no_aten:
        aten = _values_aten(table, True)  # also the ATen form's warm-up
        entry["ami_aten_value"], entry["ari_aten_value"] = float(aten[ami]), float(aten[ari])
        entry["values_max_abs_diff"] = float((native - aten).abs().max())
        entry["ami_aten"] = _median([_window(lambda: _values_aten(table, True)[ami], 1) for _ in range(3)])
        entry["ari_aten"] = _median([_window(lambda: _values_aten(table, False)[ari], 5) for _ in range(args.rounds)])
    res["compute"][f"{r}x{c}"] = entry
    res["emi_accuracy"] = _emi_accuracy(dev)
    res["note"] = ("update: 10^7 uniformly random int64 label pairs into a zero-initialised table that keeps accumulating; "
                   "native: the slice of ops.contingency.plan, native_other_slice: the other instantiation forced; "
                   "aten: bincount(true * C + pred) (it reads its output size on the host).  compute: the values vector "
                   "of one table, with the expected mutual information (ami) and without (ari); the ATen form of ami "
                   "reads the largest n on the host and loops over n.  Medians of the rounds' windows.")
    _write(res, args.out)


if __name__ == "__main__":
    main()
