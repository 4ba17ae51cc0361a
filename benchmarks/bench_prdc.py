"""K22 (precision / recall, density / coverage) on one MI355X: the fused tile kernel against the
chunked ATen form.

Times ``improved_precision_recall`` (k = 3) and ``density_coverage`` (k = 5) on the same GPU and
the same tensors along both routes: K22 (nine launches) and this package's ATen form (FP64 ``mm``,
clamp, ``topk`` and compares, a bounded chunk of query rows at a time), which is what the call runs
with the native route switched off.  The variants' windows alternate over several rounds, each
device-synchronised after a warm-up.  Kernel times come from a separate
``rocprofv3 --kernel-trace --stats`` run of this script with ``--profile-loop`` (tracing slows the
host, so wall times are taken with the profiler off); pass the resulting ``*_kernel_stats.csv`` with
``--kernel-stats`` to fold them in.  ``mfma_flops`` counts whole 128 x 128 tiles with K rounded up to
its step of 32, per pass; the rate of ``kid_gram_kernel`` at the same D (profiles/kid_r16.json) is
the yardstick.

    python benchmarks/bench_prdc.py --out profiles/prdc_r18.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o prdc -- python benchmarks/bench_prdc.py --profile-loop --shape 10000x2048
    python benchmarks/bench_prdc.py --fold RUN.json --kernel-stats 10000x2048=CSV --out profiles/prdc_r18.json
"""

import argparse
import csv
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.bench_spearman import _alternate, _aten, _write  # noqa: E402
from torcheval_amd.metrics.functional import density_coverage, improved_precision_recall  # noqa: E402
from torcheval_amd.metrics.functional.image.prdc import _prdc, _prdc_aten  # noqa: E402
from torcheval_amd.ops import prdc as K  # noqa: E402

# key: (rows per side, D, native calls per window, ATen calls per window)
SHAPES = {
    "10000x2048": (10000, 2048, 10, 2),
    "50000x2048": (50000, 2048, 2, 1),
    "10000x64": (10000, 64, 20, 2),
}


def _tiles(n: int) -> int:
    return (n + K.TILE - 1) // K.TILE


def _pass_flops(n_query: int, n_ref: int, d: int) -> int:
    """Flops one tile-kernel pass runs: whole tiles, K rounded up to its step of 32."""
    return _tiles(n_query) * _tiles(n_ref) * 2 * K.TILE * K.TILE * (-(-d // 32) * 32)


def _kernel_stats(path: str) -> dict:
    """Per-kernel times of a rocprofv3 ``*_kernel_stats.csv``: K22's kernels, the tile kernel's
    instantiations under their template arguments (bench_spearman's reader cuts names at the first
    parenthesis, which here sits inside the argument list)."""
    out = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            if "prdc_" not in name:
                continue
            short = name[name.index("prdc_"):].split("(")[0].rstrip("<")
            if short == "prdc_tile_kernel":
                mode = "Knn" if "Mode)0" in name else "Cross"
                short = f"prdc_tile_kernel<{mode}, {'16-byte' if 'true>' in name else 'element'} loads>"
            out[short] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 3),
                          "min_us": round(float(r["MinNs"]) / 1e3, 3), "max_us": round(float(r["MaxNs"]) / 1e3, 3)}
    return out


def _fold_kernels(res: dict, specs) -> None:
    for spec in specs or ():
        key, path = spec.split("=", 1)
        res["kernels"][key] = _kernel_stats(path)
        flops = res["shapes"].get(key, {}).get("mfma_flops_per_pass")
        for name, v in res["kernels"][key].items():
            if flops and name.startswith("prdc_tile_kernel"):  # both passes of an instantiation run these flops
                v["tflops"] = round(flops / (v["average_us"] * 1e-6) / 1e12, 1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", action="append", default=None, help="KEY=CSV, e.g. 10000x2048=stats.csv")
    ap.add_argument("--profile-loop", action="store_true", help="only run the native calls (under rocprofv3)")
    ap.add_argument("--shape", default=None, help="a key of SHAPES: only this shape")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fold", default=None, help="a JSON of an earlier run: add --kernel-stats to it (no GPU needed)")
    args = ap.parse_args()
    if args.fold:
        with open(args.fold) as f:
            res = json.load(f)
        _fold_kernels(res, args.kernel_stats)
        _write(res, args.out)
        return
    dev = torch.device("cuda", 0)
    keys = list(SHAPES) if args.shape is None else [args.shape]
    res = {"device": torch.cuda.get_device_name(0), "dtype": "float32", "tile": K.TILE, "shapes": {}, "kernels": {}}
    for key in keys:
        n, d, native_iters, aten_iters = SHAPES[key]
        g = torch.Generator(device=dev).manual_seed(n + d)
        real = torch.rand(n, d, device=dev, generator=g)
        fake = torch.rand(n, d, device=dev, generator=g) + 0.02

        def core(k):
            return lambda: K.prdc(real, fake, k)["values"]

        if args.profile_loop:
            for _ in range(max(2, native_iters // 2)):
                core(3)()
            torch.cuda.synchronize()
            continue

        def ipr():
            return improved_precision_recall(real, fake, k=3)

        def dc():
            return density_coverage(real, fake, k=5)

        native3, native5 = _prdc(real, fake, 3), _prdc(real, fake, 5)
        aten3, aten5 = _prdc_aten(real, fake, 3), _prdc_aten(real, fake, 5)
        iters = {"native": native_iters, "aten": aten_iters}
        res["shapes"][key] = {
            "groups": K.groups_for(n, n, d), "blocks_per_pass": _tiles(n) * K.groups_for(n, n, d),
            "mfma_flops_per_pass": _pass_flops(n, n, d),
            "values_k3_native": native3["values"].tolist(), "values_k3_aten": aten3["values"].tolist(),
            "values_k5_native": native5["values"].tolist(), "values_k5_aten": aten5["values"].tolist(),
            "tallies_k3_native_minus_aten": (native3["tallies"] - aten3["tallies"]).tolist(),
            "tallies_k5_native_minus_aten": (native5["tallies"] - aten5["tallies"]).tolist(),
            "radii_real_k3_max_abs_diff": float((native3["radii_real"] - aten3["radii_real"]).abs().max()),
            "improved_precision_recall_k3": _alternate({"native": ipr, "aten": _aten(ipr)}, iters, args.rounds),
            "density_coverage_k5": _alternate({"native": dc, "aten": _aten(dc)}, iters, args.rounds),
        }
        del native3, native5, aten3, aten5
        torch.cuda.empty_cache()
    if args.profile_loop:
        return
    res["note"] = ("native: K22, nine launches (norms, knn + radii per set, cross in both directions, hits, finish); "
                   "aten: the same call with the native route off (chunked FP64 mm, clamp, topk, compares) on the same "
                   "tensors; real = rand, fake = rand + 0.02, equal row counts; medians of the rounds' windows with "
                   "their minimum and maximum")
    _fold_kernels(res, args.kernel_stats)
    _write(res, args.out)


if __name__ == "__main__":
    main()
