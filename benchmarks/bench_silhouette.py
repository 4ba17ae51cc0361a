"""K23 (silhouette coefficient) on one MI355X: the fused tile kernel against the chunked ATen form.

Times ``silhouette_score`` with ``num_clusters`` given on the same GPU and the same tensors along
both routes: K23 (the ATen plan, then four launches) and this package's ATen form (FP64 ``cdist``
from direct differences and a one-hot product, a bounded chunk of query rows at a time), which is
what the call runs with the native route switched off.  Each variant's windows are device-synchronised and
follow a warm-up (five calls of K23, one of the ATen form, which takes seconds).  Kernel times come from a separate
``rocprofv3 --kernel-trace --stats`` run of this script with ``--profile-loop`` (tracing slows the
host, so wall times are taken with the profiler off); pass the resulting ``*_kernel_stats.csv`` with
``--kernel-stats`` to fold them in.  ``mfma_flops`` counts the whole 128 x 128 tiles the tile kernel
runs (column tiles x panels in use, K rounded up to its step of 32); the rate of
``prdc_tile_kernel<Cross>`` at the same N and D (profiles/prdc_r18.json) is the yardstick, since that
kernel has the same main loop.  ``padding_factor`` is panels x 128 / N.

    python benchmarks/bench_silhouette.py --out profiles/silhouette_r19.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o sil -- python benchmarks/bench_silhouette.py --profile-loop --shape 10000x64k10
    python benchmarks/bench_silhouette.py --fold RUN.json --kernel-stats 10000x64k10=CSV --out profiles/silhouette_r19.json
"""

import argparse
import csv
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.bench_spearman import _alternate, _aten, _window, _write  # noqa: E402
from torcheval_amd.metrics.functional import silhouette_score  # noqa: E402
from torcheval_amd.metrics.functional.clustering.silhouette import _silhouette, _silhouette_aten  # noqa: E402
from torcheval_amd.ops import silhouette as K  # noqa: E402

# key: (N, D, clusters, native calls per window, ATen calls per window)
SHAPES = {
    "10000x64k10": (10000, 64, 10, 20, 2),
    "50000x128k100": (50000, 128, 100, 3, 1),
    "10000x2048k10": (10000, 2048, 10, 10, 1),
    "50000x16k1000": (50000, 16, 1000, 3, 1),
}


def _kernel_stats(path: str) -> dict:
    """Per-kernel times of a rocprofv3 ``*_kernel_stats.csv``: K23's kernels, the templates under
    their load arm."""
    out = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            if "silhouette_" not in name:
                continue
            short = name[name.index("silhouette_"):].split("(")[0].rstrip("<")
            if "<" in name[name.index("silhouette_"):].split("(")[0]:
                short = f"{short.split('<')[0]}<{'16-byte' if 'true>' in name else 'element'} loads>"
            out[short] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 3),
                          "min_us": round(float(r["MinNs"]) / 1e3, 3), "max_us": round(float(r["MaxNs"]) / 1e3, 3)}
    return out


def _fold_kernels(res: dict, specs) -> None:
    for spec in specs or ():
        key, path = spec.split("=", 1)
        res["kernels"][key] = _kernel_stats(path)
        flops = res["shapes"].get(key, {}).get("mfma_flops")
        for name, v in res["kernels"][key].items():
            if flops and name.startswith("silhouette_tile_kernel"):
                v["tflops"] = round(flops / (v["average_us"] * 1e-6) / 1e12, 1)


def _data(n: int, d: int, k: int, dev):
    """Centres plus noise, cluster sizes about equal, labels in random order."""
    g = torch.Generator(device=dev).manual_seed(n + d + k)
    labels = torch.randint(0, k, (n,), device=dev, generator=g)
    x = torch.rand(k, d, device=dev, generator=g)[labels] + 0.35 * torch.rand(n, d, device=dev, generator=g)
    return x, labels


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", action="append", default=None, help="KEY=CSV, e.g. 10000x64k10=stats.csv")
    ap.add_argument("--profile-loop", action="store_true", help="only run the native calls (under rocprofv3)")
    ap.add_argument("--shape", default=None, help="a key of SHAPES: only this shape")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-aten", action="store_true", help="skip the ATen form (it takes seconds per call)")
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
        n, d, k, native_iters, aten_iters = SHAPES[key]
        x, labels = _data(n, d, k, dev)

        def score():
            return silhouette_score(x, labels, num_clusters=k)

        if args.profile_loop:
            for _ in range(max(2, native_iters // 2)):
                score()
            torch.cuda.synchronize()
            continue

        panels = int(K.plan(labels, k)["num_panels"])
        max_panels = K.max_panels_for(n, k)
        groups = K.groups_for(n, max_panels, d)
        col_tiles = (n + K.TILE - 1) // K.TILE
        native = _silhouette(x, labels, k)
        entry = {
            "clusters": k, "panels": panels, "max_panels": max_panels, "padding_factor": round(panels * K.TILE / n, 4),
            "groups": groups, "blocks": col_tiles * groups,
            "mfma_flops": col_tiles * panels * 2 * K.TILE * K.TILE * (-(-d // 32) * 32),
            "score_native": float(native["score64"]),
        }
        entry["silhouette_score"] = _alternate({"native": score}, {"native": native_iters}, args.rounds)
        if not args.no_aten:
            aten = _silhouette_aten(x, labels, k)  # also the ATen form's one warm-up call: it takes seconds
            entry["score_aten"] = float(aten["score64"])
            entry["samples_max_abs_diff"] = float((native["s"] - aten["s"]).abs().max())
            del aten
            windows = sorted(_window(_aten(score), aten_iters) for _ in range(args.rounds))
            entry["silhouette_score"]["aten_ms"] = round(windows[len(windows) // 2], 5)
            entry["silhouette_score"]["aten_ms_min_max"] = [round(windows[0], 5), round(windows[-1], 5)]
        res["shapes"][key] = entry
        del native
        torch.cuda.empty_cache()
    if args.profile_loop:
        return
    res["note"] = ("native: K23 (the ATen plan: argsort, searchsorted and index arithmetic; then norms, tile, stitch, "
                   "finish); aten: the same call with the native route off (chunked FP64 cdist from direct differences "
                   "and a one-hot product) on the same tensors; centres plus noise, labels in random order, "
                   "num_clusters given (no host sync); medians of the rounds' windows with their minimum and maximum")
    _fold_kernels(res, args.kernel_stats)
    _write(res, args.out)


if __name__ == "__main__":
    main()
