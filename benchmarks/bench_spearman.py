"""K14 (Spearman rank correlation) on one MI355X: the native path against this package's ATen form.

Times ``spearman_corrcoef`` and ``SpearmanCorrCoef.compute`` at 1 x 1M, 8 x 131072 and 100 x 10000,
float32, continuous and with 50-level ties, each natively and with ``torcheval_amd.ops.DISABLE_HIP``
set (the ATen form on the same GPU and the same tensors), the two alternating over several rounds,
every window device-synchronised after a warm-up.  Kernel times come from a separate
``rocprofv3 --kernel-trace --stats`` run of this script with ``--profile-loop`` (tracing slows the
host, so wall times are taken with the profiler off); pass the resulting ``*_kernel_stats.csv`` with
``--kernel-stats`` to fold them in.

    python benchmarks/bench_spearman.py --out profiles/spearman_r10.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o sp -- python benchmarks/bench_spearman.py --profile-loop --shape 1x1048576
    python benchmarks/bench_spearman.py --fold RUN.json --kernel-stats 1x1048576=CSV --out profiles/spearman_r10.json
"""

import argparse
import csv
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torcheval_amd.ops as ops  # noqa: E402
from torcheval_amd.metrics import SpearmanCorrCoef  # noqa: E402
from torcheval_amd.metrics.functional import spearman_corrcoef  # noqa: E402

SHAPES = ((1, 1 << 20), (8, 131072), (100, 10000))
LEVELS = (None, 50)
HBM_PEAK = 8.0e12  # bytes / s, spec; about 6.3e12 is reached by a float4 copy


def _window(fn, iters: int) -> float:
    """ms per call over ``iters`` calls ending in a device synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def _alternate(fns: dict, iters: dict, rounds: int) -> dict:
    """Alternate the named variants' windows; medians and the spread over the rounds."""
    res = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(5):
            fn()
    for _ in range(rounds):
        for k, fn in fns.items():
            res[k].append(_window(fn, iters[k]))
    out = {}
    for k, v in res.items():
        out[f"{k}_ms"] = round(statistics.median(v), 5)
        out[f"{k}_ms_min_max"] = [round(min(v), 5), round(max(v), 5)]
    return out


def _aten(fn):
    def run():
        ops.DISABLE_HIP = True
        try:
            return fn()
        finally:
            ops.DISABLE_HIP = False
    return run


def _inputs(rows: int, n: int, levels, dev):
    g = torch.Generator(device=dev).manual_seed(rows + n)
    x = torch.rand(rows, n, device=dev, generator=g)
    y = 0.6 * x + 0.4 * torch.rand(rows, n, device=dev, generator=g)
    if levels is not None:
        x, y = torch.floor(x * levels), torch.floor(y * levels)
    return (x[0], y[0]) if rows == 1 else (x, y)


def _kernel_stats(path: str) -> dict:
    """Per-kernel times of a rocprofv3 ``*_kernel_stats.csv``: every kernel of the traced loop."""
    out = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "").replace("(anonymous namespace)::", "").replace("void ", "")
            name = name.split("(")[0].replace("tea::", "")[-72:]
            out[name] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 3),
                         "min_us": round(float(r["MinNs"]) / 1e3, 3), "max_us": round(float(r["MaxNs"]) / 1e3, 3)}
    return out


def _fold(res: dict, specs) -> None:
    for spec in specs or ():
        key, path = spec.split("=", 1)
        res["kernels"][key] = _kernel_stats(path)


def _write(res: dict, out) -> None:
    print(json.dumps(res, indent=1))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", action="append", default=None, help="KEY=CSV, e.g. 1x1048576=stats.csv")
    ap.add_argument("--profile-loop", action="store_true", help="only run the native calls (under rocprofv3)")
    ap.add_argument("--shape", default=None, help="ROWSxN: only this shape")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fold", default=None, help="a JSON of an earlier run: add --kernel-stats to it (no GPU needed)")
    args = ap.parse_args()
    if args.fold:
        with open(args.fold) as f:
            res = json.load(f)
        _fold(res, args.kernel_stats)
        _write(res, args.out)
        return
    dev = torch.device("cuda", 0)
    shapes = SHAPES if args.shape is None else (tuple(int(v) for v in args.shape.split("x")),)
    res = {"device": torch.cuda.get_device_name(0), "dtype": "float32", "shapes": {}, "kernels": {}}
    for rows, n in shapes:
        for levels in LEVELS:
            x, y = _inputs(rows, n, levels, dev)
            tasks = rows
            m = SpearmanCorrCoef(num_tasks=tasks, device=dev).update(x, y)

            def functional():
                return spearman_corrcoef(x, y, num_tasks=tasks)

            if args.profile_loop:
                if levels is None:
                    for _ in range(200):
                        functional()
                    torch.cuda.synchronize()
                continue
            native, aten = functional(), _aten(functional)()
            big = rows * n >= 1 << 20
            iters = {"native": 300, "aten": 30 if big else 60}
            bytes_read = 2 * rows * n * 4
            res["shapes"][f"{rows}x{n}" + ("" if levels is None else f" ties{levels}")] = {
                "native_vs_aten_max_abs_diff": float((native.double() - aten.double()).abs().max()),
                "spearman_corrcoef": _alternate({"native": functional, "aten": _aten(functional)}, iters,
                                                args.rounds),
                "SpearmanCorrCoef.compute": _alternate({"native": m.compute, "aten": _aten(m.compute)}, iters,
                                                       args.rounds),
                "bytes_read": bytes_read,
                "pure_read_bound_us_at_hbm_peak": round(bytes_read / HBM_PEAK * 1e6, 2),
            }
    if args.profile_loop:
        return
    res["note"] = ("every shape's operands (8 MB) fit the 256 MiB Infinity Cache, so repeated calls on the same "
                   "tensors read from it; the bound quoted is the HBM one")
    _fold(res, args.kernel_stats)
    _write(res, args.out)


if __name__ == "__main__":
    main()
