"""K12 (structural similarity) on one MI355X: native kernels against this package's ATen form.

Times ``structural_similarity`` and ``StructuralSimilarity.update`` at 64x3x256x256 float32, each
natively and with ``torcheval_amd.ops.DISABLE_HIP`` set (the ATen chain on the same GPU), the
two alternating over several rounds, every window device-synchronised after a warm-up.  Kernel
times come from a separate ``rocprofv3 --kernel-trace --stats`` run of this script with
``--profile-loop`` (tracing slows the host, so wall times are taken with the profiler off); pass
the resulting ``*_kernel_stats.csv`` with ``--kernel-stats`` to fold them into the JSON.

    python benchmarks/bench_ssim.py --out profiles/ssim_r7.json [--kernel-stats CSV]
    rocprofv3 --kernel-trace --stats -d DIR -o ssim -- python benchmarks/bench_ssim.py --profile-loop
    python benchmarks/bench_ssim.py --fold RUN.json --kernel-stats CSV --suite SUITE.json --out profiles/ssim_r7.json
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
from torcheval_amd.metrics import StructuralSimilarity  # noqa: E402
from torcheval_amd.metrics.functional import structural_similarity  # noqa: E402

SHAPE = (64, 3, 256, 256)
HBM_PEAK = 8.0e12  # bytes / s, spec; about 6.3e12 is reached by a float4 copy


def _window(fn, iters: int) -> float:
    """ms per call over ``iters`` calls ending in a device synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def _device_ms(fn, iters: int) -> float:
    """ms per call between two device events around ``iters`` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _ab(fn, rounds: int, native_iters: int, aten_iters: int) -> dict:
    """Alternate native and ATen windows; medians and the spread over the rounds."""
    res = {"native": [], "aten": []}
    for mode in ("native", "aten"):  # warm up both paths at this shape
        ops.DISABLE_HIP = mode == "aten"
        for _ in range(5):
            fn()
    for _ in range(rounds):
        for mode, iters in (("native", native_iters), ("aten", aten_iters)):
            ops.DISABLE_HIP = mode == "aten"
            res[mode].append(_window(fn, iters))
    ops.DISABLE_HIP = False
    out = {}
    for mode, v in res.items():
        out[f"{mode}_ms"] = round(statistics.median(v), 5)
        out[f"{mode}_ms_min_max"] = [round(min(v), 5), round(max(v), 5)]
    out["aten_over_native"] = round(out["aten_ms"] / out["native_ms"], 2)
    out["native_device_ms"] = round(_device_ms(fn, native_iters), 5)
    return out


def _kernel_stats(path: str) -> dict:
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if "ssim" in name:
                short = "ssim_tiles" if "tiles" in name else "ssim_finish"
                out[short] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 3),
                              "min_us": round(float(row["MinNs"]) / 1e3, 3), "max_us": round(float(row["MaxNs"]) / 1e3, 3)}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--profile-loop", action="store_true", help="only run the native calls (under rocprofv3)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fold", default=None, help="a JSON of an earlier run: add --kernel-stats to it (no GPU needed)")
    ap.add_argument("--suite", default=None, help="with --fold: a bench_suite.py --out file whose rows to embed")
    args = ap.parse_args()
    if args.fold:
        with open(args.fold) as f:
            res = json.load(f)
        _fold(res, args.kernel_stats)
        if args.suite:  # the bench_suite.py rows of the same visit (--only tructural --out ...)
            with open(args.suite) as f:
                res["bench_suite_rows"] = json.load(f)["rows"]
        _write(res, args.out)
        return
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(SHAPE, device=dev, generator=g)
    y = (x + 0.1 * torch.randn(SHAPE, device=dev, generator=g)).clamp(0, 1)
    m = StructuralSimilarity(device=dev)

    def functional():
        return structural_similarity(x, y)

    def update():
        return m.update(x, y)

    if args.profile_loop:
        for _ in range(200):
            functional()
            update()
        torch.cuda.synchronize()
        return

    native = functional()
    ops.DISABLE_HIP = True
    aten = functional()
    ops.DISABLE_HIP = False
    bytes_read = 2 * x.numel() * x.element_size()
    res = {
        "device": torch.cuda.get_device_name(0),
        "shape": list(SHAPE),
        "dtype": "float32",
        "native_vs_aten_abs_diff": abs(float(native) - float(aten)),
        "structural_similarity": _ab(functional, args.rounds, 2000, 100),
        "StructuralSimilarity.update": _ab(update, args.rounds, 2000, 100),
        "bytes_read": bytes_read,
        "pure_read_bound_us_at_hbm_peak": round(bytes_read / HBM_PEAK * 1e6, 2),
        "note": "both inputs (100.7 MB) fit the 256 MiB Infinity Cache, so repeated calls on the same "
                "tensors read from it; the bound quoted is the HBM one",
    }
    if args.kernel_stats:
        _fold(res, args.kernel_stats)
    _write(res, args.out)


def _fold(res: dict, stats_csv: str) -> None:
    ks = _kernel_stats(stats_csv)
    res["kernels"] = ks
    if "ssim_tiles" in ks:
        t = ks["ssim_tiles"]["average_us"] * 1e-6
        res["ssim_tiles_read_TB_per_s"] = round(res["bytes_read"] / t / 1e12, 3)
        res["ssim_tiles_time_over_pure_read_bound"] = round(t / (res["bytes_read"] / HBM_PEAK), 2)


def _write(res: dict, out) -> None:
    print(json.dumps(res, indent=1))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
