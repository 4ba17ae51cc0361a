"""K13 (normalized DCG) on one MI355X: the native kernel against this package's ATen form.

Times ``normalized_dcg`` and ``NormalizedDCG.update`` at 65536 x 32 (slates: the wave-per-row
arm) and 8192 x 1000 (the workgroup-per-row arm), float32 scores, int64 relevance, k = 10, each
natively and with ``torcheval_amd.ops.DISABLE_HIP`` set (the ATen form on the same GPU and the
same tensors), the two alternating over several rounds, every window device-synchronised after a
warm-up.  Kernel times come from a separate ``rocprofv3 --kernel-trace --stats`` run of this
script with ``--profile-loop`` (tracing slows the host, so wall times are taken with the profiler
off); pass the resulting ``*_kernel_stats.csv`` (or ``*_results.db``) with ``--kernel-stats`` to
fold them in.

    python benchmarks/bench_ndcg.py --out profiles/ndcg_r9.json
    rocprofv3 --kernel-trace --stats -d DIR -o ndcg -- python benchmarks/bench_ndcg.py --profile-loop --shape 8192x1000
    python benchmarks/bench_ndcg.py --fold RUN.json --kernel-stats 8192x1000=CSV --suite SUITE.json --out profiles/ndcg_r9.json
"""

import argparse
import csv
import json
import os
import sqlite3
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torcheval_amd.ops as ops  # noqa: E402
from torcheval_amd.metrics import NormalizedDCG  # noqa: E402
from torcheval_amd.metrics.functional import normalized_dcg  # noqa: E402

SHAPES = ((65536, 32), (8192, 1000))
K = 10
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


def _inputs(n: int, c: int, dev):
    g = torch.Generator(device=dev).manual_seed(n + c)
    return torch.randn(n, c, device=dev, generator=g), torch.randint(0, 5, (n, c), device=dev, generator=g)


def _kernel_stats(path: str) -> dict:
    """Per-kernel times from rocprofv3: a ``*_kernel_stats.csv`` or, where the profiler writes a
    database instead (``*_results.db``), its ``kernels`` view."""
    if path.endswith(".db"):
        db = sqlite3.connect(path)
        rows = db.execute("select name, count(*), avg(end - start), min(end - start), max(end - start) "
                          "from kernels where name like '%ndcg%' group by name").fetchall()
        db.close()
    else:
        with open(path) as f:
            rows = [(r.get("Name", ""), int(r["Calls"]), float(r["AverageNs"]), float(r["MinNs"]), float(r["MaxNs"]))
                    for r in csv.DictReader(f) if "ndcg" in r.get("Name", "")]
    out = {}
    for name, calls, avg, lo, hi in rows:
        short = "ndcg_finish" if "finish" in name else "ndcg_narrow" if "narrow" in name else "ndcg_wide"
        out[short] = {"calls": calls, "average_us": round(avg / 1e3, 3), "min_us": round(lo / 1e3, 3),
                      "max_us": round(hi / 1e3, 3)}
    return out


def _fold(res: dict, specs) -> None:
    for spec in specs or ():
        shape, path = spec.split("=", 1)
        ks = _kernel_stats(path)
        entry = res["shapes"][shape]
        entry["kernels"] = ks
        rows = ks.get("ndcg_narrow") or ks.get("ndcg_wide")
        if rows:
            t = rows["average_us"] * 1e-6
            entry["row_kernel_read_TB_per_s"] = round(entry["bytes_read"] / t / 1e12, 3)
            entry["row_kernel_time_over_pure_read_bound"] = round(t / (entry["bytes_read"] / HBM_PEAK), 2)


def _write(res: dict, out) -> None:
    print(json.dumps(res, indent=1))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", action="append", default=None, help="SHAPE=CSV, e.g. 8192x1000=stats.csv")
    ap.add_argument("--profile-loop", action="store_true", help="only run the native calls (under rocprofv3)")
    ap.add_argument("--shape", default=None, help="NxC: only this shape")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fold", default=None, help="a JSON of an earlier run: add --kernel-stats to it (no GPU needed)")
    ap.add_argument("--suite", default=None, help="with --fold: a bench_suite.py --out file whose rows to embed")
    args = ap.parse_args()
    if args.fold:
        with open(args.fold) as f:
            res = json.load(f)
        _fold(res, args.kernel_stats)
        if args.suite:  # the bench_suite.py rows of the same visit (--only ormalized --out ...)
            with open(args.suite) as f:
                res["bench_suite_rows"] = json.load(f)["rows"]
        _write(res, args.out)
        return
    dev = torch.device("cuda", 0)
    shapes = SHAPES if args.shape is None else (tuple(int(v) for v in args.shape.split("x")),)
    res = {"device": torch.cuda.get_device_name(0), "scores": "float32", "relevance": "int64", "k": K, "shapes": {}}
    for n, c in shapes:
        x, t = _inputs(n, c, dev)
        m = NormalizedDCG(k=K, device=dev)

        def functional():
            return normalized_dcg(x, t, k=K)

        def update():
            return m.update(x, t)

        if args.profile_loop:
            for _ in range(200):
                functional()
                update()
            torch.cuda.synchronize()
            continue
        native = functional()
        ops.DISABLE_HIP = True
        aten = functional()
        ops.DISABLE_HIP = False
        bytes_read = x.numel() * x.element_size() + t.numel() * t.element_size()
        aten_iters = 50
        res["shapes"][f"{n}x{c}"] = {
            "native_vs_aten_max_abs_diff": float((native.double() - aten.double()).abs().max()),
            "normalized_dcg": _ab(functional, args.rounds, 1000, aten_iters),
            "NormalizedDCG.update": _ab(update, args.rounds, 1000, aten_iters),
            "bytes_read": bytes_read,
            "pure_read_bound_us_at_hbm_peak": round(bytes_read / HBM_PEAK * 1e6, 2),
        }
    if args.profile_loop:
        return
    res["note"] = ("both shapes' inputs (25 MB and 98 MB) fit the 256 MiB Infinity Cache, so repeated calls on the "
                   "same tensors read from it; the bound quoted is the HBM one")
    _fold(res, args.kernel_stats)
    _write(res, args.out)


if __name__ == "__main__":
    main()
