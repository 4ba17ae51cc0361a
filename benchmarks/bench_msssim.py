"""K26 (multi-scale SSIM) on one MI355X: native kernels against this package's ATen form and K12.

Per case times ``multiscale_structural_similarity`` and ``MultiScaleStructuralSimilarity.update``,
each natively and with ``torcheval_amd.ops.DISABLE_HIP`` set (the ATen form on the same GPU and
tensors), the two alternating over several rounds, every window device-synchronised after a warm-up;
and K12 ``structural_similarity`` on the level-0 pair as the second yardstick.  Kernel times come
from a separate ``rocprofv3 --kernel-trace`` run with ``--profile-loop`` (tracing slows the host, so
wall times are taken with the profiler off); ``--fold`` reads every dispatch from the trace's rocpd
SQLite database (``*_results.db``) and adds them to a case of the JSON, one entry per kernel and, for
the level kernel, per tile grid (a call launches it once per level).

    python benchmarks/bench_msssim.py --out RUN.json
    rocprofv3 --kernel-trace -d DIR -o k26 -- python benchmarks/bench_msssim.py --profile-loop --case 0
    python benchmarks/bench_msssim.py --fold RUN.json --case 0 --kernel-db DIR/k26_results.db --out RUN.json
"""

import argparse
import json
import os
import sqlite3
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torcheval_amd.ops as ops  # noqa: E402
from torcheval_amd.metrics import MultiScaleStructuralSimilarity  # noqa: E402
from torcheval_amd.metrics.functional import multiscale_structural_similarity, structural_similarity  # noqa: E402
from torcheval_amd.ops import msssim as K  # noqa: E402

# (shape, dtype, kernel_size, native iterations, ATen iterations); five levels, the default betas
CASES = [
    ((64, 3, 256, 256), torch.float32, 11, 1000, 20),
    ((64, 3, 256, 256), torch.uint8, 11, 1000, 20),
    ((16, 3, 1024, 1024), torch.float32, 11, 300, 5),
    ((256, 3, 64, 64), torch.float32, 3, 1000, 20),  # every level in the tail launch
]


def _window(fn, iters: int) -> float:
    """ms per call over ``iters`` calls ending in a device synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def _ab(fn, rounds: int, native_iters: int, aten_iters: int) -> dict:
    """Alternate native and ATen windows; medians and the spread over the rounds."""
    res = {"native": [], "aten": []}
    for mode in ("native", "aten"):  # warm up both paths at this shape
        ops.DISABLE_HIP = mode == "aten"
        for _ in range(3):
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
    return out


def _inputs(shape, dtype, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(shape, device=dev, generator=g)
    y = (x + 0.1 * torch.randn(shape, device=dev, generator=g)).clamp(0, 1)
    if dtype == torch.uint8:
        return (x * 255).round().to(dtype), (y * 255).round().to(dtype), 255.0
    return x.to(dtype), y.to(dtype), 1.0


def _case(case, rounds: int) -> dict:
    shape, dtype, ks, native_iters, aten_iters = case
    dev = torch.device("cuda", 0)
    x, y, rng = _inputs(shape, dtype, dev)
    m = MultiScaleStructuralSimilarity(rng, kernel_size=ks, device=dev)
    assert K.supported(x, y, ks, 5)

    def functional():
        return multiscale_structural_similarity(x, y, rng, kernel_size=ks)

    native = float(functional())
    ops.DISABLE_HIP = True
    aten = float(functional())
    ops.DISABLE_HIP = False
    k12 = [_window(lambda: structural_similarity(x, y, rng, kernel_size=ks), native_iters) for _ in range(rounds + 1)][1:]
    plan = K.plan(shape[2], shape[3], ks, 5)
    res = {
        "shape": list(shape), "dtype": str(dtype).replace("torch.", ""), "kernel_size": ks, "levels": 5,
        "level_launches": plan["tail"], "tail_levels": 5 - plan["tail"],
        "native_vs_aten_abs_diff": abs(native - aten),
        "multiscale_structural_similarity": _ab(functional, rounds, native_iters, aten_iters),
        "MultiScaleStructuralSimilarity.update": _ab(lambda: m.update(x, y), rounds, native_iters, aten_iters),
        "k12_structural_similarity_ms": round(statistics.median(k12), 5),
    }
    res["native_over_k12"] = round(res["multiscale_structural_similarity"]["native_ms"] / res["k12_structural_similarity_ms"], 2)
    return res


METHOD = ("wall: windows of back-to-back calls ending in a device synchronise, native and ATen alternating over "
          "the rounds, medians; kernels: a separate rocprofv3 --kernel-trace run of 100 native calls of the case, "
          "us per launch")


def _kernel_times(db_path: str) -> dict:
    """Per K26 kernel (the level kernel: per tile grid) the launches and their average / min / max us."""
    db = sqlite3.connect(db_path)
    rows = db.execute(
        "select s.kernel_name, d.grid_size_y, d.grid_size_z, count(*), avg(d.end - d.start), min(d.end - d.start), "
        "max(d.end - d.start) from rocpd_kernel_dispatch d join rocpd_info_kernel_symbol s on d.kernel_id = s.id "
        "group by s.kernel_name, d.grid_size_y, d.grid_size_z order by d.grid_size_y * d.grid_size_z desc")
    out, total = {}, 0.0
    for name, gy, gz, calls, avg, lo, hi in rows:
        for short in ("msssim_level", "msssim_tail", "msssim_finish"):
            if short in name:
                key = f"{short} ({gz}x{gy} tiles)" if short == "msssim_level" else short
                out[key] = {"calls": calls, "average_us": round(avg / 1e3, 2), "min_us": round(lo / 1e3, 2),
                            "max_us": round(hi / 1e3, 2)}
                total += avg / 1e3
    out["sum_of_averages_us"] = round(total, 2)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--case", type=int, default=None, help="one case of CASES (default: all)")
    ap.add_argument("--profile-loop", action="store_true", help="only run the native calls (under rocprofv3)")
    ap.add_argument("--fold", default=None, help="a JSON of an earlier run: add --kernel-db to --case (no GPU needed)")
    ap.add_argument("--kernel-db", default=None, help="the rocpd database of a --profile-loop trace of --case")
    args = ap.parse_args()
    if args.fold:
        with open(args.fold) as f:
            res = json.load(f)
        res["cases"][args.case]["kernels"] = _kernel_times(args.kernel_db)
    elif args.profile_loop:
        shape, dtype, ks, _, _ = CASES[args.case]
        x, y, rng = _inputs(shape, dtype, torch.device("cuda", 0))
        for _ in range(100):
            multiscale_structural_similarity(x, y, rng, kernel_size=ks)
        torch.cuda.synchronize()
        return
    else:
        cases = CASES if args.case is None else [CASES[args.case]]
        res = {"device": torch.cuda.get_device_name(0), "method": METHOD,
               "cases": [_case(c, args.rounds) for c in cases]}
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
