"""K27 (Hausdorff / average surface distance) on one MI355X: native kernels against this package's ATen
form, and K17 ``dice_score`` on the same maps as a floor.

The search launch's early exit depends on the input, so there are two kinds of ``8 x 512 x 512`` maps
with 4 classes: ``blobs`` (thresholded low-pass noise; the prediction is the target's field slightly
perturbed, so the surfaces are close) and ``sparse`` (classes 1..3 on 2 % of the pixels each,
independently in both maps: isolated surface pixels and long, ragged searches).  Per kind it times
``hausdorff_distance`` (maximum and 95th percentile) and ``average_surface_distance`` natively and with
``torcheval_amd.ops.DISABLE_HIP`` set (the ATen form on the same GPU and tensors), the two alternating
over several rounds, every window device-synchronised after a warm-up.  Kernel times come from a
separate ``rocprofv3 --kernel-trace`` run with ``--profile-loop`` (tracing slows the host, so wall times
are taken with the profiler off); ``--fold`` reads the dispatches from the trace's rocpd SQLite database.

    python benchmarks/bench_surface_distance.py --out RUN.json
    rocprofv3 --kernel-trace -d DIR -o k27 -- python benchmarks/bench_surface_distance.py --profile-loop --kind blobs
    python benchmarks/bench_surface_distance.py --fold RUN.json --kind blobs --kernel-db DIR/k27_results.db --out RUN.json
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
from torcheval_amd.metrics.functional import average_surface_distance, dice_score, hausdorff_distance  # noqa: E402
from torcheval_amd.ops import surface_distance as K  # noqa: E402

SHAPE = (8, 512, 512)
CLASSES = 4
KINDS = ("blobs", "sparse")
CALLS = {
    "hausdorff_distance": lambda p, t: hausdorff_distance(p, t, num_classes=CLASSES),
    "hausdorff_distance(percentile=95)": lambda p, t: hausdorff_distance(p, t, num_classes=CLASSES, percentile=95),
    "average_surface_distance": lambda p, t: average_surface_distance(p, t, num_classes=CLASSES),
}
KERNELS = ("surface_clear", "surface_rows", "surface_search", "surface_finish", "surface_combine")
METHOD = ("wall: windows of back-to-back calls ending in a device synchronise, native and ATen alternating over "
          "the rounds, medians; kernels: a separate rocprofv3 --kernel-trace run of 100 native calls of each "
          "functional of the kind, us per launch")


def _maps(kind: str, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    if kind == "sparse":
        def one():
            r = torch.rand(SHAPE, device=dev, generator=g)
            return (r < 0.06).long() * (1 + (r * 50).long().clamp(max=2))  # classes 1..3 on 2 % each
        return one(), one()
    field = torch.randn((SHAPE[0], 1) + SHAPE[1:], device=dev, generator=g)
    for _ in range(3):  # a box blur three times over: close to a Gaussian low-pass
        field = torch.nn.functional.avg_pool2d(field, 31, stride=1, padding=15)
    field = field[:, 0] / field.std()
    noisy = field + 0.05 * torch.randn(SHAPE, device=dev, generator=g)
    edges = torch.tensor([-0.6, 0.0, 0.6], device=dev)
    return torch.bucketize(noisy, edges), torch.bucketize(field, edges)


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
    for mode in ("native", "aten"):  # warm up both paths
        ops.DISABLE_HIP = mode == "aten"
        for _ in range(2):
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


def _kind(kind: str, rounds: int, native_iters: int, aten_iters: int) -> dict:
    p, t = _maps(kind, torch.device("cuda", 0))
    assert K.supported(p, t, CLASSES)
    res = {"kind": kind, "shape": list(SHAPE), "num_classes": CLASSES, "dtype": "int64"}
    for name, fn in CALLS.items():
        native = fn(p, t)
        ops.DISABLE_HIP = True
        aten = fn(p, t)
        ops.DISABLE_HIP = False
        same = torch.isclose(native, aten, rtol=2.0 ** -22, atol=0, equal_nan=True)
        res[name] = {"values_match_aten": bool(same.all()), "mean_of_finite": float(native[native.isfinite()].mean())}
        res[name].update(_ab(lambda: fn(p, t), rounds, native_iters, aten_iters))
    dice = [_window(lambda: dice_score(p, t, num_classes=CLASSES), native_iters) for _ in range(rounds + 1)][1:]
    res["k17_dice_score_ms"] = round(statistics.median(dice), 5)
    return res


def _kernel_times(db_path: str) -> dict:
    """Per K27 kernel the launches and their average / min / max us."""
    db = sqlite3.connect(db_path)
    rows = db.execute(
        "select s.kernel_name, count(*), avg(d.end - d.start), min(d.end - d.start), max(d.end - d.start) "
        "from rocpd_kernel_dispatch d join rocpd_info_kernel_symbol s on d.kernel_id = s.id group by s.kernel_name")
    out, total = {}, 0.0
    for name, calls, avg, lo, hi in rows:
        for short in KERNELS:
            if short in name:
                out[short] = {"calls": calls, "average_us": round(avg / 1e3, 2), "min_us": round(lo / 1e3, 2),
                              "max_us": round(hi / 1e3, 2)}
                total += avg / 1e3
    out["sum_of_averages_us"] = round(total, 2)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--native-iters", type=int, default=200)
    ap.add_argument("--aten-iters", type=int, default=1)
    ap.add_argument("--kind", choices=KINDS, default=None, help="one kind of maps (default: both)")
    ap.add_argument("--profile-loop", action="store_true", help="only run the native calls (under rocprofv3)")
    ap.add_argument("--fold", default=None, help="a JSON of an earlier run: add --kernel-db to --kind (no GPU needed)")
    ap.add_argument("--kernel-db", default=None, help="the rocpd database of a --profile-loop trace of --kind")
    args = ap.parse_args()
    if args.fold:
        with open(args.fold) as f:
            res = json.load(f)
        next(k for k in res["kinds"] if k["kind"] == args.kind)["kernels"] = _kernel_times(args.kernel_db)
    elif args.profile_loop:
        p, t = _maps(args.kind, torch.device("cuda", 0))
        for fn in CALLS.values():
            for _ in range(100):
                fn(p, t)
        torch.cuda.synchronize()
        return
    else:
        kinds = KINDS if args.kind is None else (args.kind,)
        res = {"device": torch.cuda.get_device_name(0), "method": METHOD,
               "kinds": [_kind(k, args.rounds, args.native_iters, args.aten_iters) for k in kinds]}
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
