"""K28 (panoptic quality) on one MI355X: native kernels against this package's ATen form, and K17
``mean_iou``'s label arm on maps of the same pixel count as the streaming yardstick.

The workload is ``32 x 512 x 512`` maps of ``(category, instance)`` with a few dozen blob segments per
image: the category is a thresholded low-pass noise field (5 classes, 3 of them things), the instance
of a thing pixel the 128 x 128 grid cell it lies in, and the prediction is the target's field slightly
perturbed.  It times one ``PanopticQuality.update()`` and one ``panoptic_quality`` call for int64 and
int32 maps, natively and with ``torcheval_amd.ops.DISABLE_HIP`` set (the ATen form on the same GPU and
tensors), the two alternating over several rounds, every window device-synchronised after a warm-up.
Kernel times come from a separate ``rocprofv3 --kernel-trace`` run with ``--profile-loop`` (tracing slows
the host, so wall times are taken with the profiler off); ``--fold`` reads the dispatches from the trace's
rocpd SQLite database.

    python benchmarks/bench_panoptic_quality.py --out RUN.json
    rocprofv3 --kernel-trace -d DIR -o k28 -- python benchmarks/bench_panoptic_quality.py --profile-loop
    python benchmarks/bench_panoptic_quality.py --fold RUN.json --kernel-db DIR/k28_results.db --out RUN.json
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
from torcheval_amd.metrics import PanopticQuality  # noqa: E402
from torcheval_amd.metrics.functional import mean_iou, panoptic_quality  # noqa: E402
from torcheval_amd.ops import panoptic as K  # noqa: E402

SHAPE = (32, 512, 512)
THINGS, STUFFS = (1, 2, 7), (0, 5)
KERNELS = ("panoptic_pairs", "panoptic_match", "panoptic_finish")
METHOD = ("wall: windows of back-to-back calls ending in a device synchronise, native and ATen alternating over "
          "the rounds, medians; kernels: a separate rocprofv3 --kernel-trace run of 100 native int64 updates, us per "
          "launch")


def _maps(dev, dtype):
    g = torch.Generator(device=dev).manual_seed(0)
    field = torch.randn((SHAPE[0], 1) + SHAPE[1:], device=dev, generator=g)
    for _ in range(3):  # a box blur three times over: close to a Gaussian low-pass
        field = torch.nn.functional.avg_pool2d(field, 31, stride=1, padding=15)
    field = field[:, 0] / field.std()
    noisy = field + 0.05 * torch.randn(SHAPE, device=dev, generator=g)
    edges = torch.tensor([-0.9, -0.3, 0.3, 0.9], device=dev)
    cats = torch.tensor(sorted(THINGS + STUFFS), device=dev)
    ys, xs = torch.meshgrid(torch.arange(SHAPE[1], device=dev), torch.arange(SHAPE[2], device=dev), indexing="ij")
    cell = (ys // 128) * (SHAPE[2] // 128) + xs // 128

    def one(f):
        return torch.stack([cats[torch.bucketize(f, edges)], cell.expand(SHAPE)], dim=-1).to(dtype).contiguous()
    return one(noisy), one(field)


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


def _dtype(dtype, rounds: int, native_iters: int, aten_iters: int) -> dict:
    dev = torch.device("cuda", 0)
    p, t = _maps(dev, dtype)
    kw = {"things": THINGS, "stuffs": STUFFS}
    assert K.supported(p, t, 5)
    native = panoptic_quality(p, t, return_sq_and_rq=True, **kw)
    ops.DISABLE_HIP = True
    aten = panoptic_quality(p, t, return_sq_and_rq=True, **kw)
    ops.DISABLE_HIP = False
    segments = torch.unique(t[0].reshape(-1, 2), dim=0).shape[0]
    res = {"dtype": str(dtype), "shape": list(SHAPE) + [2], "target_segments_of_image_0": segments,
           "pq_sq_rq": [round(v, 6) for v in native.tolist()],
           "values_match_aten": bool(torch.isclose(native, aten, rtol=2.0 ** -22, atol=0, equal_nan=True).all())}
    metric = PanopticQuality(device=dev, **kw)
    res["update"] = _ab(lambda: metric.update(p, t), rounds, native_iters, aten_iters)
    res["functional"] = _ab(lambda: panoptic_quality(p, t, **kw), rounds, native_iters, aten_iters)
    # the streaming yardstick: a kernel of the parent commit that reads the same number of pixels
    a, b = p[..., 0].long().contiguous(), t[..., 0].long().contiguous()
    iou = [_window(lambda: mean_iou(a, b, num_classes=8), native_iters) for _ in range(rounds + 1)][1:]
    res["k17_mean_iou_label_arm_int64_ms"] = round(statistics.median(iou), 5)
    return res


def _kernel_times(db_path: str) -> dict:
    """Per K28 kernel the launches and their average / min / max us."""
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
    ap.add_argument("--profile-loop", action="store_true", help="only run native int64 updates (under rocprofv3)")
    ap.add_argument("--fold", default=None, help="a JSON of an earlier run: add --kernel-db to it (no GPU needed)")
    ap.add_argument("--kernel-db", default=None, help="the rocpd database of a --profile-loop trace")
    args = ap.parse_args()
    if args.fold:
        with open(args.fold) as f:
            res = json.load(f)
        res["kernels_int64_update"] = _kernel_times(args.kernel_db)
    elif args.profile_loop:
        p, t = _maps(torch.device("cuda", 0), torch.int64)
        metric = PanopticQuality(device=p.device, things=THINGS, stuffs=STUFFS)
        for _ in range(100):
            metric.update(p, t)
        torch.cuda.synchronize()
        return
    else:
        res = {"device": torch.cuda.get_device_name(0), "method": METHOD,
               "runs": [_dtype(d, args.rounds, args.native_iters, args.aten_iters) for d in (torch.int64, torch.int32)]}
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
