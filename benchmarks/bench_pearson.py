"""K16 (Pearson / concordance correlation) on one MI355X: the native path against this package's ATen form.

Times ``pearson_corrcoef`` and ``PearsonCorrCoef.update`` at 1 x 2^20 (float32 and bfloat16),
1 x 2^20 bfloat16 with ``target`` one element off ``input``'s 16-byte alignment (element loads for
``target``), 8 x 131072, 100 x 10000, the ``.t()`` view of a row-major 8192 x 1000 tensor (column arm), the same
values as a contiguous 1000 x 8192 pair (row arm) and a training-loop batch of 1 x 8192, each
natively and with ``torcheval_amd.ops.DISABLE_HIP`` set (the ATen form on the same GPU and the same
tensors), the two alternating over several rounds, every window device-synchronised after a
warm-up.  ``MeanSquaredError.update`` on the same two tensors (the parents of the views) is the
yardstick: its kernel reads the same bytes once.  Kernel times come from a separate
``rocprofv3 --kernel-trace --stats`` run of this script with ``--profile-loop`` (tracing slows the
host, so wall times are taken with the profiler off); pass the resulting ``*_kernel_stats.csv`` with
``--kernel-stats`` to fold them in.

    python benchmarks/bench_pearson.py --out profiles/pearson_r12.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o pe -- python benchmarks/bench_pearson.py --profile-loop --shape 1000x8192xf32xcolumn
    python benchmarks/bench_pearson.py --fold RUN.json --kernel-stats 1000x8192xf32xcolumn=CSV --out profiles/pearson_r12.json
"""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.bench_spearman import HBM_PEAK, _alternate, _aten, _fold, _write  # noqa: E402
from torcheval_amd.metrics import MeanSquaredError, PearsonCorrCoef  # noqa: E402
from torcheval_amd.metrics.functional import pearson_corrcoef  # noqa: E402
from torcheval_amd.ops import corrcoef as k16  # noqa: E402

# tasks, n, dtype, layout
SHAPES = ((1, 1 << 20, "f32", "row"), (1, 1 << 20, "bf16", "row"), (1, 1 << 20, "bf16", "row_offset"),
          (8, 131072, "f32", "row"), (100, 10000, "f32", "row"), (1000, 8192, "f32", "column"),
          (1000, 8192, "f32", "row"), (1, 8192, "f32", "row"))
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _inputs(tasks: int, n: int, dtype: torch.dtype, layout: str, dev):
    """The operands as the metric takes them, and as ``MeanSquaredError`` does (contiguous)."""
    g = torch.Generator(device=dev).manual_seed(tasks + n)
    x = torch.randn(tasks, n, device=dev, generator=g) + 3.0
    y = 0.5 * x + torch.randn(tasks, n, device=dev, generator=g)
    x, y = x.to(dtype), y.to(dtype)
    if layout == "column":
        px, py = x.t().contiguous(), y.t().contiguous()  # [n, tasks] predictions, as a training loop holds them
        return (px.t(), py.t()), (px, py)
    if layout == "row_offset":  # the two heads differ: the second operand takes element loads
        buf = torch.zeros(tasks, n + 8, dtype=dtype, device=dev)
        buf[:, 1:n + 1] = y
        y = buf[:, 1:n + 1]
    if tasks == 1:
        return (x[0], y[0]), (x[0], y[0])
    return (x, y), (x, y)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", action="append", default=None, help="KEY=CSV, e.g. 1000x8192xf32xcolumn=stats.csv")
    ap.add_argument("--profile-loop", action="store_true", help="only run the native calls (under rocprofv3)")
    ap.add_argument("--shape", default=None, help="TASKSxNxDTYPExLAYOUT: only this shape")
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
    shapes = SHAPES
    if args.shape is not None:
        t, n, d, layout = args.shape.split("x")
        shapes = ((int(t), int(n), d, layout),)
    res = {"device": torch.cuda.get_device_name(0), "shapes": {}, "kernels": {}}
    for tasks, n, d, layout in shapes:
        (x, y), (mx, my) = _inputs(tasks, n, DTYPES[d], layout, dev)
        assert k16.supported(x, y) and k16.arm(x.reshape(tasks, -1) if x.dim() == 1 else x,
                                               y.reshape(tasks, -1) if y.dim() == 1 else y) == layout.split("_")[0]
        m = PearsonCorrCoef(num_tasks=tasks, device=dev)
        mse = MeanSquaredError(device=dev)

        def functional():
            return pearson_corrcoef(x, y, num_tasks=tasks)

        def update():
            return m.update(x, y)

        def yardstick():
            return mse.update(mx, my)

        if args.profile_loop:
            for _ in range(200):
                functional()
                update()
                yardstick()
            torch.cuda.synchronize()
            continue
        native, aten = functional(), _aten(functional)()
        big = tasks * n >= 1 << 20
        iters = {"native": 300, "aten": 30 if big else 60}
        bytes_read = 2 * tasks * n * x.element_size()
        res["shapes"][f"{tasks}x{n}x{d}x{layout}"] = {
            "native_vs_aten_max_abs_diff": float((native.double() - aten.double()).abs().max()),
            "pearson_corrcoef": _alternate({"native": functional, "aten": _aten(functional)}, iters, args.rounds),
            "PearsonCorrCoef.update": _alternate({"native": update, "aten": _aten(update)}, iters, args.rounds),
            "MeanSquaredError.update": _alternate({"native": yardstick}, {"native": 300}, args.rounds),
            "bytes_read": bytes_read,
            "pure_read_bound_us_at_hbm_peak": round(bytes_read / HBM_PEAK * 1e6, 2),
        }
    if args.profile_loop:
        return
    res["note"] = ("every shape's operands (at most 66 MB) fit the 256 MiB Infinity Cache, so repeated calls on the "
                   "same tensors read from it; the bound quoted is the HBM one")
    _fold(res, args.kernel_stats)
    _write(res, args.out)


if __name__ == "__main__":
    main()
