"""K19 (Kendall rank correlation) on one MI355X: the native path against this package's ATen form
and against ``spearman_corrcoef`` (K14), which pays for the same two sorts.

Times ``kendall_rank_corrcoef`` and ``KendallRankCorrCoef.compute`` at 1 x 1M, 8 x 131072 and
100 x 10000, float32, continuous and with 50-level ties, each natively and with
``torcheval_amd.ops.DISABLE_HIP`` set (the ATen form on the same GPU and the same tensors), and
``spearman_corrcoef`` on the same tensors, the three alternating over several rounds, every window
device-synchronised after a warm-up.  Kernel times come from a separate
``rocprofv3 --kernel-trace --stats`` run of this script with ``--profile-loop`` (tracing slows the
host, so wall times are taken with the profiler off); pass the resulting ``*_kernel_stats.csv`` with
``--kernel-stats`` to fold them in.

    python benchmarks/bench_kendall.py --out profiles/kendall_r15.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kd -- python benchmarks/bench_kendall.py --profile-loop --shape 1x1048576
    python benchmarks/bench_kendall.py --fold RUN.json --kernel-stats 1x1048576=CSV --out profiles/kendall_r15.json
"""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.bench_spearman import LEVELS, SHAPES, _alternate, _aten, _fold, _inputs, _write  # noqa: E402
from torcheval_amd.metrics import KendallRankCorrCoef  # noqa: E402
from torcheval_amd.metrics.functional import kendall_rank_corrcoef, spearman_corrcoef  # noqa: E402
from torcheval_amd.metrics.functional.regression.kendall import _kendall_counts  # noqa: E402
from torcheval_amd.ops import kendall as K  # noqa: E402


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
    res = {"device": torch.cuda.get_device_name(0), "dtype": "float32", "tile": K.TILE, "shapes": {}, "kernels": {}}
    for rows, n in shapes:
        for levels in LEVELS:
            x, y = _inputs(rows, n, levels, dev)
            tasks = rows
            m = KendallRankCorrCoef(num_tasks=tasks, device=dev).update(x, y)

            def functional():
                return kendall_rank_corrcoef(x, y, num_tasks=tasks)

            def spearman():
                return spearman_corrcoef(x, y, num_tasks=tasks)

            if args.profile_loop:
                if levels is None:
                    for _ in range(200):
                        functional()
                    torch.cuda.synchronize()
                continue
            native, aten = functional(), _aten(functional)()
            same = torch.equal(_kendall_counts(x, y), _aten(lambda: _kendall_counts(x, y))())
            big = rows * n >= 1 << 20
            iters = {"native": 200, "aten": 10 if big else 20, "spearman": 200}
            res["shapes"][f"{rows}x{n}" + ("" if levels is None else f" ties{levels}")] = {
                "native_vs_aten_max_abs_diff": float((native.double() - aten.double()).abs().max()),
                "native_counts_equal_aten_counts": same,
                "kendall_rank_corrcoef": _alternate(
                    {"native": functional, "aten": _aten(functional), "spearman": spearman}, iters, args.rounds),
                "KendallRankCorrCoef.compute": _alternate({"native": m.compute, "aten": _aten(m.compute)}, iters,
                                                          args.rounds),
            }
    if args.profile_loop:
        return
    res["note"] = ("spearman = spearman_corrcoef (K3a + K14) on the same tensors: it sorts the same 2 rows x n keys, "
                   "in one stacked K3a call where K19 needs two dependent ones; every shape's operands (8 MB) fit "
                   "the 256 MiB Infinity Cache, so repeated calls on the same tensors read from it")
    _fold(res, args.kernel_stats)
    _write(res, args.out)


if __name__ == "__main__":
    main()
