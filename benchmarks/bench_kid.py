"""K20 (Kernel Inception Distance) on one MI355X: the fused Gram kernel against the unfused forms.

Times ``kernel_inception_distance`` and ``KernelInceptionDistance.compute`` (index draws included)
and, on one fixed pair of index tensors per shape, the two K20 launches alone against three
yardsticks on the same GPU and the same tensors:

1. this package's ATen form in float32 (batched gather, ``bmm``, power, sums: what torchmetrics runs),
2. the same form in float64 (the library's fallback and the tests' reference),
3. ``torch.bmm`` alone on pre-gathered ``[S, m, D]`` float32 operands for the three Gram blocks, the
   library-GEMM floor of any unfused form (it writes the Gram matrices and does nothing with them).

The variants' windows alternate over several rounds, each device-synchronised after a warm-up.
Kernel times come from a separate ``rocprofv3 --kernel-trace --stats`` run of this script with
``--profile-loop`` (tracing slows the host, so wall times are taken with the profiler off); pass the
resulting ``*_kernel_stats.csv`` with ``--kernel-stats`` to fold them in.

    python benchmarks/bench_kid.py --out profiles/kid_r16.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kid -- python benchmarks/bench_kid.py --profile-loop --shape 10000x2048
    python benchmarks/bench_kid.py --fold RUN.json --kernel-stats 10000x2048=CSV --out profiles/kid_r16.json
"""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.bench_spearman import _alternate, _aten, _fold, _write  # noqa: E402
from torcheval_amd.metrics import KernelInceptionDistance  # noqa: E402
from torcheval_amd.metrics.functional import kernel_inception_distance  # noqa: E402
from torcheval_amd.metrics.functional.image.kid import _draw, _kid_sums_aten, _mmd2  # noqa: E402
from torcheval_amd.ops import kid as K  # noqa: E402

# key: (rows per side, D, subsets, subset_size)
SHAPES = {
    "10000x2048": (10000, 2048, 100, 1000),
    "50000x2048": (50000, 2048, 100, 1000),
    "10000x64": (10000, 64, 100, 1000),
    "2000x2048 S10 m100": (2000, 2048, 10, 100),
}


def _mfma_flops(d: int, subsets: int, m: int) -> int:
    """Flops the Gram kernel runs: whole 128 x 128 tiles, K rounded up to its step of 32; the
    symmetric blocks count their upper-triangle tiles only."""
    return subsets * K.items(m) * 2 * K.TILE * K.TILE * (-(-d // 32) * 32)


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
        _fold(res, args.kernel_stats)
        for key, k in res["kernels"].items():
            gram = next((v for n, v in k.items() if "kid_gram_kernel" in n), None)
            if gram is not None and key in res["shapes"]:
                res["shapes"][key]["kid_gram_kernel_tflops"] = round(
                    res["shapes"][key]["mfma_flops"] / (gram["average_us"] * 1e-6) / 1e12, 1)
        _write(res, args.out)
        return
    dev = torch.device("cuda", 0)
    keys = list(SHAPES) if args.shape is None else [args.shape]
    res = {"device": torch.cuda.get_device_name(0), "dtype": "float32", "tile": K.TILE, "shapes": {}, "kernels": {}}
    for key in keys:
        n, d, subsets, m = SHAPES[key]
        g = torch.Generator(device=dev).manual_seed(n + d)
        real = torch.rand(n, d, device=dev, generator=g)
        fake = 0.8 * torch.rand(n, d, device=dev, generator=g) + 0.3
        idx_r, idx_f = _draw(subsets, n, m, dev, g), _draw(subsets, n, m, dev, g)
        gamma = 1.0 / d

        def core():
            return K.kid(real, fake, idx_r, idx_f, 3, gamma, 1.0)[1]

        if args.profile_loop:
            for _ in range(20):
                core()
            torch.cuda.synchronize()
            continue

        def aten(dtype):
            return lambda: _mmd2(_kid_sums_aten(real, fake, idx_r, idx_f, 3, gamma, 1.0, dtype), m)

        gx, gy = real[idx_r.long()], fake[idx_f.long()]  # the bmm floor's operands, gathered once

        def bmm_only():
            return (torch.bmm(gx, gx.transpose(1, 2)), torch.bmm(gy, gy.transpose(1, 2)),
                    torch.bmm(gx, gy.transpose(1, 2)))

        metric = KernelInceptionDistance(model=torch.nn.Identity(), feature_dim=d, subsets=subsets, subset_size=m,
                                         seed=0, device=dev)
        metric.update_activations(real, True).update_activations(fake, False)

        def functional():
            return kernel_inception_distance(real, fake, subsets=subsets, subset_size=m)

        native = core()
        f32, f64 = aten(torch.float32)(), aten(torch.float64)()
        iters = {"native": 20, "aten_f32": 3, "aten_f64": 3, "bmm_only_f32": 5}
        api_iters = {"native": 10, "aten": 2}
        res["shapes"][key] = {
            "subsets": subsets, "subset_size": m, "tiles_per_subset": K.items(m),
            "mfma_flops": _mfma_flops(d, subsets, m),
            "mean_mmd2": float(f64.mean()),
            "native_vs_aten_f64_max_abs_diff": float((native - f64).abs().max()),
            "aten_f32_vs_aten_f64_max_abs_diff": float((f32.double() - f64).abs().max()),
            "two_launches_on_fixed_indices": _alternate(
                {"native": core, "aten_f32": aten(torch.float32), "aten_f64": aten(torch.float64),
                 "bmm_only_f32": bmm_only}, iters, args.rounds),
            "kernel_inception_distance": _alternate({"native": functional, "aten": _aten(functional)}, api_iters,
                                                    args.rounds),
            "KernelInceptionDistance.compute": _alternate({"native": metric.compute, "aten": _aten(metric.compute)},
                                                          api_iters, args.rounds),
        }
        del gx, gy, metric
    if args.profile_loop:
        return
    res["note"] = ("aten_f32 / aten_f64: _kid_sums_aten (gather, bmm, power, zeroed diagonal, sums) in that dtype on "
                   "the same index tensors; bmm_only_f32: three torch.bmm on operands gathered once outside the "
                   "window; the API rows include the index draws (torch.rand + topk per side) and, for aten, run "
                   "the float64 form")
    _fold(res, args.kernel_stats)
    _write(res, args.out)


if __name__ == "__main__":
    main()
