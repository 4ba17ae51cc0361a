"""K21 (Inception Score) on one MI355X: the native path against this package's ATen form.

Times ``inception_score`` and ``InceptionScore.update_logits`` + ``compute`` at 50000 x 1000 f32 (the
standard IS-50k), 50000 x 1008 f32, 8192 x 1000 f32, 10000 x 1000 bf16 and 65536 x 10 f32 (the narrow
shape, not tuned), each natively and with ``torcheval_amd.ops.DISABLE_HIP`` set (the ATen form on
the same GPU and the same tensor), the two alternating over several rounds, every window
device-synchronised after a warm-up.  Two yardsticks are not the code under test: ``perplexity``
(K7) and ``multiclass_calibration_error`` with ``from_logits=True`` (K15's logits arm) on the same
tensor, which read the same bytes once with an online log-sum-exp; and the pure-read time of the
logits at the HBM peak.  Kernel times come from a separate ``rocprofv3 --kernel-trace --stats`` run
of this script with ``--profile-loop`` (tracing slows the host, so wall times are taken with the
profiler off); pass the resulting ``*_kernel_stats.csv`` with ``--kernel-stats`` to fold them in.

    python benchmarks/bench_inception_score.py --out profiles/inception_score_r17.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o is -- python benchmarks/bench_inception_score.py --profile-loop --shape 50000x1000xf32
    python benchmarks/bench_inception_score.py --fold RUN.json --kernel-stats 50000x1000xf32=CSV --out profiles/inception_score_r17.json
"""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.bench_kl_divergence import DTYPES, _iters  # noqa: E402
from benchmarks.bench_spearman import HBM_PEAK, _alternate, _aten, _fold, _write  # noqa: E402
from torcheval_amd.metrics import InceptionScore  # noqa: E402
from torcheval_amd.metrics.functional import inception_score, multiclass_calibration_error, perplexity  # noqa: E402

SHAPES = ((50000, 1000, "f32"), (50000, 1008, "f32"), (8192, 1000, "f32"), (10000, 1000, "bf16"), (65536, 10, "f32"))


def _inputs(n: int, c: int, dtype: torch.dtype, dev):
    g = torch.Generator(device=dev).manual_seed(n + c)
    x = (torch.randn(n, c, device=dev, generator=g) * 3).to(dtype)
    return x, torch.randint(0, c, (n,), device=dev, generator=g)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", action="append", default=None, help="KEY=CSV, e.g. 50000x1000xf32=stats.csv")
    ap.add_argument("--profile-loop", action="store_true", help="only run the native calls (under rocprofv3)")
    ap.add_argument("--shape", default=None, help="NxCxDTYPE: only this shape")
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
        n, c, d = args.shape.split("x")
        shapes = ((int(n), int(c), d),)
    res = {"device": torch.cuda.get_device_name(0), "splits": 10, "shapes": {}, "kernels": {}}
    for n, c, d in shapes:
        x, labels = _inputs(n, c, DTYPES[d], dev)
        m = InceptionScore(model=torch.nn.Identity(), num_classes=c, device=dev)

        def functional():
            return inception_score(x)

        def update_compute():
            return m.update_logits(x).compute()

        def ppl():
            return perplexity(x[None], labels[None])

        def ece():
            return multiclass_calibration_error(x, labels, from_logits=True)

        if args.profile_loop:
            for _ in range(20):
                functional()
                update_compute()
                ppl()
                ece()
            torch.cuda.synchronize()
            continue
        native, aten = functional(), _aten(functional)()
        iters = {"native": _iters(functional, 300), "aten": _iters(_aten(functional), 50)}
        one = {"native": iters["native"]}
        print(f"{n}x{c}x{d}: {iters} calls per window", file=sys.stderr, flush=True)
        bytes_read = x.numel() * x.element_size()
        res["shapes"][f"{n}x{c}x{d}"] = {
            "native": [float(v) for v in native],
            "native_vs_aten_abs_diff": [abs(float(p) - float(q)) for p, q in zip(native, aten)],
            "inception_score": _alternate({"native": functional, "aten": _aten(functional)}, iters, args.rounds),
            "InceptionScore.update_logits+compute": _alternate(
                {"native": update_compute, "aten": _aten(update_compute)}, iters, args.rounds),
            "perplexity_on_the_same_tensor": _alternate({"native": ppl}, one, args.rounds),
            "calibration_error_logits_on_the_same_tensor": _alternate({"native": ece}, one, args.rounds),
            "calls_per_window": iters,
            "bytes_read": bytes_read,
            "pure_read_bound_us_at_hbm_peak": round(bytes_read / HBM_PEAK * 1e6, 2),
        }
        del x, labels, m
        torch.cuda.empty_cache()
    if args.profile_loop:
        return
    res["how"] = (
        "Wall times: ms per call over a window of calls_per_window back-to-back calls that ends in a device "
        "synchronise, after 5 warm-up calls per variant; native and ATen windows alternate over 5 rounds; the median "
        "and the [min, max] over the rounds are kept.  Repeated calls read the same tensor: 50000 x 1000 f32 is 200 MB "
        "and fits the 256 MiB Infinity Cache, as do the smaller shapes, so repeated reads are served from it and not "
        "from HBM.  The bound quoted is bytes_read at the 8 TB/s HBM peak.  Kernel times: a separate rocprofv3 "
        "--kernel-trace --stats run (no counters) of --profile-loop per shape, 20 calls of each entry point.")
    _fold(res, args.kernel_stats)
    _write(res, args.out)


if __name__ == "__main__":
    main()
