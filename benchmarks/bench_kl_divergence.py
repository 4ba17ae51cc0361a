"""K18 (KL divergence) on one MI355X: the native path against this package's ATen form.

Times ``kl_divergence`` (``"mean"``) and ``KLDivergence.update`` at 4096 x 32000 f32, 4096 x 50257
f32, 2048 x 128256 bf16, 8192 x 1000 f32 and 1M x 10 f32 (the narrow shape: only the wave arm
exists, not tuned), for logits and for weights, each natively and with
``torcheval_amd.ops.DISABLE_HIP`` set (the ATen form on the same GPU and the same tensors), the two
alternating over several rounds, every window device-synchronised after a warm-up.  Two yardsticks
are not the code under test: ``perplexity`` (K7) on ``input`` alone, which walks half the bytes the
same way, and the pure-read time of both operands at the HBM peak.  Kernel times come from a
separate ``rocprofv3 --kernel-trace --stats`` run of this script with ``--profile-loop`` (tracing
slows the host, so wall times are taken with the profiler off); pass the resulting
``*_kernel_stats.csv`` with ``--kernel-stats`` to fold them in.

    python benchmarks/bench_kl_divergence.py --out profiles/kl_divergence_r14.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kl -- python benchmarks/bench_kl_divergence.py --profile-loop --shape 4096x32000xf32
    python benchmarks/bench_kl_divergence.py --fold RUN.json --kernel-stats 4096x32000xf32=CSV --out profiles/kl_divergence_r14.json
"""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.bench_spearman import HBM_PEAK, _alternate, _aten, _fold, _window, _write  # noqa: E402
from torcheval_amd.metrics import KLDivergence  # noqa: E402
from torcheval_amd.metrics.functional import kl_divergence, perplexity  # noqa: E402

SHAPES = ((4096, 32000, "f32"), (4096, 50257, "f32"), (2048, 128256, "bf16"), (8192, 1000, "f32"), (1 << 20, 10, "f32"))
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _inputs(n: int, c: int, dtype: torch.dtype, logits: bool, dev):
    g = torch.Generator(device=dev).manual_seed(n + c)
    x = torch.randn(n, c, device=dev, generator=g) * 3
    t = x + torch.randn(n, c, device=dev, generator=g)
    if not logits:
        x, t = torch.softmax(x, dim=1), torch.softmax(t, dim=1)
    labels = torch.randint(0, c, (n,), device=dev, generator=g)
    return x.to(dtype), t.to(dtype), labels


def _iters(fn, most: int) -> int:
    """Calls per window: about a quarter of a second of work, ``most`` at the most, 3 at the least."""
    fn()
    return max(3, min(most, int(250.0 / max(_window(fn, 1), 1e-3))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", action="append", default=None, help="KEY=CSV, e.g. 4096x32000xf32=stats.csv")
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
    res = {"device": torch.cuda.get_device_name(0), "reduction": "mean", "shapes": {}, "kernels": {}}
    for n, c, d in shapes:
        for logits in (True, False):
            x, t, labels = _inputs(n, c, DTYPES[d], logits, dev)
            m = KLDivergence(from_logits=logits, device=dev)

            def functional():
                return kl_divergence(x, t, from_logits=logits)

            def update():
                return m.update(x, t)

            def ppl():
                return perplexity(x[None], labels[None])

            if args.profile_loop:
                for _ in range(20):
                    functional()
                    update()
                    ppl()
                torch.cuda.synchronize()
                continue
            native, aten = functional(), _aten(functional)()
            iters = {"native": _iters(functional, 300), "aten": _iters(_aten(functional), 50)}
            one = {"native": iters["native"]}
            print(f"{n}x{c}x{d} logits={logits}: {iters} calls per window", file=sys.stderr, flush=True)
            bytes_read = 2 * x.numel() * x.element_size()
            res["shapes"][f"{n}x{c}x{d} " + ("logits" if logits else "weights")] = {
                "native_vs_aten_abs_diff": abs(float(native) - float(aten)),
                "kl_divergence": _alternate({"native": functional, "aten": _aten(functional)}, iters, args.rounds),
                "KLDivergence.update": _alternate({"native": update, "aten": _aten(update)}, iters, args.rounds),
                "perplexity_of_input_alone": _alternate({"native": ppl}, one, args.rounds),
                "calls_per_window": iters,
                "bytes_read": bytes_read,
                "pure_read_bound_us_at_hbm_peak": round(bytes_read / HBM_PEAK * 1e6, 2),
            }
            del x, t, labels, m
            torch.cuda.empty_cache()
    if args.profile_loop:
        return
    res["how"] = (
        "Wall times: ms per call over a window of calls_per_window back-to-back calls that ends in a device "
        "synchronise, after 5 warm-up calls per variant; native and ATen windows alternate over 5 rounds; the median "
        "and the [min, max] over the rounds are kept.  Repeated calls read the same tensors: 8192 x 1000 (66 MB for "
        "both operands) and 1M x 10 (84 MB) fit the 256 MiB Infinity Cache and are served from it, the three wide "
        "shapes (1.0-1.6 GB) are not.  The bound quoted is bytes_read at the 8 TB/s HBM peak.  Kernel times: a separate "
        "rocprofv3 --kernel-trace --stats run (no counters) of --profile-loop per shape, 20 calls of each entry point "
        "per mode.")
    _fold(res, args.kernel_stats)
    _write(res, args.out)


if __name__ == "__main__":
    main()
