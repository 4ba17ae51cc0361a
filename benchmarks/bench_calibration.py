"""K15 (multiclass calibration error) on one MI355X: the native path against this package's ATen form.

Times ``multiclass_calibration_error`` and ``MulticlassCalibrationError.update`` at 8192 x 1000 f32,
4096 x 32000 f32, 2048 x 128256 bf16 and 1M x 10 f32, for probabilities and for logits, each
natively and with ``torcheval_amd.ops.DISABLE_HIP`` set (the ATen form on the same GPU and the same
tensors), the two alternating over several rounds, every window device-synchronised after a
warm-up.  ``MulticlassAccuracy.update`` (K1) and ``perplexity`` (K7) on the same tensors are the
yardsticks: the wave-per-row kernel does the argmax of the one and the sum of the other over the
same bytes.  Kernel times come from a separate ``rocprofv3 --kernel-trace --stats`` run of this
script with ``--profile-loop`` (tracing slows the host, so wall times are taken with the profiler
off); pass the resulting ``*_kernel_stats.csv`` with ``--kernel-stats`` to fold them in.

    python benchmarks/bench_calibration.py --out profiles/calibration_r11.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o cal -- python benchmarks/bench_calibration.py --profile-loop --shape 8192x1000xf32
    python benchmarks/bench_calibration.py --fold RUN.json --kernel-stats 8192x1000xf32=CSV --out profiles/calibration_r11.json
"""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.bench_spearman import HBM_PEAK, _alternate, _aten, _fold, _window, _write  # noqa: E402
from torcheval_amd.metrics import MulticlassAccuracy, MulticlassCalibrationError  # noqa: E402
from torcheval_amd.metrics.functional import multiclass_calibration_error, perplexity  # noqa: E402

SHAPES = ((8192, 1000, "f32"), (4096, 32000, "f32"), (2048, 128256, "bf16"), (1 << 20, 10, "f32"))
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _inputs(n: int, c: int, dtype: torch.dtype, logits: bool, dev):
    g = torch.Generator(device=dev).manual_seed(n + c)
    x = torch.randn(n, c, device=dev, generator=g) * 3
    if not logits:
        x = torch.softmax(x, dim=1)
    x = x.to(dtype)
    t = torch.where(torch.rand(n, device=dev, generator=g) < 0.5, x.argmax(1),
                    torch.randint(0, c, (n,), device=dev, generator=g))
    return x, t


def _iters(fn, most: int) -> int:
    """Calls per window: about a quarter of a second of work, ``most`` at the most, 3 at the least.
    The ATen form's three ``scatter_add``s of a million float64 values into 15 bins contend on 15
    addresses and take orders of magnitude longer than anything else here."""
    fn()
    return max(3, min(most, int(250.0 / max(_window(fn, 1), 1e-3))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", action="append", default=None, help="KEY=CSV, e.g. 8192x1000xf32=stats.csv")
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
    res = {"device": torch.cuda.get_device_name(0), "n_bins": 15, "norm": "l1", "shapes": {}, "kernels": {}}
    for n, c, d in shapes:
        for logits in (False, True):
            x, t = _inputs(n, c, DTYPES[d], logits, dev)
            m = MulticlassCalibrationError(from_logits=logits, device=dev)
            acc = MulticlassAccuracy(device=dev)

            def functional():
                return multiclass_calibration_error(x, t, from_logits=logits)

            def update():
                return m.update(x, t)

            if args.profile_loop:
                for _ in range(100):
                    functional()
                    update()
                    acc.update(x, t)
                    perplexity(x[None], t[None])
                torch.cuda.synchronize()
                continue
            native, aten = functional(), _aten(functional)()
            iters = {"native": _iters(functional, 300), "aten": _iters(_aten(functional), 50)}
            one = {"native": iters["native"]}
            print(f"{n}x{c}x{d} logits={logits}: {iters} calls per window", file=sys.stderr, flush=True)
            bytes_read = x.numel() * x.element_size() + t.numel() * t.element_size()
            res["shapes"][f"{n}x{c}x{d} " + ("logits" if logits else "probabilities")] = {
                "native_vs_aten_abs_diff": abs(float(native) - float(aten)),
                "multiclass_calibration_error": _alternate({"native": functional, "aten": _aten(functional)}, iters,
                                                           args.rounds),
                "MulticlassCalibrationError.update": _alternate({"native": update, "aten": _aten(update)}, iters,
                                                                args.rounds),
                "MulticlassAccuracy.update": _alternate({"native": lambda: acc.update(x, t)}, one, args.rounds),
                "perplexity": _alternate({"native": lambda: perplexity(x[None], t[None])}, one, args.rounds),
                "calls_per_window": iters,
                "bytes_read": bytes_read,
                "pure_read_bound_us_at_hbm_peak": round(bytes_read / HBM_PEAK * 1e6, 2),
            }
            del x, t, m, acc
            torch.cuda.empty_cache()
    if args.profile_loop:
        return
    res["note"] = ("8192 x 1000 (33 MB) and 1M x 10 (40 MB) fit the 256 MiB Infinity Cache, so repeated calls on the "
                   "same tensors read from it; the two 525 MB shapes do not.  The bound quoted is the HBM one")
    _fold(res, args.kernel_stats)
    _write(res, args.out)


if __name__ == "__main__":
    main()
