"""K17 (segmentation mean IoU / Dice) on one MI355X: the native path against this package's ATen form.

Times ``mean_iou`` and ``MeanIoU.update`` at 8x19x1024x2048 f32 and bf16 (Cityscapes), 16x150x512x512
f32 (ADE20K), 32x21x512x512 f32 (VOC), the Cityscapes shape in ``channels_last`` (the element arm)
and a 16x512x512 pair of label maps, each with and without ``ignore_index=255``, natively and with
``torcheval_amd.ops.DISABLE_HIP`` set (the ATen form on the same GPU and the same tensors), the two
alternating over several rounds, every window device-synchronised after a warm-up.  Next to every
time stands the operands' pure-read time at the HBM peak.  The label maps are blocky (32 x 32
blocks of one label, a twentieth of them void) and the scores favour the label, wrongly in a tenth
of the blocks, as a trained network's do: neighbouring pixels mostly share a (target, prediction)
pair.  Kernel times come from a separate ``rocprofv3 --kernel-trace --stats`` run of this script
with ``--profile-loop`` (tracing slows the host, so wall times are taken with the profiler off);
pass the resulting ``*_kernel_stats.csv`` with ``--kernel-stats`` to fold them in.

    python benchmarks/bench_segmentation.py --out profiles/segmentation_r13.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o seg -- python benchmarks/bench_segmentation.py --profile-loop --shape 8x19x1024x2048xf32
    python benchmarks/bench_segmentation.py --fold RUN.json --kernel-stats 8x19x1024x2048xf32=CSV --out profiles/segmentation_r13.json
"""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.bench_spearman import HBM_PEAK, _alternate, _aten, _fold, _window, _write  # noqa: E402
from torcheval_amd.metrics import MeanIoU  # noqa: E402
from torcheval_amd.metrics.functional import mean_iou  # noqa: E402
from torcheval_amd.ops import segmentation as K  # noqa: E402

# (N, C, H, W, dtype, layout); C == 0: a pair of label maps
SHAPES = ((8, 19, 1024, 2048, "f32", "nchw"), (8, 19, 1024, 2048, "bf16", "nchw"), (16, 150, 512, 512, "f32", "nchw"),
          (32, 21, 512, 512, "f32", "nchw"), (8, 19, 1024, 2048, "f32", "nhwc"), (16, 0, 512, 512, "i64", "labels"))
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
BLOCK = 32
VOID = 255


def _key(n, c, h, w, d, layout) -> str:
    return f"{n}x{c}x{h}x{w}x{d}" + ("" if layout == "nchw" else "x" + layout)


def _inputs(n: int, c: int, h: int, w: int, d: str, layout: str, dev):
    """(input, target, target with void blocks) on ``dev``."""
    g = torch.Generator(device=dev).manual_seed(n + c + h)
    classes = c if c else 19
    coarse = torch.randint(0, classes, (n, h // BLOCK, w // BLOCK), device=dev, generator=g)
    wrong = torch.rand(coarse.shape, device=dev, generator=g) < 0.1
    favoured = torch.where(wrong, torch.randint(0, classes, coarse.shape, device=dev, generator=g), coarse)
    void = torch.where(torch.rand(coarse.shape, device=dev, generator=g) < 0.05, VOID, coarse)

    def fine(v):
        return v.repeat_interleave(BLOCK, 1).repeat_interleave(BLOCK, 2).contiguous()

    target, target_void, favoured = fine(coarse), fine(void), fine(favoured)
    if c == 0:
        return favoured, target, target_void
    x = torch.randn(n, c, h, w, device=dev, generator=g)
    x.scatter_add_(1, favoured[:, None], torch.full((n, 1, h, w), 6.0, device=dev))
    x = x.to(DTYPES[d])
    if layout == "nhwc":
        x = x.contiguous(memory_format=torch.channels_last)
    return x, target, target_void


def _iters(fn, most: int, least: int) -> int:
    """Calls per window: about a quarter of a second of work, between ``least`` and ``most``."""
    fn()
    return max(least, min(most, int(250.0 / max(_window(fn, 1), 1e-3))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", action="append", default=None, help="KEY=CSV, e.g. 8x19x1024x2048xf32=stats.csv")
    ap.add_argument("--profile-loop", action="store_true", help="only run the native calls (under rocprofv3)")
    ap.add_argument("--shape", default=None, help="a key of the result, e.g. 8x19x1024x2048xf32xnhwc: only this shape")
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
    shapes = [s for s in SHAPES if args.shape is None or _key(*s) == args.shape]
    res = {"device": torch.cuda.get_device_name(0), "average": "macro", "span": K.SPAN, "max_blocks": K.max_blocks(),
           "shapes": {}, "kernels": {}}
    for shape in shapes:
        n, c, h, w, d, layout = shape
        x, target, target_void = _inputs(*shape, dev)
        classes = c if c else 19
        for ignore, t in ((None, target), (VOID, target_void)):
            m = MeanIoU(num_classes=classes, ignore_index=ignore, device=dev)

            def functional():
                return mean_iou(x, t, num_classes=classes, ignore_index=ignore)

            def update():
                return m.update(x, t)

            if args.profile_loop:
                for _ in range(30):
                    functional()
                    update()
                torch.cuda.synchronize()
                continue
            native, aten = functional(), _aten(functional)()
            iters = {"native": _iters(functional, 300, 3), "aten": _iters(_aten(functional), 50, 2)}
            print(f"{_key(*shape)} ignore_index={ignore}: {iters} calls per window", file=sys.stderr, flush=True)
            bytes_read = x.numel() * x.element_size() + t.numel() * t.element_size()
            res["shapes"][f"{_key(*shape)} ignore_index={ignore}"] = {
                "arm": K.arm(x),
                "value": float(native),
                "native_vs_aten_abs_diff": abs(float(native) - float(aten)),
                "mean_iou": _alternate({"native": functional, "aten": _aten(functional)}, iters, args.rounds),
                "MeanIoU.update": _alternate({"native": update, "aten": _aten(update)}, iters, args.rounds),
                "calls_per_window": iters,
                "bytes_read": bytes_read,
                "pure_read_bound_us_at_hbm_peak": round(bytes_read / HBM_PEAK * 1e6, 2),
            }
            del m
        del x, target, target_void
        torch.cuda.empty_cache()
    if args.profile_loop:
        return
    res["note"] = ("every scores shape is larger than the 256 MiB Infinity Cache; the 16x512x512 label maps (2 x 34 MB) "
                   "fit it, so repeated calls on them read from it.  The bound quoted is the HBM one")
    _fold(res, args.kernel_stats)
    _write(res, args.out)


if __name__ == "__main__":
    main()
