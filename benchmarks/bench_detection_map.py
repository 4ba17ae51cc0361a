"""K24 (detection mean average precision) on one MI355X: the fused match and curve kernels against
the ATen form.

Synthetic data at COCO-val scale: 5000 images, 100 detections and about 7 ground truths per image
(3 to 11), 80 classes, updates of 32 images; half of the detections are jittered copies of a ground
truth of their image, so the curves are not trivial.  Timed on the same GPU and the same tensors:

* ``update``: one ``MeanAveragePrecision.update_packed`` of 32 images (K24: one ``map_match`` launch
  and the small copy of the image offsets) against the ATen form of the same update, which is a
  Python loop over images, classes and kept detections and therefore runs at ``--aten-images``
  images (default 4); its time per image is what scales.
* ``compute``: ``compute()`` on the states of all 5000 images (the ATen plan: two stable sorts, a
  gather and a ``searchsorted``; then ``map_curve``'s two launches) against the ATen tables (a loop
  over the classes with ground truth).
* ``epoch``: all 157 updates and one ``compute()``, K24 only.

Every window is device-synchronised and follows a warm-up; the figures are medians over the rounds
with their minimum and maximum.

    python benchmarks/bench_detection_map.py --out profiles/detection_map_r20.json
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.bench_spearman import _alternate, _aten, _window, _write  # noqa: E402
from torcheval_amd.metrics import MeanAveragePrecision  # noqa: E402
from torcheval_amd.ops import detection as K  # noqa: E402

KEYS = ("map", "map_50", "map_75", "mar")


def data(images: int, detections: int, classes: int, dev, seed: int = 0):
    """Packed boxes of ``images`` images: ``detections`` detections each and 3 to 11 ground truths."""
    g = torch.Generator().manual_seed(seed)
    target_counts = torch.randint(3, 12, (images,), generator=g)
    n_gt = int(target_counts.sum())
    xy = torch.rand(n_gt, 2, generator=g) * 500
    tb = torch.cat([xy, xy + 20 + torch.rand(n_gt, 2, generator=g) * 120], dim=1)
    tl = torch.randint(0, classes, (n_gt,), generator=g)
    starts = torch.cumsum(target_counts, 0) - target_counts
    m = images * detections
    image = torch.arange(images).repeat_interleave(detections)
    pick = starts[image] + (torch.rand(m, generator=g) * target_counts[image]).long()
    copied = torch.rand(m, generator=g) < 0.5
    xy = torch.rand(m, 2, generator=g) * 500
    noise = torch.cat([xy, xy + 20 + torch.rand(m, 2, generator=g) * 120], dim=1)
    pb = torch.where(copied[:, None], tb[pick] + torch.randn(m, 4, generator=g) * 6, noise)
    pb[:, 2:] = torch.maximum(pb[:, 2:], pb[:, :2])
    pl = torch.where(copied, tl[pick], torch.randint(0, classes, (m,), generator=g))
    ps = torch.where(copied, 0.3 + 0.7 * torch.rand(m, generator=g), 0.6 * torch.rand(m, generator=g))
    return (pb.to(dev), ps.to(dev), pl.to(dev), [detections] * images, tb.to(dev), tl.to(dev), target_counts.tolist())


def batches(args, size: int):
    """The packed arguments cut into updates of ``size`` images."""
    pb, ps, pl, pc, tb, tl, tc = args
    out, d0, g0 = [], 0, 0
    for lo in range(0, len(pc), size):
        nd, ng = sum(pc[lo:lo + size]), sum(tc[lo:lo + size])
        out.append((pb[d0:d0 + nd], ps[d0:d0 + nd], pl[d0:d0 + nd], pc[lo:lo + size],
                    tb[g0:g0 + ng], tl[g0:g0 + ng], tc[lo:lo + size]))
        d0, g0 = d0 + nd, g0 + ng
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--detections", type=int, default=100)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--aten-images", type=int, default=4, help="images of the ATen form's update")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    packed = data(args.images, args.detections, args.classes, dev)
    updates = batches(packed, args.batch)
    small = batches(packed, args.aten_images)[0]
    res = {"device": torch.cuda.get_device_name(0), "images": args.images, "detections_per_image": args.detections,
           "ground_truths": len(packed[5]), "classes": args.classes, "images_per_update": args.batch,
           "max_boxes": K.max_boxes()}

    scratch = MeanAveragePrecision(args.classes, device=dev)

    def update(batch):
        def run():
            scratch.update_packed(*batch)
        return run

    res["update"] = _alternate({"native": update(updates[0])}, {"native": 200}, args.rounds)
    res["update_small"] = _alternate({"native": update(small)}, {"native": 200}, args.rounds)
    aten_update = _aten(update(small))
    aten_update()  # the ATen form's warm-up: one call
    windows = sorted(_window(aten_update, 1) for _ in range(args.rounds))
    res["update_small"]["images"] = args.aten_images
    res["update_small"]["aten_ms"] = round(windows[len(windows) // 2], 3)
    res["update_small"]["aten_ms_min_max"] = [round(windows[0], 3), round(windows[-1], 3)]
    # the two forms of the small update leave the same states, the scores bit for bit
    scratch.reset()
    update(small)()
    native_state = [t.clone() for t in (scratch.det_scores[0].view(torch.int32), scratch.det_labels[0],
                                        scratch.det_hits[0], scratch.gt_count)]
    scratch.reset()
    aten_update()
    res["update_small"]["states_equal"] = all(
        torch.equal(a, b) for a, b in zip(native_state, (scratch.det_scores[0].view(torch.int32),
                                                         scratch.det_labels[0], scratch.det_hits[0], scratch.gt_count)))
    scratch.reset()

    full = MeanAveragePrecision(args.classes, device=dev)

    def epoch():
        full.reset()
        for batch in updates:
            full.update_packed(*batch)
        return full.compute()

    res["epoch"] = _alternate({"native": epoch}, {"native": 3}, args.rounds)
    res["epoch"]["updates"] = len(updates)
    value = epoch()
    res["compute"] = _alternate({"native": full.compute}, {"native": 50}, args.rounds)
    aten_compute = _aten(full.compute)
    reference = aten_compute()
    windows = sorted(_window(aten_compute, 3) for _ in range(args.rounds))
    res["compute"]["aten_ms"] = round(windows[len(windows) // 2], 3)
    res["compute"]["aten_ms_min_max"] = [round(windows[0], 3), round(windows[-1], 3)]
    res["values"] = {k: float(value[k]) for k in KEYS}
    res["values_aten_tables"] = {k: float(reference[k]) for k in KEYS}
    res["note"] = ("native: K24 (update: map_match, one launch; compute: the ATen plan of two stable sorts, a gather "
                   "and a searchsorted, then map_curve's two launches); aten: the same calls with the native route "
                   "off on the same tensors (update: the definition in a loop over images, classes and kept "
                   "detections, at update_small's image count; compute: a loop over the classes with ground truth); "
                   "the update windows append to one metric (12 bytes per detection); medians of the rounds' windows "
                   "with their minimum and maximum")
    _write(res, args.out)


if __name__ == "__main__":
    main()
