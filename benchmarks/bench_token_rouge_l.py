"""K30 (token LCS length / ROUGE-L) on one MI355X: the native kernels against this package's ATen form on
the same GPU, against a host copy with the Python table, and, for orientation, against K29
(``TokenErrorRate``: the same table size, walked systolically) on the same rows.

Four shapes, about 10 % substitutions, insertions and deletions between prediction and target, int64 and
int32 ids: 4096 pairs with target lengths uniform in 10..60, 1024 pairs of 256 target tokens, 256 of 512 and
32 of 2048 (one wave per pair leaves the device underfilled there; the shape is recorded, not served by an
arm of its own).  It times one ``TokenROUGEL.update()`` natively and with ``torcheval_amd.ops.DISABLE_HIP``
set (the ATen form on the same GPU and tensors) and one native ``TokenErrorRate.update()``, alternating over
several rounds, every window device-synchronised after a warm-up.  The host route is a device-to-host copy
of ids and lengths plus the two-row table on Python lists; the table is timed on the first ``host_pairs``
pairs (about 2^21 cells) and scaled to the batch, and the JSON says so.

    python benchmarks/bench_token_rouge_l.py --out RUN.json
"""

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torcheval_amd.ops as ops  # noqa: E402
from benchmarks.bench_token_edit_distance import _pairs, _tensors, _window  # noqa: E402
from torcheval_amd.metrics import TokenErrorRate, TokenROUGEL  # noqa: E402
from torcheval_amd.metrics.functional import token_lcs_length  # noqa: E402
from torcheval_amd.ops import edit_distance as K29  # noqa: E402
from torcheval_amd.ops import lcs as K  # noqa: E402

SHAPES = ((4096, 10, 60), (1024, 256, 256), (256, 512, 512), (32, 2048, 2048))  # pairs, target lengths from .. to
HOST_CELLS = 2**21
METHOD = ("wall: windows of back-to-back calls ending in a device synchronise, the sides of a comparison alternating "
          "over the rounds, medians and min/max; host route: copy of the whole batch plus the Python table on "
          "host_pairs pairs, the table's time scaled by pairs / host_pairs")


def _table(a, b):
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b, 1):
            cur.append(prev[j - 1] + 1 if x == y else max(prev[j], cur[j - 1]))
        prev = cur
    return prev[-1]


def _shape(pairs: int, lo: int, hi: int, dtype, rounds: int) -> dict:
    dev = torch.device("cuda", 0)
    hyps, refs = _pairs(pairs, lo, hi, seed=pairs)
    (x, xl), (t, tl) = _tensors(hyps, dtype, dev), _tensors(refs, dtype, dev)
    assert K.supported(x, t)
    native = token_lcs_length(x, t, xl, tl)
    ops.DISABLE_HIP = True
    aten = token_lcs_length(x, t, xl, tl)
    ops.DISABLE_HIP = False
    host_pairs = max(1, min(pairs, HOST_CELLS // (hi * hi)))
    res = {"pairs": pairs, "target_lengths": [lo, hi], "dtype": str(dtype), "widths": [x.shape[1], t.shape[1]],
           "chunks": K.pick_chunks(x.shape[1], t.shape[1]), "lcs_sum": int(native.sum()),
           "lengths_equal_aten": bool(torch.equal(native, aten)),
           "lengths_equal_table": native[:host_pairs].tolist() == [_table(a, b) for a, b in zip(hyps[:host_pairs], refs[:host_pairs])],
           "k29_arm": ("wave", "block")[K29.pick_arm(pairs, x.shape[1], t.shape[1])], "host_pairs": host_pairs}
    rouge, ter = TokenROUGEL(device=dev), TokenErrorRate(device=dev)
    sides = {"native": (False, lambda: rouge.update(x, t, xl, tl), 200),
             "aten": (True, lambda: rouge.update(x, t, xl, tl), 3),
             "k29_update": (False, lambda: ter.update(x, t, xl, tl), 200)}
    times = {name: [] for name in sides}
    for _ in range(rounds + 1):  # the first round warms up
        for name, (disabled, fn, iters) in sides.items():
            ops.DISABLE_HIP = disabled
            times[name].append(_window(fn, iters))
    ops.DISABLE_HIP = False
    for name, v in times.items():
        res[f"{name}_ms"] = round(statistics.median(v[1:]), 5)
        res[f"{name}_ms_min_max"] = [round(min(v[1:]), 5), round(max(v[1:]), 5)]
    t0 = time.perf_counter()
    xc, tc, xn, tn = x.cpu().tolist(), t.cpu().tolist(), xl.cpu().tolist(), tl.cpu().tolist()
    t1 = time.perf_counter()
    for k in range(host_pairs):
        _table(xc[k][:xn[k]], tc[k][:tn[k]])
    t2 = time.perf_counter()
    res["host_copy_ms"] = round((t1 - t0) * 1e3, 3)
    res["host_table_ms_measured"] = round((t2 - t1) * 1e3, 3)
    res["host_route_ms_scaled"] = round((t1 - t0 + (t2 - t1) * pairs / host_pairs) * 1e3, 3)
    res["aten_over_native"] = round(res["aten_ms"] / res["native_ms"], 2)
    res["host_over_native"] = round(res["host_route_ms_scaled"] / res["native_ms"], 1)
    res["native_over_k29"] = round(res["native_ms"] / res["k29_update_ms"], 2)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "method": METHOD,
           "runs": [_shape(*s, d, args.rounds) for s in SHAPES for d in (torch.int64, torch.int32)]}
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
