"""K29 (token edit distance) on one MI355X: native kernels against this package's ATen form and against
what users do today (copy the ids to the host and call ``word_error_rate`` on strings), and the wave arm
against the block arm.

Two workloads, both with about 10 % substitutions, insertions and deletions between prediction and
target, int64 and int32 ids: ``asr``, 4096 pairs with target lengths uniform in 10..60, and ``docs``, 32
pairs of 2048 target tokens.  It times one ``TokenErrorRate.update()`` natively and with
``torcheval_amd.ops.DISABLE_HIP`` set (the ATen form on the same GPU and tensors), the two alternating
over several rounds, every window device-synchronised after a warm-up; the host route (device-to-host
copy of ids and lengths plus ``word_error_rate`` on prebuilt strings, and separately the string
construction); and ``ops.edit_distance.edit_distance`` with either arm forced, alternating, at ``docs`` and
shapes in between.  Kernel times come from separate ``rocprofv3 --kernel-trace`` runs with
``--profile-loop`` (tracing slows the host, so wall times are taken with the profiler off); ``--fold`` reads
the dispatches from the traces' rocpd SQLite databases.

    python benchmarks/bench_token_edit_distance.py --out RUN.json
    rocprofv3 --kernel-trace -d DIR -o asr -- python benchmarks/bench_token_edit_distance.py --profile-loop asr
    python benchmarks/bench_token_edit_distance.py --fold RUN.json --kernel-db asr=DIR/asr_results.db --out RUN.json
"""

import argparse
import json
import os
import random
import sqlite3
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torcheval_amd.ops as ops  # noqa: E402
from torcheval_amd.metrics import TokenErrorRate  # noqa: E402
from torcheval_amd.metrics.functional import token_edit_distance, word_error_rate  # noqa: E402
from torcheval_amd.ops import edit_distance as K  # noqa: E402

WORKLOADS = {"asr": (4096, 10, 60), "docs": (32, 2048, 2048)}  # pairs, target lengths from .. to
ARM_SHAPES = ((32, 2048), (128, 1024), (256, 512), (512, 256), (1024, 256), (2048, 128))
VOCAB = 1000
KERNELS = ("edit_distance_prep", "edit_distance_wave", "edit_distance_block", "edit_distance_finish")
METHOD = ("wall: windows of back-to-back calls ending in a device synchronise, the two sides of a comparison "
          "alternating over the rounds, medians; kernels: separate rocprofv3 --kernel-trace runs of 100 native int64 "
          "updates per workload, us per launch")


def _pairs(pairs: int, lo: int, hi: int, seed: int = 0):
    """Target rows and predictions with about 10 % substitutions, insertions and deletions."""
    r = random.Random(seed)
    refs, hyps = [], []
    for _ in range(pairs):
        ref = [r.randrange(VOCAB) for _ in range(r.randint(lo, hi))]
        hyp = []
        for tok in ref:
            u = r.random()
            if u < 0.033:
                continue
            hyp.append(r.randrange(VOCAB) if u < 0.066 else tok)
            if u > 0.967:
                hyp.append(r.randrange(VOCAB))
        refs.append(ref)
        hyps.append(hyp)
    return hyps, refs


def _tensors(rows, dtype, dev):
    width = max(len(r) for r in rows)
    x = torch.tensor([r + [0] * (width - len(r)) for r in rows], dtype=dtype)
    return x.to(dev), torch.tensor([len(r) for r in rows], dtype=torch.int64).to(dev)


def _window(fn, iters: int) -> float:
    """ms per call over ``iters`` calls ending in a device synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def _alternate(sides: dict, rounds: int) -> dict:
    """Alternate the windows of ``{name: (setup, fn, iters)}``; medians and the spread over the rounds."""
    res = {name: [] for name in sides}
    for setup, fn, _ in sides.values():  # warm up every side
        setup()
        for _ in range(2):
            fn()
    for _ in range(rounds):
        for name, (setup, fn, iters) in sides.items():
            setup()
            res[name].append(_window(fn, iters))
    ops.DISABLE_HIP = False
    out = {}
    for name, v in res.items():
        out[f"{name}_ms"] = round(statistics.median(v), 5)
        out[f"{name}_ms_min_max"] = [round(min(v), 5), round(max(v), 5)]
    return out


def _hip(disabled: bool):
    def setup():
        ops.DISABLE_HIP = disabled
    return setup


def _workload(name: str, dtype, rounds: int, native_iters: int) -> dict:
    dev = torch.device("cuda", 0)
    hyps, refs = _pairs(*WORKLOADS[name])
    (x, xl), (t, tl) = _tensors(hyps, dtype, dev), _tensors(refs, dtype, dev)
    assert K.supported(x, t)
    native = token_edit_distance(x, t, xl, tl)
    ops.DISABLE_HIP = True
    aten = token_edit_distance(x, t, xl, tl)
    ops.DISABLE_HIP = False
    res = {"workload": name, "dtype": str(dtype), "pairs": x.shape[0], "widths": [x.shape[1], t.shape[1]],
           "arm": ("wave", "block")[K.pick_arm(x.shape[0], x.shape[1], t.shape[1])],
           "errors": int(native.sum()), "distances_equal_aten": bool(torch.equal(native, aten))}
    metric = TokenErrorRate(device=dev)
    update = lambda: metric.update(x, t, xl, tl)  # noqa: E731
    res["update"] = _alternate({"native": (_hip(False), update, native_iters), "aten": (_hip(True), update, 1)}, rounds)
    res["update"]["aten_over_native"] = round(res["update"]["aten_ms"] / res["update"]["native_ms"], 2)
    # what users do today: ids to the host, then the string metric (strings prebuilt; their cost apart)
    t0 = time.perf_counter()
    hs, rs = ([" ".join(map(str, r)) for r in rows] for rows in (hyps, refs))
    res["string_construction_ms"] = round((time.perf_counter() - t0) * 1e3, 3)

    def host():
        x.cpu(), t.cpu(), xl.cpu(), tl.cpu()
        return word_error_rate(hs, rs)
    assert abs(host().item() - metric.compute().item()) < 1e-6
    res["host_route"] = _alternate({"copy_and_word_error_rate": (_hip(False), host, 1)}, rounds)
    return res


def _arms(pairs: int, length: int, dtype, rounds: int) -> dict:
    dev = torch.device("cuda", 0)
    hyps, refs = _pairs(pairs, length, length, seed=pairs)
    (x, xl), (t, tl) = _tensors(hyps, dtype, dev), _tensors(refs, dtype, dev)
    got = [K.edit_distance(x, t, xl, tl, None, arm=arm) for arm in (K.ARM_WAVE, K.ARM_BLOCK)]
    iters = max(5, min(200, 2**21 // (pairs * length)))
    res = _alternate({name: (_hip(False), lambda arm=arm: K.edit_distance(x, t, xl, tl, None, arm=arm), iters)
                      for name, arm in (("wave", K.ARM_WAVE), ("block", K.ARM_BLOCK))}, rounds)
    return {"pairs": pairs, "target_length": length, "dtype": str(dtype), "arms_equal": bool(torch.equal(*got)),
            "wave_over_block": round(res["wave_ms"] / res["block_ms"], 2), **res}


def _kernel_times(db_path: str) -> dict:
    """Per K29 kernel the launches and their average / min / max us."""
    db = sqlite3.connect(db_path)
    rows = db.execute(
        "select s.kernel_name, count(*), avg(d.end - d.start), min(d.end - d.start), max(d.end - d.start) "
        "from rocpd_kernel_dispatch d join rocpd_info_kernel_symbol s on d.kernel_id = s.id group by s.kernel_name")
    out = {}
    for name, calls, avg, lo, hi in rows:
        for short in KERNELS:
            if short in name:
                out[short] = {"calls": calls, "average_us": round(avg / 1e3, 2), "min_us": round(lo / 1e3, 2),
                              "max_us": round(hi / 1e3, 2)}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--native-iters", type=int, default=100)
    ap.add_argument("--profile-loop", default=None, choices=sorted(WORKLOADS),
                    help="only run native int64 updates of one workload (under rocprofv3)")
    ap.add_argument("--fold", default=None, help="a JSON of an earlier run: add --kernel-db to it (no GPU needed)")
    ap.add_argument("--kernel-db", action="append", default=[], help="WORKLOAD=the rocpd database of its trace")
    args = ap.parse_args()
    if args.fold:
        with open(args.fold) as f:
            res = json.load(f)
        res["kernels_int64_update"] = {w: _kernel_times(p) for w, p in (s.split("=", 1) for s in args.kernel_db)}
    elif args.profile_loop:
        dev = torch.device("cuda", 0)
        hyps, refs = _pairs(*WORKLOADS[args.profile_loop])
        (x, xl), (t, tl) = _tensors(hyps, torch.int64, dev), _tensors(refs, torch.int64, dev)
        metric = TokenErrorRate(device=dev)
        for _ in range(100):
            metric.update(x, t, xl, tl)
        torch.cuda.synchronize()
        return
    else:
        dtypes = (torch.int64, torch.int32)
        res = {"device": torch.cuda.get_device_name(0), "method": METHOD,
               "dispatch": {"BLOCK_MAX_PAIRS": K.BLOCK_MAX_PAIRS, "BLOCK_MIN_WIDTH": K.BLOCK_MIN_WIDTH},
               "runs": [_workload(w, d, args.rounds, args.native_iters) for w in WORKLOADS for d in dtypes],
               "arms": [_arms(b, n, d, args.rounds) for b, n in ARM_SHAPES for d in dtypes]}
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
