"""Token edit distance exactly as docs/parity.md defines it: the two-row Levenshtein table on Python lists
after slicing to the lengths and removing ``ignore_index``, and the named cases the CPU and GPU tests share.
A case is ``(pairs, ignore_index, extra, dtypes, group)``: ``pairs`` the true ``(input, target)`` rows, ``extra``
columns of padding filled with ``PAD`` on both sides (so an over-read matches and changes the answer; lengths
are passed exactly when ``extra > 0`` or the rows differ in length), ``group`` the GPU test item it runs in."""

import functools
import random

import torch

from torcheval_amd.metrics.functional.text import (
    _wil_compute,
    _word_error_rate_compute,
    _word_information_preserved_compute,
)

PAD, IG = 1, -100
SYMBOLS = (-1, 1, 2)  # three symbols: dense in ties between up, left and diag; PAD is one of them


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def rnd(n, seed):
    r = random.Random(seed)
    return [r.choice(SYMBOLS) for _ in range(n)]


def _pairs(lengths, make):
    return [(make(n, 2 * k), make(m, 2 * k + 1)) for k, (n, m) in enumerate(lengths)]


_EDGES = [(0, 0), (0, 65), (65, 0), (1, 129), (129, 1), (64, 64), (65, 64), (64, 65), (129, 130)]
_HI = [(1 << 32) | v for v in range(70)]
_R = rnd(200, 99)
BOTH = ("int32", "int64")
CASES = {
    "rnd3_b9": (_pairs(_EDGES, rnd), None, 3, BOTH, "strips"),
    "equal_b5": (_pairs([(64, 64), (65, 64), (64, 65), (1, 129), (129, 130)], lambda n, k: [5] * n), None, 0, BOTH, "strips"),
    "different_b5": (_pairs([(0, 65), (65, 0), (63, 128), (128, 63), (129, 1)],
                            lambda n, k: list(range(1000 * k, 1000 * k + n))), None, 2, BOTH, "strips"),
    "shift_b1": ([(_R[:129], _R[1:130])], None, 0, BOTH, "strips"),
    "full_64_b1": ([(rnd(64, 7), rnd(64, 8))], None, 0, BOTH, "strips"),
    "empty_b1": ([([], [])], None, 2, BOTH, "strips"),
    # ids that differ only above bit 32, and negative ids
    "wide_ids_b5": ([(_HI, list(range(70))), (_HI[:65], _HI[1:66]), ([-v - 1 for v in range(64)], list(range(64))),
                     ([-(1 << 40)] * 3, [-(1 << 40), 1 << 40]), ([2**63 - 1, -2**63], [-2**63, 2**63 - 1])], None, 1,
                    ("int64",), "ids_and_ignore"),
    # ignore_index at position 0, at 63 and 64, at the end, all of a row, and with lengths
    "ignore_b5": ([([IG] + rnd(70, 1), _R[:63] + [IG, IG] + _R[63:66] + [IG]), ([IG] * 70, rnd(65, 2)),
                   ([IG if i % 7 == 0 else v for i, v in enumerate(rnd(130, 3))], rnd(129, 4) + [IG]),
                   ([IG] * 3, [IG]), ([2, IG], rnd(129, 5))], IG, 2, BOTH, "ids_and_ignore"),
    "ignore_nolen_b1": ([(_R[:64] + [IG] + _R[70:100], [IG] + _R[:95])], IG, 0, BOTH, "ids_and_ignore"),
    "long_stream_b1": ([(rnd(4096, 11), rnd(70, 12))], None, 0, BOTH, "capacity"),
    "long_lanes_b1": ([(rnd(70, 13), rnd(4096, 14))], None, 0, BOTH, "capacity"),
    # more strips than the block arm has waves, so a wave wraps round to a second strip while its neighbours
    # still work on the edge column: 10 strips of 11 macro steps (a round is 2 W = 16 macro steps) ...
    "two_rounds_b1": ([(rnd(600, 15), rnd(600, 16))], None, 0, BOTH, "capacity"),
    # ... and 10 strips, the last one partial, of 19 macro steps (a round is the 19 of one strip)
    "two_rounds_long_b1": ([(rnd(1100, 17), rnd(600, 18))], None, 0, BOTH, "capacity"),
}
# a GPU test item is a group of cases
GROUPS = {g: tuple(n for n in CASES if CASES[n][4] == g) for g in ("strips", "ids_and_ignore", "capacity")}


@functools.lru_cache(maxsize=None)
def expected(name):
    """The distances and the totals (errors, input_total, target_total, max_total), Python ints."""
    pairs, ignore = CASES[name][0], CASES[name][1]
    kept = [([v for v in a if v != ignore], [v for v in b if v != ignore]) for a, b in pairs]
    d = [levenshtein(a, b) for a, b in kept]
    return d, (sum(d), sum(len(a) for a, _ in kept), sum(len(b) for _, b in kept),
               sum(max(len(a), len(b)) for a, b in kept))


def tensors(name, dtype="int64", device="cpu"):
    """``(input, target, input_lengths, target_lengths)`` of a case; the lengths None where every row is full."""
    pairs, _, extra = CASES[name][:3]
    out, lens = [], []
    for side in (0, 1):
        rows = [p[side] for p in pairs]
        width = max(len(r) for r in rows) + extra
        out.append(torch.tensor([r + [PAD] * (width - len(r)) for r in rows], dtype=torch.int64)
                   .reshape(len(rows), width).to(getattr(torch, dtype)).to(device))
        full = all(len(r) == width for r in rows)
        lens.append(None if full else torch.tensor([len(r) for r in rows], dtype=torch.int32, device=device))
    return out[0], out[1], lens[0], lens[1]


def total_tensors(totals, device="cpu"):
    return [torch.tensor(float(v), dtype=torch.float64, device=device) for v in totals]


def measures(totals, device="cpu"):
    """The four measures as the word-level ``_compute`` functions give them on the oracle's totals."""
    e, i, t, m = total_tensors(totals, device)
    return {"wer": _word_error_rate_compute(e, t), "mer": _word_error_rate_compute(e, m),
            "wil": _wil_compute(e - m, t, i), "wip": _word_information_preserved_compute(m - e, t, i)}


def bits(x):
    return x.cpu().view(torch.int64)
