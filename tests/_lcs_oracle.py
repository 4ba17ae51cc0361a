"""Token LCS length and ROUGE-L exactly as docs/parity.md defines them: the two-row LCS table on Python lists
after slicing to the lengths and removing ``ignore_index``, P, R and F in Python floats, and the named cases
the CPU and GPU tests share.  A case is ``(input rows, target rows, input lengths, target lengths,
ignore_index, dtypes)``; the rows are whole padded rows, random past their lengths too, so an over-read
matches and changes the answer."""

import functools
import random

import torch

IG = -100
BOTH = ("int32", "int64")


def lcs(a, b):
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b, 1):
            cur.append(prev[j - 1] + 1 if x == y else max(prev[j], cur[j - 1]))
        prev = cur
    return prev[-1]


def prf(l, n, m):
    p, r = (l / n if n else 0.0), (l / m if m else 0.0)
    return p, r, (2 * p * r / (p + r) if p + r else 0.0)


def rnd(n, seed, symbols=(-1, 1, 2, 7)):
    r = random.Random(seed)
    return [r.choice(symbols) for _ in range(n)]


def _rows(b, width, seed, **kw):
    return [rnd(width, seed + k, **kw) for k in range(b)]


def _chunk(w):
    """Both widths ``w``, the smallest of a kernel instance: one side cut to about 70 tokens, once per side.
    The whole rows are distinct ids below 10**6.  The cut row starts with tokens of the whole row in their order, one
    from every 64-column register and more at random places, with five stray ids among them, so the answer
    hangs on a match in every register of the instance, the highest included."""
    cut, r = min(w, 70), random.Random(w + 7)
    whole = [random.Random(w + i).sample(range(10**6), w) for i in range(2)]
    places = {min(w - 1, 64 * c + r.randrange(64)) for c in range((w + 63) // 64)}
    while len(places) < cut - 6:
        places.add(r.randrange(w))
    short = []
    for i, row in enumerate(whole):
        head = [row[j] for j in sorted(places)]
        for k in range(5):
            head.insert(r.randrange(len(head) + 1), 10**6 + k)
        short.append(head + rnd(w - len(head), w + 9 + i, symbols=range(10**6)))
    return ([whole[0], short[1]], [short[0], whole[1]], [w, cut], [cut - 1, w], None, BOTH)


def _two(p, q, width=384):
    """``x`` at columns ``p`` and ``q`` of a row of ``y``."""
    return [_X if j in (p, q) else _Y for j in range(width)]


_X, _Y = 5, 9
_HI = [(1 << 32) | v for v in range(70)]
_EDGE = [0, 1, 63, 64, 65, 128, 129, 0, 70, 0]
CASES = {f"chunks_w{w}": _chunk(w) for w in (64, 65, 129, 257, 513, 1025, 2049, 4096)}
CASES.update({
    # lengths of the stationary side (input: the widths tie) round the 64-column words; an empty row on either side, on both
    "length_edges": (_rows(10, 132, 20), _rows(10, 132, 40), _EDGE, [70, 70, 70, 132, 64, 65, 1, 70, 0, 0], None, BOTH),
    # one 64-bit word: stationary lengths to its edge, stream lengths round the 64-token stream chunks
    "one_word_edges": (_rows(8, 64, 60), _rows(8, 200, 80), [0, 1, 63, 64, 64, 64, 33, 64],
                       [200, 200, 200, 0, 1, 64, 65, 128], None, BOTH),
    # a carry generated in word 0 must run through the all-ones words above it: x at column 0 (then at column
    # 63), then 255 (192) times y, against [x] and [x, y, x]
    "carry_chain": ([[_X] + [_Y] * 255] * 2 + [[_Y] * 63 + [_X] + [_Y] * 192] * 2, [[_X, _Y, _X] + [_Y] * 253] * 4,
                    None, [1, 3, 1, 3], None, BOTH),
    # a carry that has a consequence only if it crosses pure-propagate words (all ones, no match): x twice in a row of
    # y, one word or four between them, against [x] the answer is 1 and a carry lost on the way makes it 2; then [x, y, x]
    "carry_propagate": ([_two(0, 128), _two(63, 320), _two(0, 383)] * 2, [[_X, _Y, _X] + [_Y] * 381] * 6,
                        None, [1, 1, 1, 3, 3, 3], None, BOTH),
    "dense_200x130": (_rows(4, 200, 100, symbols=(0, 1, 2)), _rows(4, 130, 110, symbols=(0, 1, 2)), None, None, None, BOTH),
    "dense_130x200": (_rows(4, 130, 120, symbols=(0, 1, 2)), _rows(4, 200, 130, symbols=(0, 1, 2)), None, None, None, BOTH),
    # ids that differ only above bit 31, negative ids, the extremes; in two words and in one
    "wide_ids": ([_HI, _HI, [-v - 1 for v in range(70)], [2**63 - 1, -2**63] * 35],
                 [list(range(70)), _HI[1:] + [3], [-v - 1 if v % 3 else v for v in range(70)], [-2**63, 2**63 - 1, 0] * 23 + [0]],
                 None, [70, 70, 70, 69], None, ("int64",)),
    "wide_ids_one_word": ([_HI[:60], _HI[:60], [2**63 - 1, -2**63] * 30], [list(range(60)), _HI[1:61], [-2**63, 2**63 - 1, 0] * 20],
                          None, None, None, ("int64",)),
    # ignore_index inside the rows (at the word edges too), absent from a pair, filling a row; with lengths and without
    "ignore": ([[IG] + rnd(131, 1), rnd(132, 2), [IG] * 132, [IG if i % 7 == 0 else v for i, v in enumerate(rnd(132, 3))]],
               [rnd(63, 4) + [IG, IG] + rnd(67, 5), rnd(132, 6), rnd(132, 7), rnd(131, 8) + [IG]], [132, 100, 132, 130],
               [132, 132, 65, 132], IG, BOTH),
    "ignore_no_lengths": ([rnd(40, 9) + [IG] + rnd(20, 10), [IG] * 61], [[IG] + rnd(59, 11), rnd(60, 12)], None, None, IG, BOTH),
})
SMALL = ("chunks_w64", "chunks_w129", "length_edges", "one_word_edges", "carry_chain", "carry_propagate", "wide_ids", "ignore", "ignore_no_lengths")


@functools.lru_cache(maxsize=None)
def expected(name, rows=None):
    """The LCS lengths and the sums of P, R and F (Python floats, added in index order) of the pairs
    ``rows`` (a ``(start, stop)`` pair; all of them by default)."""
    x, t, il, tl, ignore, _ = CASES[name]
    kept = [tuple([v for v in row[:n] if v != ignore] for row, n in ((a, p), (b, q)))
            for a, b, p, q in zip(x, t, il or [None] * len(x), tl or [None] * len(x))][slice(*(rows or (None,)))]
    lengths = [lcs(a, b) for a, b in kept]
    return lengths, [sum(v) for v in zip(*(prf(l, len(a), len(b)) for l, (a, b) in zip(lengths, kept)))]


def tensors(name, dtype="int64", device="cpu"):
    """``(input, target, input_lengths, target_lengths)`` of a case."""
    x, t, il, tl = CASES[name][:4]
    ids = [torch.tensor(rows, dtype=torch.int64).to(getattr(torch, dtype)).to(device) for rows in (x, t)]
    return (*ids, *(None if n is None else torch.tensor(n, dtype=torch.int32, device=device) for n in (il, tl)))
