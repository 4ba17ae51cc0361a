"""K1 micro accuracy, the one-shot arm of the pending-cell launch (``cls_micro_oneshot_kernel``):
taken when every wave of the grid gets at most one row (n <= 8192), the rows are 16-B aligned and
the last row's chunk ends below 2^31 bytes; every other update keeps ``cls_micro_pend_kernel``.
The shapes sit on both sides of each condition and on every count of unclamped wave-loads.  All
counts are exact integers against CPU ``torch.argmax(x.float(), 1) == target``; the random part of
the inputs is small integers in [-2, 2], so ties are common and the first-index rule decides."""

import functools

import pytest
import torch

from torcheval_amd.metrics import MulticlassAccuracy
from torcheval_amd.metrics.functional import multiclass_accuracy

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
I64, I32 = torch.int64, torch.int32
INF, NAN = float("inf"), float("nan")

SMALL_N = (1, 7, 8, 9, 63, 65)
LARGE_N = (8191, 8192, 8193)  # 8193 rows: more than one row for some wave, the loop arm
# 33: the first width above the narrow kernel's limit (f32 rows of it are not 16-B aligned, so the
# unaligned arm); 36 / 40: the first 16-B-aligned widths above it
WIDTHS = {F32: (33, 768, 769, 772, 1000, 1020, 1024), BF16: (1536, 1544, 2040, 2048), F16: (1536, 1544, 2040, 2048)}
NARROW = {F32: (33, 36), BF16: (40,), F16: (40,)}
TARGET_COLS = (0, 255, 256, 767, 768)  # and C - 1


def _f32_div(a, b):
    return float(torch.tensor(float(a)) / torch.tensor(float(b)))


def _want(x, y):
    return int((torch.argmax(x.float(), 1) == y).sum())


@functools.lru_cache(maxsize=None)
def _random_case(n, c, dtype):
    """(x on CPU, int64 targets on CPU): random rows with strict hits, targets at the columns
    where a wave-load or a lane begins or ends, out-of-range targets and non-finite rows."""
    g = torch.Generator().manual_seed(1000 * n + c)
    x = torch.randint(-2, 3, (n, c), generator=g).to(dtype)
    y = torch.randint(0, c, (n,), generator=g)
    r = torch.arange(n)
    cols = [t for t in TARGET_COLS if t < c] + [c - 1]
    for k, t in enumerate(cols):
        y[r % 16 == k] = t
    hit = r % 3 == 0  # the target holds a strict maximum
    x[r[hit], y[hit]] = 3
    y[r % 23 == 5] = -1
    y[r % 23 == 6] = c
    y[r % 23 == 7] = 2**40  # -> 0 as int32, a valid column: the oracle sees the converted targets
    x[r[r % 29 == 3], (y[r % 29 == 3] + 1).clamp(0, c - 1)] = NAN
    x[r % 31 == 4] = -INF
    x[r[r % 37 == 2], c // 2] = INF
    return x, y


def _special_rows(c, dtype):
    """One row per (target column, row kind) and one per out-of-range target."""
    rows, ys = [], []

    def add(row, t):
        rows.append(row)
        ys.append(t)

    for t in [t for t in TARGET_COLS if t < c] + [c - 1]:
        before, after = (t - 1) // 2, t + (c - t) // 2  # before < t where t > 0; after > t where t < c - 1
        base = torch.zeros(c)
        base[t] = 2
        if t > 0:
            row = base.clone()
            row[before] = 2  # the maximum duplicated before the target: wrong
            add(row, t)
        if t < c - 1:
            row = base.clone()
            row[after] = 2  # duplicated after the target: right
            add(row, t)
        row = torch.zeros(c)
        row[t] = -0.0  # -0.0 at the target, +0.0 elsewhere: equal, the first column wins
        add(row, t)
        row = torch.full((c,), -0.0)
        row[t] = 0.0  # +0.0 at the target, -0.0 elsewhere
        add(row, t)
        for pos in {t, before if t > 0 else t, after if t < c - 1 else t}:
            row = base.clone()
            row[pos] = NAN  # a NaN at / before / after the target
            add(row, t)
            row = base.clone()
            row[pos] = INF
            add(row, t)
        add(torch.full((c,), -INF), t)  # all -inf: column 0
        row = torch.full((c,), -INF)
        row[t] = -1  # the target the only finite column
        add(row, t)
    for t in (-1, c, 2**40):
        row = torch.zeros(c)
        row[0] = 1
        add(row, t)
    return torch.stack(rows).to(dtype), torch.tensor(ys, dtype=I64)


def _check(xd, x, y):
    """x: the CPU copy of the device view xd.  The metric path and the functional path, with
    int64 and with int32 targets (the oracle sees the targets as converted)."""
    for tdtype in (I64, I32):
        yt = y.to(tdtype)
        want, n = _want(x, yt.to(I64)), x.shape[0]
        yd = yt.to(DEV)
        m = MulticlassAccuracy(device=DEV)
        m.update(xd, yd)
        assert (float(m.num_correct), float(m.num_total)) == (want, n), tdtype
        assert float(m.compute()) == _f32_div(want, n), tdtype
        # one float32 rounding of a quotient in [0, 1] is at most 6e-8; one row miscounted is 1 / n > 1e-4
        assert float(multiclass_accuracy(xd, yd)) == pytest.approx(want / n, abs=1e-7), tdtype


def _count_cases():
    out = []
    for dtype in (F32, BF16, F16):
        shapes = [(n, c) for n in SMALL_N for c in WIDTHS[dtype]] + [(n, c) for n in LARGE_N for c in NARROW[dtype]]
        if dtype == F32:
            shapes.append((8192, 1000))  # the benchmark's update
        for n, c in shapes:
            out.append(pytest.param(n, c, dtype, id=f"{str(dtype)[6:]}-{n}x{c}"))
    return out


@pytest.mark.parametrize("n,c,dtype", _count_cases())
def test_counts_exactly(n, c, dtype):
    x, y = _random_case(n, c, dtype)
    _check(x.to(DEV), x, y)


@pytest.mark.parametrize("dtype,c", [(d, c) for d in (F32, BF16, F16) for c in WIDTHS[d] + NARROW[d][-1:]],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_special_rows(dtype, c):
    """Ties before and after the target, signed zeros, NaN, +inf and all -inf rows with the target
    at columns 0, 255, 256, 767, 768 and C - 1, and the out-of-range targets -1, C and 2^40."""
    x, y = _special_rows(c, dtype)
    assert x.shape[0] <= 8192
    _check(x.to(DEV), x, y)


# ------------------------------------------------------------------ layouts
@pytest.mark.parametrize("n", [65, 8192])
def test_row_strided_view(n):
    x, y = _random_case(n, 1000, F32)
    buf = torch.zeros(n, 1024, device=DEV)
    buf[:, :1000] = x.to(DEV)
    xd = buf[:, :1000]
    assert xd.stride() == (1024, 1)
    _check(xd, x, y)


@pytest.mark.parametrize("shift", [4, 1], ids=["base+16B", "base+4B"])
def test_offset_base(shift):
    """A base 16 bytes into the allocation keeps the aligned arms; 4 bytes in, the rows are only
    4-B aligned and the update must take the unaligned arm."""
    n, c = 65, 1000
    x, y = _random_case(n, c, F32)
    buf = torch.zeros(n * c + shift, device=DEV)
    xd = buf[shift:].view(n, c)
    xd.copy_(x.to(DEV))
    assert xd.data_ptr() % 16 == (4 * shift) % 16 and xd.is_contiguous()
    _check(xd, x, y)


def test_last_row_beyond_2_pow_31_bytes():
    """Rows 262400 bytes apart: the last of 8192 starts above 2^31 bytes, past what the one-shot
    arm's 32-bit row offset holds, so the update must take the 64-bit arm.  Only the view is
    written; the rest of the buffer stays uninitialised."""
    n, c, width = 8192, 1000, 65600
    x, y = _random_case(n, c, F32)
    buf = torch.empty(n, width, device=DEV)
    xd = buf[:, :c]
    xd.copy_(x.to(DEV))
    assert (n - 1) * width * 4 > 2**31 and xd.stride() == (width, 1)
    _check(xd, x, y)
    # the same rows packed from the front of the buffer: 2047 rows end below 2^31 bytes, 2048 do not
    for rows in (2047, 2048):
        _check(xd[:rows], x[:rows], y[:rows])


# ------------------------------------------------------------------ both arms into one set of cells
@pytest.mark.parametrize("order", ["oneshot-loop", "loop-oneshot"])
def test_two_updates_then_compute(order):
    a = _random_case(65, 1000, F32)  # the one-shot arm
    b = _random_case(8193, 36, F32)  # the loop arm
    first, second = (a, b) if order == "oneshot-loop" else (b, a)
    m = MulticlassAccuracy(device=DEV)
    m.update(first[0].to(DEV), first[1].to(DEV))
    m.update(second[0].to(DEV), second[1].to(DEV))
    want, total = _want(*a) + _want(*b), 65 + 8193
    assert float(m.compute()) == _f32_div(want, total)
    assert (float(m.num_correct), float(m.num_total)) == (want, total)
