"""K1 micro accuracy, head and tail: every launch arm of ``cls_micro_pend_kernel`` (its
parameters travel as preloaded plain kernel arguments) and the fold kernel
``micro_finish_kernel`` that closes a run of updates.  All counts are exact integers against CPU
``torch.argmax(x, 1) == target``; inputs are small integers in [-2, 2], so ties are common and
the first-index rule decides."""

import functools
import importlib.util
import json
import os
import subprocess
import sys

import pytest
import torch

from torcheval_amd.metrics import MulticlassAccuracy

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
I64, I32 = torch.int64, torch.int32


@functools.lru_cache(maxsize=None)
def _case(n, c, layout, dtype, seed=0):
    """(x view on CPU, targets int64 on CPU, correct count).  Layouts: ``plain`` [n, c];
    ``shift`` the view x[:, 1:] of [n, c + 1] (rows start 4 or 2 bytes off 16-B alignment);
    ``strided`` the view x[:, :c] of [n, c + 8] (row_stride != c)."""
    g = torch.Generator().manual_seed(1000 * n + c + seed)
    width = {"plain": c, "shift": c + 1, "strided": c + 8}[layout]
    full = torch.randint(-2, 3, (n, width), generator=g).to(dtype)
    x = {"plain": full, "shift": full[:, 1:], "strided": full[:, :c]}[layout]
    y = torch.randint(0, c, (n,), generator=g)
    r = torch.arange(n)
    hit = r % 3 == 0  # a share of rows whose target holds a strict maximum
    x[r[hit], y[hit]] = 3
    y[r % 11 == 5] = -1  # never correct
    y[r % 13 == 6] = c  # never correct
    # NaN before / at / after the target's column (torch.argmax: NaN is the max, first NaN wins)
    for k, off in ((4, -1), (5, 0), (6, 1)):
        rows = r[(r % 7 == k) & (y > 0) & (y < c - 1)]
        x[rows, y[rows] + off] = float("nan")
    want = int((torch.argmax(x.float(), 1) == y).sum())
    return x, y, want


def _run(n, c, layout, dtype, tdtype):
    x, y, want = _case(n, c, layout, dtype)
    base = {"plain": None, "shift": 1, "strided": 0}[layout]
    if base is None:
        xd = x.to(DEV)
    else:  # rebuild the same view on the device (a copy of the view would be contiguous)
        xd = x._base.to(DEV)[:, base : base + c]
    assert xd.shape == (n, c) and xd.stride(1) == 1
    m = MulticlassAccuracy(device=DEV)
    m.update(xd, y.to(tdtype).to(DEV))
    return float(m.num_correct), float(m.num_total), want


def _update_cases():
    out = []
    for dtype in (F32, BF16, F16):
        shapes = [(1, 1000, "plain"), (7, 1000, "plain"), (8, 1000, "plain"), (9, 1000, "plain"),
                  (8193, 33, "plain"), (67, 33, "plain"), (67, 1000, "plain"), (67, 1024, "plain"),
                  (67, 1000, "strided"), (67, 33, "strided")]
        if dtype == F32:  # the UNAL arm: 16-B loads from 4-B-aligned rows
            shapes += [(67, 1001, "plain"), (67, 1000, "shift"), (9, 33, "shift")]
        else:  # 16-bit rows stay on the micro path up to 2048 columns
            shapes += [(67, 2048, "plain"), (9, 2048, "strided")]
        for n, c, layout in shapes:
            for tdtype in (I64, I32):
                out.append(pytest.param(n, c, layout, dtype, tdtype,
                                        id=f"{str(dtype)[6:]}-{str(tdtype)[6:]}-{n}x{c}-{layout}"))
    return out


@pytest.mark.parametrize("n,c,layout,dtype,tdtype", _update_cases())
def test_update_arm_counts_exactly(n, c, layout, dtype, tdtype):
    got, total, want = _run(n, c, layout, dtype, tdtype)
    assert (got, total) == (want, n)


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
@pytest.mark.parametrize("tdtype", [I64, I32])
@pytest.mark.parametrize("c", [33, 1000])
def test_nan_rows_before_at_after_target(dtype, tdtype, c):
    """One row each: a NaN before, at and after the target's column, the target otherwise the
    strict maximum.  Only the NaN at the target's column leaves the row correct."""
    t = c // 2
    x = torch.zeros(3, c)
    x[:, t] = 2
    x[0, t - 1] = x[1, t] = x[2, t + 1] = float("nan")
    x, y = x.to(dtype), torch.full((3,), t)
    assert (torch.argmax(x.float(), 1) == y).tolist() == [False, True, False]
    for keep in ([0], [1], [2], [0, 1, 2]):
        m = MulticlassAccuracy(device=DEV)
        m.update(x[keep].to(DEV), y[keep].to(tdtype).to(DEV))
        assert float(m.num_correct) == float(1 in keep) and float(m.num_total) == len(keep)


# ------------------------------------------------------------------ the 4-wave arm (child process)
_WPB4_CASES = [(n, c, layout, dtype, tdtype)
               for dtype in (F32, BF16, F16) for tdtype in (I64, I32)
               for n, c, layout in ((9, 1000, "plain"), (8193, 33, "plain"), (67, 1000, "strided"))] + \
              [(67, 1001, "plain", F32, I64), (67, 1000, "shift", F32, I32)]


def child_main():
    bad = []
    for n, c, layout, dtype, tdtype in _WPB4_CASES:
        got, total, want = _run(n, c, layout, dtype, tdtype)
        if (got, total) != (want, n):
            bad.append([n, c, layout, str(dtype), str(tdtype), got, total, want])
    print(json.dumps({"wpb": os.environ.get("TORCHEVAL_AMD_K1_WPB"), "cases": len(_WPB4_CASES), "failures": bad}))


def test_four_wave_arm_in_child_process():
    """TORCHEVAL_AMD_K1_WPB=4 is read once per process, so the 256-thread form runs in a child."""
    child = (
        "import importlib.util as u; s = u.spec_from_file_location('k1_head_tail', %r); "
        "m = u.module_from_spec(s); s.loader.exec_module(m); m.child_main()" % os.path.abspath(__file__)
    )
    env = dict(os.environ, TORCHEVAL_AMD_K1_WPB="4")
    r = subprocess.run([sys.executable, "-c", child], env=env, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["wpb"] == "4" and res["cases"] == len(_WPB4_CASES) == 20
    assert res["failures"] == []


# ------------------------------------------------------------------ the fold
def _batch(seed, tdtype=I64):
    x, y, want = _case(67, 1000, "plain", F32, seed)
    return x.to(DEV), y.to(tdtype).to(DEV), want


def _f32_div(a, b):
    return float(torch.tensor(float(a)) / torch.tensor(float(b)))


def test_fold_twice_zeroes_the_cells():
    m = MulticlassAccuracy(device=DEV)
    wants = []
    for seed in (1, 2, 3):
        x, y, w = _batch(seed)
        m.update(x, y)
        wants.append(w)
    assert float(m.compute()) == _f32_div(sum(wants), 3 * 67)
    assert int(m.__dict__["_pend"].abs().sum()) == 0
    for seed in (4, 5):
        x, y, w = _batch(seed)
        m.update(x, y)
        wants.append(w)
    assert float(m.compute()) == _f32_div(sum(wants), 5 * 67)
    assert float(m.num_correct) == sum(wants) and float(m.num_total) == 5 * 67


def test_num_correct_reads_with_and_without_pending_cells():
    m = MulticlassAccuracy(device=DEV)
    assert float(m.num_correct) == 0.0  # nothing pending: no fold
    x, y, w = _batch(6)
    m.update(x, y)
    assert m.__dict__["_pend_dirty"]
    assert float(m.num_correct) == w  # the fold without an output (out = None)
    assert not m.__dict__["_pend_dirty"] and int(m.__dict__["_pend"].abs().sum()) == 0
    assert float(m.num_correct) == w and float(m.num_total) == 67  # nothing pending again


def test_reset_with_cells_pending():
    m = MulticlassAccuracy(device=DEV)
    x, y, _ = _batch(7)
    m.update(x, y)
    m.reset()
    x, y, w = _batch(8)
    m.update(x, y)
    assert float(m.compute()) == _f32_div(w, 67)
    assert float(m.num_correct) == w and float(m.num_total) == 67


@pytest.mark.parametrize("hits", [1, 3, 5])
def test_fold_adds_in_float32_above_2_pow_24(hits):
    """num_correct holds 2^24 + 2 (float32 spacing 2 there): adding an odd count must round as
    the CPU's float32 add does (ties to even), not be carried in a wider type."""
    c0 = 2**24 + 2
    x = torch.zeros(9, 33)
    y = torch.full((9,), 5)
    x[:hits, 5] = 1  # rows 0..hits-1 are correct; all-zero rows predict column 0
    assert int((torch.argmax(x, 1) == y).sum()) == hits
    m = MulticlassAccuracy(device=DEV)
    m.num_correct = torch.tensor(float(c0), device=DEV)
    m.update(x.to(DEV), y.to(DEV))
    want = torch.tensor(float(c0), dtype=torch.float32) + torch.tensor(float(hits), dtype=torch.float32)
    assert float(m.num_correct) == float(want)
    assert float(want) != c0 + hits  # the case does round
