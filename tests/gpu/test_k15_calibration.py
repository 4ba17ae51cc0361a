"""K15 (csrc/kernels/calibration.hip) on the GPU: multiclass calibration error in one pass.

Oracle: tests/_calibration_oracle.py, numpy FP64 of the definition in docs/parity.md.

* Probabilities: the confidence is an input value, so ``bin_count`` and ``correct_sum`` must equal
  the oracle's exactly at every shape, and on every edge ``float32(b / n_bins)`` with its two
  float32 neighbours (the test that catches a multiply-and-ceil bin function).
* Logits: a float32 confidence may differ from the FP64 one in the last bits, so the seeded CPU
  generator redraws every row whose FP64 confidence lies within 1e-3 of an edge (rows of one class
  excepted: their confidence is exactly 1 on every side); counts are then exact again.
* ``conf_sum`` and the values (the K12 rule): the GPU result lies within ``MULT`` x the error of the
  float32 ATen form (``DISABLE_HIP``, same tensors) against the FP64 oracle, plus 1e-6.  Both
  errors are against the oracle, never against each other.  Measured on an MI355X over the 1100
  logits comparisons below: where the ATen error exceeds 1e-7 (99 of them) the GPU / ATen ratio has
  median 1.0 and maximum 2.8; the largest GPU error is 2.6e-5 (``conf_sum`` of 262151 rows) against
  1.8e-5; below 1e-7 the ratio reaches 7 (2.1e-7 against 3e-8), which the floor covers.  The
  multiplier of 4 (K12's) holds without widening.

Shapes are the smallest at which each piece can go wrong: one row, fewer rows than a block's waves
and more; widths around the thread / wave arm split (32 | 33), around a lane's 16-value step and a
wave's 1024-value step (1000, 1001, 4097: the unrolled pair of steps); row starts misaligned by 1-3
elements and row-strided views; a few more rows than one launch covers per arm.
"""

import contextlib
import functools
import math

import numpy as np
import pytest
import torch

import torcheval_amd.ops as ops
from tests import _calibration_oracle as O
from torcheval_amd.config import flags
from torcheval_amd.metrics import MulticlassCalibrationError
from torcheval_amd.metrics.functional import multiclass_calibration_error
from torcheval_amd.ops import calibration as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
MULT, FLOOR = 4.0, 1e-6
NORMS = ("l1", "max", "l2")
NS = (1, 5, 37)
CS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1000, 1001, 4097)
LOGIT_BINS = (15, 100)
MARGIN = 1e-3


@pytest.fixture
def native_calls(monkeypatch):
    """Counts the calls through the K15 wrapper: the native path really ran."""
    calls = []
    for name in ("calibration_update", "calibration_error"):
        real = getattr(K, name)

        def spy(*a, _real=real, **k):
            calls.append(1)
            return _real(*a, **k)

        monkeypatch.setattr(K, name, spy)
    return calls


@contextlib.contextmanager
def aten_form():
    """The package's own ATen form on ROCm tensors (what TORCHEVAL_AMD_DISABLE_HIP=1 selects)."""
    old = ops.DISABLE_HIP
    ops.DISABLE_HIP = True
    try:
        yield
    finally:
        ops.DISABLE_HIP = old


@functools.lru_cache(maxsize=None)
def scores(n: int, c: int, seed: int, logits: bool, dtype: torch.dtype):
    """Seeded CPU scores and labels; shared between tests, never modified.  Logit rows are redrawn
    until no FP64 confidence lies within MARGIN of an edge of any LOGIT_BINS table."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, c, generator=g) * 3)
    if logits:
        x = x.to(dtype)
        e = np.unique(np.concatenate([O.edges(b).astype(np.float64) for b in LOGIT_BINS]))  # 0 first, 1 last
        while c > 1:
            conf = O.softmax_confidence(x.double().numpy())
            hi = np.clip(np.searchsorted(e, conf), 1, len(e) - 1)
            near = torch.from_numpy(np.minimum(conf - e[hi - 1], e[hi] - conf) < MARGIN)
            if not bool(near.any()):
                break
            x[near] = (torch.randn(int(near.sum()), c, generator=g) * 3).to(dtype)
    else:
        x = torch.softmax(x, dim=1).to(dtype)
    t = torch.where(torch.rand(n, generator=g) < 0.5, x.float().argmax(1), torch.randint(0, c, (n,), generator=g))
    return x, t


def oracle_states(x: torch.Tensor, t: torch.Tensor, n_bins: int, logits: bool):
    xs = x.double().numpy()
    conf = O.softmax_confidence(xs) if logits else x.float().max(dim=1).values.numpy()
    return O.states(conf, O.argmax_first(xs), t.numpy(), n_bins)


def bound(aten_err: float) -> float:
    return MULT * aten_err + FLOOR


RATIOS = []  # GPU error / ATen error of every logits comparison whose ATen error is not zero


def check(xd, td, x, t, n_bins, logits):
    """One class update and the three functional values of device tensors against the oracle, with
    the ATen form of the same tensors as the yardstick of the float errors."""
    want = oracle_states(x, t, n_bins, logits)
    m = MulticlassCalibrationError(n_bins=n_bins, from_logits=logits, device=DEV).update(xd, td)
    got = [s.cpu().numpy() for s in (m.bin_count, m.correct_sum, m.conf_sum)]
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    assert got[0].sum() == x.shape[0]
    with aten_form():
        a = MulticlassCalibrationError(n_bins=n_bins, from_logits=logits, device=DEV).update(xd, td)
        aten_vals = {norm: float(multiclass_calibration_error(xd, td, n_bins=n_bins, norm=norm, from_logits=logits))
                     for norm in NORMS}
    pairs = [(np.abs(got[2] - want[2]).max(), np.abs(a.conf_sum.cpu().numpy() - want[2]).max())]
    for norm in NORMS:
        w = O.value(*want, norm)
        v = multiclass_calibration_error(xd, td, n_bins=n_bins, norm=norm, from_logits=logits)
        assert v.dtype == torch.float32 and v.shape == () and v.device == xd.device
        pairs.append((abs(float(v) - w), abs(aten_vals[norm] - w)))
        m.norm = norm
        assert abs(float(m.compute()) - float(v)) <= 2.0**-23  # the class's value launch, same sums
    print(f"k15 {tuple(x.shape)} {x.dtype} bins {n_bins} logits {logits} (conf_sum, l1, max, l2) gpu / aten errors:",
          " ".join(f"{e:.2e}/{a:.2e}" for e, a in pairs))
    for err, aten_err in pairs:
        if logits and aten_err > 0:
            RATIOS.append(err / aten_err)
        assert err <= bound(aten_err), (err, aten_err, tuple(x.shape), n_bins, logits)


# ----------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_shapes_alignments_and_dtypes(dtype, logits, native_calls):
    i = 0
    for n in NS:
        for c in CS:
            x, t = scores(n, c, 100 + c, logits, dtype)
            td = (t if i % 2 == 0 else t.int()).to(DEV)
            n_bins = LOGIT_BINS[i % 2] if logits else (10, 15, 100)[i % 3]
            before = len(native_calls)
            check(x.to(DEV), td, x, t, n_bins, logits)
            assert len(native_calls) == before + 4  # one update, three functional calls
            # the same rows starting 1-3 elements off a fresh allocation's alignment, in a wider buffer
            k = 1 + i % 3
            wide = torch.zeros(n, c + 5, dtype=dtype, device=DEV)
            wide[:, k:k + c] = x.to(DEV)
            view = wide[:, k:k + c]
            assert view.data_ptr() % 16 != 0 and (n == 1 or c == 1 or not view.is_contiguous())
            check(view, td, x, t, n_bins, logits)
            i += 1
    # every second row of a taller buffer
    x, t = scores(37, 65, 165, logits, dtype)
    tall = torch.zeros(74, 65, dtype=dtype, device=DEV)
    tall[::2] = x.to(DEV)
    check(tall[::2], t.to(DEV), x, t, 15, logits)
    if logits:
        r = sorted(RATIOS)
        print(f"k15 error ratios {dtype}: {len(r)} comparisons, median {r[len(r) // 2]:.2f}, max {r[-1]:.2f}")


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_wave_walk_head_both_body_loops_and_tail(dtype, logits, native_calls):
    """The smallest shape that reaches every part of the wave arm's walk: columns 1:2086 of a
    [5, 2087] buffer.  Five rows are one more than a block's waves; the odd stride gives every row
    another head; the body of 2064 or 2080 values runs the two-step loop in every lane and the single
    step in the low ones, and a tail is left."""
    x, t = scores(5, 2085, 2085, logits, dtype)
    wide = torch.zeros(5, 2087, dtype=dtype, device=DEV)
    wide[:, 1:2086] = x.to(DEV)
    view = wide[:, 1:2086]
    assert view.data_ptr() % 16 != 0 and view.stride(0) == 2087
    check(view, t.to(DEV), x, t, 15, logits)
    assert len(native_calls) == 4


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("c", [2, 33])
def test_more_rows_than_one_launch_covers(c, logits, native_calls):
    n = K.rows_per_launch(c) + 7
    x, t = scores(n, c, 200 + c, logits, torch.float32)
    xd, td = x.to(DEV), t.to(DEV)
    check(xd, td, x, t, 15, logits)
    assert len(native_calls) == 4
    # two runs on the same tensors: bit-identical states and value
    a = MulticlassCalibrationError(from_logits=logits, device=DEV).update(xd, td)
    b = MulticlassCalibrationError(from_logits=logits, device=DEV).update(xd, td)
    for name in ("bin_count", "correct_sum", "conf_sum"):
        assert torch.equal(getattr(a, name), getattr(b, name))
    assert float(a.bin_count.sum()) == n
    for norm in NORMS:
        v1 = multiclass_calibration_error(xd, td, norm=norm, from_logits=logits)
        v2 = multiclass_calibration_error(xd, td, norm=norm, from_logits=logits)
        assert torch.equal(v1, v2)


@pytest.mark.parametrize("n,c,n_bins", [(401, 33, 15), (401, 33, 256), (401, 33, 1), (257, 8, 15)])
def test_finish_runs_full_short_and_empty(n, c, n_bins, native_calls):
    """The finish launch's fold over runs of blocks (tea_partials.h run_fold), float32 probabilities.
    401 rows of the wave arm are 101 blocks: with 15 bins 22 runs of 5 blocks (20 full, one of a
    single block, one empty); with 256 bins one run of seven rounds of loads, the last holding 5;
    with one bin 341 runs, 240 of them empty.  257 rows of the thread arm are two blocks.  (Two
    blocks of the wave arm and the capped 1024 are reached by the tests above.)"""
    assert n_bins <= K.max_bins()
    x, t = scores(n, c, 600 + n_bins, False, torch.float32)
    check(x.to(DEV), t.to(DEV), x, t, n_bins, False)
    assert len(native_calls) == 4


# ----------------------------------------------------------------------------- bins
@pytest.mark.parametrize("c", [3, 40])
@pytest.mark.parametrize("n_bins", [10, 15, 100])
def test_rows_on_the_edges_and_next_to_them(n_bins, c, native_calls):
    e = O.edges(n_bins)
    v = np.concatenate([e, np.nextafter(e, np.float32(2)), np.nextafter(e, np.float32(-1))])
    v = v[(v >= 0) & (v <= 1)]
    x = torch.zeros(len(v), c)
    x[:, c - 2] = torch.from_numpy(v)
    t = torch.full((len(v),), c - 2, dtype=torch.int64)
    t[::3] = 0
    m = MulticlassCalibrationError(n_bins=n_bins, device=DEV).update(x.to(DEV), t.to(DEV))
    assert len(native_calls) == 1
    want = O.states(v, O.argmax_first(x.numpy()), t.numpy(), n_bins)
    assert np.array_equal(m.bin_count.cpu().numpy(), want[0])
    assert np.array_equal(m.correct_sum.cpu().numpy(), want[1])
    np.testing.assert_allclose(m.conf_sum.cpu().numpy(), want[2], rtol=2.0**-45, atol=0)


def test_bins_at_the_cap_and_one_above(native_calls):
    x, t = scores(37, 65, 165, False, torch.float32)
    xd, td = x.to(DEV), t.to(DEV)
    cap = K.max_bins()
    check(xd, td, x, t, cap, False)
    assert len(native_calls) == 4
    check(xd, td, x, t, cap + 1, False)  # the ATen form: no native call
    assert len(native_calls) == 4
    x, t = scores(37, 2, 102, False, torch.float32)
    check(x.to(DEV), t.to(DEV), x, t, cap, False)
    assert len(native_calls) == 8


# ----------------------------------------------------------------------------- bad rows
def _bad_cases(c: int):
    x, t = scores(9, c, 300 + c, False, torch.float32)
    lx, lt = scores(9, c, 310 + c, True, torch.float32)
    out = []
    bt = t.clone()
    bt[4] = c
    out.append(("target", x, bt, False, 1))
    bt = t.clone()
    bt[4] = -1
    out.append(("target", x, bt, False, 1))
    for logits, base, lab in ((False, x, t), (True, lx, lt)):
        nan = base.clone()
        nan[4, c - 1] = math.nan
        out.append(("nan", nan, lab, logits, 2))
    inf = lx.clone()
    inf[4, 1] = math.inf
    out.append(("+inf", inf, lt, True, 2))
    ninf = lx.clone()
    ninf[4] = -math.inf
    out.append(("all -inf", ninf, lt, True, 2))
    big = x.clone()
    big[4, 0] = 1.5
    out.append(("above 1", big, t, False, 2))
    both = x.clone()
    both[4, 0] = math.nan
    bt = t.clone()
    bt[4] = c + 3
    out.append(("both", both, bt, False, 3))
    return out


@pytest.mark.parametrize("c", [5, 40])
def test_bad_rows(c, native_calls):
    keep = [0, 1, 2, 3, 5, 6, 7, 8]
    for name, x, t, logits, bits in _bad_cases(c):
        xd, td = x.to(DEV), t.to(DEV)
        for norm in NORMS:  # validate is off: no raise, the value is NaN
            assert multiclass_calibration_error(xd, td, norm=norm, from_logits=logits).isnan(), name
        m = MulticlassCalibrationError(from_logits=logits, device=DEV)
        m.update(xd[:4], td[:4])
        m.update(xd, td)  # no raise at the update
        assert int(m._err.item()) == bits, name
        first, good = oracle_states(x[:4], t[:4], 15, logits), oracle_states(x[keep], t[keep], 15, logits)
        want = [a + b for a, b in zip(first, good)]
        assert np.array_equal(m.bin_count.cpu().numpy(), want[0]), name
        assert np.array_equal(m.correct_sum.cpu().numpy(), want[1]), name
        conf = m.conf_sum.cpu().numpy()
        assert math.isnan(conf[0]) and not np.isnan(conf[1:]).any()
        # 12 rows of float32 confidences, each within 2e-6 of its FP64 value
        np.testing.assert_allclose(conf[1:], want[2][1:], rtol=0, atol=12 * 2e-6)
        with pytest.raises(ValueError, match="label outside" if bits & 1 else "confidence is not in"):
            m.compute()
        assert int(m._err.item()) == 0 and float(m.bin_count.sum()) == 12.0  # the flag cleared, nothing else
        assert m.compute().isnan()  # and no second raise
        m.reset()
        assert not m.update(xd[keep], td[keep]).compute().isnan()
        with flags(validate=True):
            with pytest.raises(ValueError, match="label outside" if bits & 1 else "confidence is not in"):
                multiclass_calibration_error(xd, td, from_logits=logits)
            assert not multiclass_calibration_error(xd[keep], td[keep], from_logits=logits).isnan()
    assert len(native_calls) > 0


# ----------------------------------------------------------------------------- class
@pytest.mark.parametrize("c", [10, 300])
def test_class_update_is_one_native_op_and_no_aten_op(c, native_calls):
    """What an update dispatches: the K15 op (its two launches) and nothing else.  States after
    four updates equal those of one update with all rows, bit for bit in the counts."""
    from torch.utils._python_dispatch import TorchDispatchMode

    from torcheval_amd.parallel.state_buffer import buffer_of

    seen = []

    class Recorder(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    x, t = scores(43, c, 400 + c, True, torch.float32)
    xd, td = x.to(DEV), t.to(DEV)
    m = MulticlassCalibrationError(from_logits=True, device=DEV)
    sb = buffer_of(m)
    assert sb is not None
    ptrs = tuple(s.data_ptr() for s in (m.bin_count, m.correct_sum, m.conf_sum))
    parts = [(xd[lo:hi], td[lo:hi]) for lo, hi in ((0, 5), (5, 6), (6, 42), (42, 43))]
    with Recorder():
        for px, pt in parts:
            m.update(px, pt)
    assert seen == ["torcheval_amd_calibration.calibration_update.default"] * 4, seen
    assert len(native_calls) == 4
    assert buffer_of(m, build=False) is sb
    assert tuple(s.data_ptr() for s in (m.bin_count, m.correct_sum, m.conf_sum)) == ptrs
    whole = MulticlassCalibrationError(from_logits=True, device=DEV).update(xd, td)
    assert torch.equal(m.bin_count, whole.bin_count) and torch.equal(m.correct_sum, whole.correct_sum)
    torch.testing.assert_close(m.conf_sum, whole.conf_sum, rtol=2.0**-45, atol=0)
    for norm in NORMS:
        m.norm = norm
        got = m.compute()
        assert got.dtype == torch.float32 and got.is_cuda and got.shape == ()
        v = multiclass_calibration_error(xd, td, norm=norm, from_logits=True)
        assert abs(float(got) - float(v)) <= 2.0**-23
    moved = m.to("cpu")
    assert moved.bin_count.device.type == "cpu" and abs(float(moved.compute()) - float(got)) <= 2.0**-23
    m.reset()
    assert float(m.bin_count.sum()) == 0.0 and m.compute().isnan()


def _loop_data(i: int, c: int):
    g = torch.Generator(device=DEV).manual_seed(500 + i)
    x = torch.randn(256, c, device=DEV, generator=g) * 3
    return x, torch.randint(0, c, (256,), device=DEV, generator=g)


@pytest.mark.parametrize("c", [10, 300])
def test_compiled_update_loop_matches_eager(c):
    eager = MulticlassCalibrationError(from_logits=True, device=DEV)
    comp = MulticlassCalibrationError(from_logits=True, device=DEV)
    torch._dynamo.reset()

    @torch.compile(fullgraph=True)
    def step(*args):
        comp.update(*args)

    for i in range(4):
        x, t = _loop_data(i, c)
        step(x, t)
        eager.update(x, t)
    for name in ("bin_count", "correct_sum", "conf_sum"):
        assert torch.equal(getattr(comp, name), getattr(eager, name))
    assert float(comp.bin_count.sum()) == 1024.0
    torch.testing.assert_close(comp.compute(), eager.compute(), rtol=0, atol=0)


def test_compiled_graph_holds_the_dispatcher_op():
    m = MulticlassCalibrationError(device=DEV)
    seen = []

    def backend(gm, example_inputs):
        seen.extend(str(n.target) for n in gm.graph.nodes if n.op == "call_function")
        return gm

    torch._dynamo.reset()
    step = torch.compile(lambda x, y: m.update(x, y), backend=backend, fullgraph=True)
    x, t = _loop_data(0, 32)
    step(x.softmax(1), t)
    assert any("torcheval_amd_calibration.calibration_update" in s for s in seen), seen
    assert float(m.bin_count.sum()) == 256.0
