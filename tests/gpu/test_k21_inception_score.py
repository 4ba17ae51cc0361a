"""K21 (csrc/kernels/inception_score.hip) on the GPU: the Inception Score's statistics in one read
of the logits, and their value.

Oracle: tests/_inception_oracle.py, numpy FP64 of the definition in docs/parity.md, on the values
the kernel sees (16-bit logits widened exactly).

* Exactness.  Dyadic cases (rows of ``0`` / ``-inf`` with ``2^t`` zeros): every probability is
  ``2^-t``, so ``prob_sum`` and ``num_rows`` must equal the constructed values exactly and
  ``neg_entropy_sum`` lie within ``n_s 2^-40`` of ``-sum t log 2``.  This pins the partition, the
  tail masking, both load arms and the fold, at every width at which a lane's share or the last
  group changes and at row counts around the splits and the blocks.
* Accuracy (the K12 / K15 / K18 rule).  Seeded logits with ``|x| <= 8``: ``split_log`` and the mean
  lie, relative, within ``MULT`` x the error of the ATen form (``DISABLE_HIP``, same device tensors)
  plus 1e-6; one float32 ulp of ``log C + 8`` is below that floor.  ``prob_sum`` lies elementwise
  within ``MULT`` x the ATen form's largest error plus ``2^-20 prob_sum``: each ``p`` carries one
  ``exp_neg`` ulp and a float32 row sum of at most 32 sequential adds per lane (33 ulps, ``2^-19``
  of ``Z`` at the very worst and ``sqrt`` of that typically), and the accumulation itself is FP64.
  ``neg_entropy_sum`` lies within ``MULT`` x ATen plus ``n_s 1e-6``.  Both errors are against the
  oracle, never against each other.
"""

import contextlib
import functools
import math

import numpy as np
import pytest
import torch

import torcheval_amd.ops as ops
from tests import _inception_oracle as O
from torcheval_amd.metrics import InceptionScore
from torcheval_amd.metrics.functional import inception_score
from torcheval_amd.metrics.functional.image.inception_score import _inception_score_stats, _inception_score_values
from torcheval_amd.ops import inception_score as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
MULT, FLOOR = 4.0, 1e-6
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
WIDTHS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000, 1008, 1023, 1024, 1025, 2047, 2048)
SPLITS = (1, 2, 10, 64)
NAN, INF = math.nan, math.inf


def row_counts(s: int):
    return sorted({n for n in (1, s - 1, s, s + 1, 4 * s, 4 * s + 1) if n >= 1})


def firsts(s: int):
    return sorted({0, min(3, s - 1), s - 1})


# every (splits, rows, first split) the exactness tests walk
COMBOS = [(s, n, f) for s in SPLITS for n in row_counts(s) for f in firsts(s)]


@pytest.fixture
def native_calls(monkeypatch):
    """Counts the calls through the K21 wrapper: the native path really ran."""
    calls = []
    for name in ("inception_update", "inception_value"):
        real = getattr(K, name)

        def spy(*a, _real=real, _name=name, **k):
            calls.append(_name)
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
def dyadic(n: int, c: int, s: int, first: int):
    """A dyadic case (CPU float32 logits, the three expected states); shared, never modified.
    ``0`` and ``-inf`` are exact in every dtype."""
    x, prob_sum, neg, rows = O.dyadic(n, c, s, first, seed=1000 * c + 10 * n + s + first)
    return torch.from_numpy(x), prob_sum, neg, rows


def check_exact(xd: torch.Tensor, case, s: int, first: int, what: str):
    _, prob_sum, neg, rows = case
    got = _inception_score_stats(xd, s, first)
    assert all(g.dtype == torch.float64 and g.device == DEV for g in got)
    p, h, r = (g.cpu().numpy() for g in got)
    assert np.array_equal(r, rows), (what, r, rows)
    assert np.array_equal(p, prob_sum), (what, np.argwhere(p != prob_sum)[:8])
    assert (np.abs(h - neg) <= rows * 2.0**-40).all(), (what, h, neg)


# ----------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("dtype", DTYPES)
def test_dyadic_rows_at_every_width(dtype, native_calls):
    """Every width, each with its share of the (splits, rows, first split) combinations, so that
    every combination meets a width; contiguous tensors, so the widths decide the load arm."""
    seen = set()
    for k, c in enumerate(WIDTHS):
        for s, n, first in COMBOS[k::len(WIDTHS)] + [(10, 41, 3)]:
            case = dyadic(n, c, s, first)
            check_exact(case[0].to(DEV, dtype), case, s, first, f"{n}x{c} S={s} first={first} {dtype}")
            seen.add((s, n, first))
    assert seen >= set(COMBOS) and native_calls and set(native_calls) == {"inception_update"}


@pytest.mark.parametrize("dtype", DTYPES)
def test_dyadic_rows_at_every_partition(dtype, native_calls):
    """Every combination at eight columns and at 257 (a lane's share of 16 with a tail)."""
    for c in (8, 257):
        for s, n, first in COMBOS:
            case = dyadic(n, c, s, first)
            check_exact(case[0].to(DEV, dtype), case, s, first, f"{n}x{c} S={s} first={first} {dtype}")
    assert len(native_calls) == 2 * len(COMBOS)


@pytest.mark.parametrize("s", [1, 10, 64])
def test_more_rows_than_the_grid_covers(s, native_calls):
    """Eight columns.  A few rows above what the capped grid of ``S x B`` blocks covers at one row
    per wave, and (S = 10) a few above what it covers at the rows per wave the grid rule aims at,
    where the cap is reached and the waves stride further."""
    per_split = K.MAX_BLOCKS // s
    counts = [s * per_split * K.WAVES_PER_BLOCK + 5]
    if s == 10:
        counts.append(s * per_split * K.WAVES_PER_BLOCK * K.ROWS_PER_WAVE_NARROW + 5)
        assert K.blocks_per_split(counts[-1], s, 8) == per_split
    for n in counts:
        first = s - 1
        case = dyadic(n, 8, s, first)
        check_exact(case[0].to(DEV), case, s, first, f"{n}x8 S={s}")
    assert len(native_calls) == len(counts)


# ----------------------------------------------------------------------------- load arms
def in_parent(v: torch.Tensor, dtype, k: int, pad: int) -> torch.Tensor:
    """``v`` ``[n, c]`` as columns ``k : k + c`` of a fresh ``[n, k + c + pad]`` parent of NaN."""
    n, c = v.shape
    parent = torch.full((n, k + c + pad), NAN, dtype=dtype, device=DEV)
    parent[:, k:k + c] = v.to(DEV, dtype)
    return parent[:, k:k + c]


@pytest.mark.parametrize("dtype", DTYPES)
def test_load_arms_padded_parents_and_column_slices(dtype, native_calls):
    """The same dyadic cases through views.  What lies around a row in its parent is NaN, so a
    load outside a row's ``C`` elements shows.  A padded parent whose row stride is a multiple of
    16 bytes keeps the 16-byte arm at every width (the guarded last group); one more column of
    padding, or a view that starts 1 or 3 columns in, takes the element arm."""
    es = torch.empty((), dtype=dtype).element_size()
    per16 = 16 // es
    s, n, first = 10, 41, 3
    for c in (1, 5, 65, 257, 1000, 1023, 1025, 2047):
        case = dyadic(n, c, s, first)
        aligned_pad = (-c) % per16 + per16
        views = {
            "padded, aligned": in_parent(case[0], dtype, 0, aligned_pad),
            "padded, unaligned": in_parent(case[0], dtype, 0, aligned_pad + 1),
            "x[:, 1:]": in_parent(case[0], dtype, 1, 0),
            "x[:, 3:]": in_parent(case[0], dtype, 3, (-(c + 3)) % per16),
        }
        assert views["padded, aligned"].data_ptr() % 16 == 0 and (views["padded, aligned"].stride(0) * es) % 16 == 0
        assert (views["padded, unaligned"].stride(0) * es) % 16 != 0
        assert views["x[:, 1:]"].data_ptr() % 16 != 0 and views["x[:, 3:]"].data_ptr() % 16 != 0
        assert (views["x[:, 3:]"].stride(0) * es) % 16 == 0  # aligned stride, base off alignment
        for name, view in views.items():
            assert not view.is_contiguous() or c == 1
            check_exact(view, case, s, first, f"{n}x{c} {dtype} {name}")
    assert len(native_calls) == 8 * 4


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_sixteen_bit_rows_of_odd_width(dtype, native_calls):
    """Contiguous 16-bit rows of odd width: every second row starts 2 bytes off a 4-byte boundary."""
    for c in (3, 63, 255, 1023, 2047):
        case = dyadic(41, c, 10, 3)
        check_exact(case[0].to(DEV, dtype), case, 10, 3, f"41x{c} {dtype}")
    case = dyadic(41, 1023, 10, 3)
    every_second = torch.full((82, 1023), NAN, dtype=dtype, device=DEV)
    every_second[::2] = case[0].to(DEV, dtype)
    check_exact(every_second[::2], case, 10, 3, "every second row")
    one_row = case[0][:1].to(DEV, dtype).expand(41, 1023)  # row stride 0
    got = _inception_score_stats(one_row, 10, 3)
    assert torch.equal(got[2].cpu(), torch.from_numpy(case[3]))
    assert len(native_calls) == 7


# ----------------------------------------------------------------------------- accuracy
@functools.lru_cache(maxsize=None)
def seeded(n: int, c: int, dtype: torch.dtype):
    """Seeded CPU logits within [-8, 8] in ``dtype``, and the oracle's states and values of them."""
    g = torch.Generator().manual_seed(7 * n + c)
    x = (torch.randn(n, c, generator=g, dtype=torch.float64) * 3).clamp(-8, 8).to(dtype)
    want = O.stats(x.double().numpy(), 10)
    return x, want, O.values(*want)


def rel(got, want):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / np.abs(want)))


def check_accuracy(got_states, got_values, aten_states, aten_values, want, want_values, what: str):
    """The accuracy rule on three states and ``(split_log, mean, std)``."""
    gp, gh, gr = (t.cpu().numpy() for t in got_states)
    ap, ah, _ = (t.cpu().numpy() for t in aten_states)
    wp, wh, wr = want
    assert np.array_equal(gr, wr)
    p_err, p_aten = np.abs(gp - wp), float(np.abs(ap - wp).max())
    h_err, h_aten = np.abs(gh - wh), float(np.abs(ah - wh).max())
    log_err, log_aten = rel(got_values[0].cpu().numpy(), want_values[0]), rel(aten_values[0].cpu().numpy(), want_values[0])
    mean_err, mean_aten = rel(float(got_values[1]), want_values[1]), rel(float(aten_values[1]), want_values[1])
    std_err = abs(float(got_values[2]) - want_values[2])
    std_aten = abs(float(aten_values[2]) - want_values[2])
    print(f"k21 {what}: gpu / aten error: prob_sum {p_err.max():.2e} / {p_aten:.2e} "
          f"(of the floor where ATen is exact: {float((p_err[wp > 0] / (2.0**-20 * wp[wp > 0])).max()):.3f}), neg_entropy_sum {h_err.max():.2e} / {h_aten:.2e}, "
          f"split_log rel {log_err:.2e} / {log_aten:.2e}, mean rel {mean_err:.2e} / {mean_aten:.2e}, "
          f"std {std_err:.2e} / {std_aten:.2e}")
    assert (p_err <= MULT * p_aten + 2.0**-20 * wp).all(), (what, "prob_sum", float(p_err.max()), p_aten)
    assert (h_err <= MULT * h_aten + wr * 1e-6).all(), (what, "neg_entropy_sum", h_err, h_aten)
    assert log_err <= MULT * log_aten + FLOOR, (what, "split_log", log_err, log_aten)
    assert mean_err <= MULT * mean_aten + FLOOR, (what, "mean", mean_err, mean_aten)
    # the deviation is a difference of values that each carry the mean's relative error
    assert std_err <= MULT * std_aten + FLOOR * want_values[1], (what, "std", std_err, std_aten)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,c", [(33, 65), (257, 1000), (64, 2048), (4101, 33)])
def test_accuracy_against_the_oracle(n, c, dtype, native_calls):
    x, want, want_values = seeded(n, c, dtype)
    xd = x.to(DEV)
    got = _inception_score_stats(xd, 10)
    got_values = _inception_score_values(*got)
    assert native_calls == ["inception_update", "inception_value"]
    mean, std = inception_score(xd, splits=10)
    assert native_calls == ["inception_update", "inception_value"] * 2
    assert mean.dtype == torch.float32 and mean.shape == () and mean.device == DEV and std.dtype == torch.float32
    assert torch.equal(mean, got_values[1]) and torch.equal(std, got_values[2])
    with aten_form():
        aten = _inception_score_stats(xd, 10)
        aten_values = _inception_score_values(*aten)
    assert len(native_calls) == 4
    check_accuracy(got, got_values, aten, aten_values, want, want_values, f"{n}x{c} {dtype}")


# ----------------------------------------------------------------------------- special values
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [5, 1000, 1023, 2048])
def test_special_values(c, dtype, native_calls):
    """``-inf`` columns are masked classes; a NaN, a ``+inf`` and an all ``-inf`` row, the entry in
    the first, a middle and the last column, make their split NaN, NaN matching the oracle's NaN
    exactly, and leave every other split bit-identical to a run without the bad rows."""
    g = torch.Generator().manual_seed(c)
    clean = (torch.randn(45, c, generator=g) * 3).clamp(-8, 8).to(dtype)
    clean[:, c // 2] = -INF
    clean[7, : c - 1] = -INF  # one class left
    x = clean.clone()
    x[3, 0] = NAN            # split 3
    x[14, c // 3] = INF      # split 4
    x[25, c - 1] = NAN       # split 5
    x[36] = -INF             # split 6
    s = 10
    want = O.stats(x.double().numpy(), s)
    bad = [3, 4, 5, 6]
    assert np.isnan(want[1]).nonzero()[0].tolist() == bad
    got = _inception_score_stats(x.to(DEV), s)
    ref = _inception_score_stats(clean.to(DEV), s)
    gp, gh, gr = (t.cpu().numpy() for t in got)
    assert np.array_equal(np.isnan(gp), np.isnan(want[0])) and np.array_equal(np.isnan(gh), np.isnan(want[1]))
    assert np.array_equal(gr, want[2])
    ok = [k for k in range(s) if k not in bad]
    assert torch.equal(got[0][ok], ref[0][ok]) and torch.equal(got[1][ok], ref[1][ok])
    split_log, mean, std = _inception_score_values(*got)
    assert split_log.isnan().nonzero().flatten().tolist() == bad and bool(mean.isnan()) and bool(std.isnan())
    assert torch.equal(split_log[ok], _inception_score_values(*ref)[0][ok])
    # the clean rows, masked classes included, against the oracle
    cw = O.stats(clean.double().numpy(), s)
    cv = O.values(*cw)
    with aten_form():
        aten = _inception_score_stats(clean.to(DEV), s)
        aten_values = _inception_score_values(*aten)
    assert (ref[0][:, c // 2] == 0).all()
    check_accuracy(ref, _inception_score_values(*ref), aten, aten_values, cw, cv, f"45x{c} {dtype} with masked classes")
    assert native_calls.count("inception_update") == 2


def test_empty_splits_and_one_split(native_calls):
    x, _, _ = seeded(33, 65, torch.float32)
    xd = x.to(DEV)
    split_log, mean, std = _inception_score_values(*_inception_score_stats(xd[:3], 5))
    assert split_log.isnan().tolist() == [False, False, False, True, True]
    assert float(mean) == pytest.approx(1.0, abs=1e-6) and float(std) == pytest.approx(0.0, abs=1e-6)
    mean, std = inception_score(xd, splits=1)
    assert float(mean) == pytest.approx(O.score(x.double().numpy(), 1)[0], rel=2e-6) and float(std) == 0.0
    assert len(native_calls) == 4
    empty = [torch.zeros(sh, dtype=torch.float64, device=DEV) for sh in ((4, 9), (4,), (4,))]
    split_log, mean, std = _inception_score_values(*empty)
    assert bool(split_log.isnan().all()) and bool(mean.isnan()) and bool(std.isnan())
    assert all(bool(v.isnan()) and v.device == DEV for v in inception_score(xd[:0], splits=3))


# ----------------------------------------------------------------------------- class
def test_class_updates_equal_the_functional_on_the_concatenation(native_calls):
    """Odd-sized updates.  What an update dispatches is the K21 op and nothing else; the states are
    views of the state buffer and are written in place."""
    from torch.utils._python_dispatch import TorchDispatchMode

    from torcheval_amd.parallel.state_buffer import buffer_of

    seen = []

    class Recorder(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    x, want, want_values = seeded(257, 1000, torch.float32)
    xd = x.to(DEV)
    m = InceptionScore(model=torch.nn.Identity(), num_classes=1000, splits=10, device=DEV)
    sb = buffer_of(m)
    assert sb is not None
    ptrs = (m.prob_sum.data_ptr(), m.neg_entropy_sum.data_ptr(), m.num_rows.data_ptr())
    parts = [xd[lo:hi] for lo, hi in ((0, 7), (7, 8), (8, 138), (138, 201), (201, 257))]
    with Recorder():
        for part in parts:
            m.update_logits(part)
    assert seen == ["torcheval_amd_inception.inception_update.default"] * 5, seen
    assert buffer_of(m, build=False) is sb
    assert (m.prob_sum.data_ptr(), m.neg_entropy_sum.data_ptr(), m.num_rows.data_ptr()) == ptrs
    whole = _inception_score_stats(xd, 10)
    assert torch.equal(m.num_rows, whole[2]) and float(m.num_rows.sum()) == 257.0
    states = (m.prob_sum, m.neg_entropy_sum, m.num_rows)
    first = m.compute()
    again = m.compute()
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert first[0].dtype == torch.float32 and first[0].device == DEV and first[0].shape == ()
    with aten_form():
        aten = _inception_score_stats(xd, 10)
        aten_values = _inception_score_values(*aten)
    check_accuracy(states, _inception_score_values(*states), aten, aten_values, want, want_values, "five updates")
    assert float(first[0]) == pytest.approx(float(inception_score(xd, splits=10)[0]), rel=1e-6)
    moved = m.to("cpu")
    assert moved.prob_sum.device.type == "cpu" and float(moved.compute()[0]) == pytest.approx(float(first[0]), rel=1e-6)
    m.reset()
    assert m._rows_seen == 0 and float(m.num_rows.sum()) == 0.0 and bool(m.compute()[0].isnan())


def test_two_runs_are_bit_identical(native_calls):
    x, _, _ = seeded(4101, 33, torch.float32)
    xd = x.to(DEV)
    a, b = _inception_score_stats(xd, 10), _inception_score_stats(xd, 10)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    va, vb = _inception_score_values(*a), _inception_score_values(*b)
    assert all(torch.equal(p, q) for p, q in zip(va, vb))
    ma = InceptionScore(model=torch.nn.Identity(), num_classes=33, device=DEV).update_logits(xd).update_logits(xd)
    mb = InceptionScore(model=torch.nn.Identity(), num_classes=33, device=DEV).update_logits(xd).update_logits(xd)
    assert torch.equal(ma.prob_sum, mb.prob_sum) and torch.equal(ma.neg_entropy_sum, mb.neg_entropy_sum)
    assert float(ma.num_rows.sum()) == 2 * 4101


def test_what_the_kernel_does_not_take_runs_the_aten_form(native_calls):
    x, _, _ = seeded(33, 65, torch.float32)
    g = torch.Generator().manual_seed(2049)
    wide = (torch.randn(12, 2049, generator=g) * 3).to(DEV)
    cases = {
        "C = 2049": (wide, 4),
        "S = 65": (x.to(DEV), 65),
        "float64": (x.double().to(DEV), 4),
        "strided last dimension": (x.to(DEV).repeat_interleave(2, dim=1)[:, ::2], 4),
    }
    for name, (xd, s) in cases.items():
        states = _inception_score_stats(xd, s)
        assert not K.supported(xd, *states), name
        assert "inception_update" not in native_calls, name
        want = O.stats(xd.double().cpu().numpy(), s)
        np.testing.assert_array_equal(states[2].cpu().numpy(), want[2])
        rtol = 1e-12 if xd.dtype == torch.float64 else 1e-5
        np.testing.assert_allclose(states[0].cpu().numpy(), want[0], rtol=rtol, atol=0)
        np.testing.assert_allclose(states[1].cpu().numpy(), want[1], rtol=rtol, atol=0)
        with aten_form():
            aten = _inception_score_stats(xd, s)
        for p, q in zip(states, aten):  # index_add_ adds in no fixed order
            torch.testing.assert_close(p, q, rtol=1e-12, atol=0)
        got = inception_score(xd, splits=s)
        assert float(got[0]) == pytest.approx(O.values(*want)[1], rel=2e-6)
    zeros = [torch.zeros(sh, dtype=torch.float64, device=DEV) for sh in ((4, 65), (4,), (4,))]
    assert K.supported(x.to(DEV), *zeros) and not K.supported(x.to(DEV), zeros[0].float(), *zeros[1:])
    # float64 results do not take the float32 value launch
    mean, _ = inception_score(cases["float64"][0], splits=4)
    assert mean.dtype == torch.float64
    # the value launch takes float32 results of up to 64 splits at any width: C = 2049 and the strided case
    assert native_calls == ["inception_value"] * 2


# ----------------------------------------------------------------------------- torch.compile
def _loop_data(i: int, c: int):
    g = torch.Generator(device=DEV).manual_seed(900 + i)
    return torch.randn(258, c, device=DEV, generator=g) * 3


@pytest.mark.parametrize("c", [10, 1000])
def test_compiled_update_loop_matches_eager(c):
    """258 rows into four splits: the split of an update's first row alternates between 0 and 2."""
    eager = InceptionScore(model=torch.nn.Identity(), num_classes=c, splits=4, device=DEV)
    comp = InceptionScore(model=torch.nn.Identity(), num_classes=c, splits=4, device=DEV)
    torch._dynamo.reset()

    @torch.compile(fullgraph=True)
    def step(x):
        comp.update_logits(x)

    for i in range(3):
        x = _loop_data(i, c)
        step(x)
        eager.update_logits(x)
    assert comp._rows_seen == eager._rows_seen == (3 * 258) % 4
    assert torch.equal(comp.prob_sum, eager.prob_sum) and torch.equal(comp.neg_entropy_sum, eager.neg_entropy_sum)
    assert torch.equal(comp.num_rows, eager.num_rows) and float(comp.num_rows.sum()) == 3 * 258
    assert comp.num_rows.tolist() == [194.0, 194.0, 193.0, 193.0]
    for p, q in zip(comp.compute(), eager.compute()):
        torch.testing.assert_close(p, q, rtol=0, atol=0)


def test_compiled_graph_holds_the_dispatcher_op():
    m = InceptionScore(model=torch.nn.Identity(), num_classes=32, splits=4, device=DEV)
    seen = []

    def backend(gm, example_inputs):
        seen.extend(str(n.target) for n in gm.graph.nodes if n.op == "call_function")
        return gm

    torch._dynamo.reset()
    step = torch.compile(lambda x: m.update_logits(x), backend=backend, fullgraph=True)
    step(_loop_data(0, 32))
    assert any("torcheval_amd_inception.inception_update" in s for s in seen), seen
    assert float(m.num_rows.sum()) == 258.0
