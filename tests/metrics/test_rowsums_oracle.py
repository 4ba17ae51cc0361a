"""The K5b host twin (csrc/runtime/rowsums_host.cpp, CPU tensors of at most HOST_MAX elements)
against the float64 oracle of tests/_rowsums_oracle.py, and the argument check both devices share.

The exact family must match bit for bit, the float family within the derived bound; both are
described in tests/_rowsums_cases.py, which also builds the cases the GPU arms run."""

import pytest
import torch

from tests import _rowsums_cases as C
from tests import _rowsums_oracle as O
from tests._rowsums_cases import F32, F64, Case, Out
from tests._rowsums_oracle import ADD, COUNT, MAX, MIN, RANGE, SET, SSE, TMAX, TMIN, W, WSSE, WT, WTT, WX
from torcheval_amd.ops import native, rowsums as rs

ALL = C.SETS["all"]


def _run(cases):
    for c in cases:
        assert c.rows * c.n <= rs.HOST_MAX
    bad = C.run_cases(cases, "cpu")
    assert not bad, bad[:8]


def test_oracle_constants_are_the_table():
    assert (WX, WT, W, SSE, WSSE, WTT, TMIN, TMAX, COUNT, RANGE) == (
        rs.WX, rs.WT, rs.W, rs.SSE, rs.WSSE, rs.WTT, rs.TMIN, rs.TMAX, rs.COUNT, rs.RANGE)
    assert (SET, ADD, MIN, MAX, O.FIRST_ROW) == (rs.SET, rs.ADD, rs.MIN, rs.MAX, rs.FIRST_ROW)
    assert rs.HOST_MAX == 8192


def test_oracle_by_hand():
    """The oracle itself on numbers small enough to check on paper."""
    x = torch.tensor([[1.0, 2.0, 3.0], [0.0, -1.0, 4.0]])
    t = torch.tensor([[0.0, 2.0, 5.0], [1.0, 1.0, 1.0]])
    w = torch.tensor([[1.0, 0.0, 2.0], [3.0, 1.0, 1.0]])
    z = lambda v=0.0, dt=F64: torch.full((2,), v, dtype=dt)
    outs = [(z(), WX, SET), (z(), WT, SET), (z(), W, SET), (z(), SSE, SET), (z(), WSSE, SET), (z(), WTT, SET),
            (z(1.0), TMIN, MIN), (z(3.0, F32), TMAX, MAX), (z(10.0), COUNT, ADD), (z(), RANGE, SET)]
    got = O.rowsums_oracle(x, t, w, 1.0, outs, 2)
    want = [[7.0, 3.0], [10.0, 5.0], [3.0, 5.0], [5.0, 14.0], [9.0, 16.0], [50.0, 5.0], [0.0, 1.0], [5.0, 3.0],
            [13.0, 13.0], [5.0, 2.0]]
    assert [g.tolist() for g in got] == want
    assert got[7].dtype == F32 and outs[6][0].tolist() == [1.0, 1.0]  # the initial states are not written
    # a scalar weight scales the weighted sums once per row, never SSE; W = w * n
    got = O.rowsums_oracle(x, t, None, 0.5, [(z(), WX, SET), (z(), W, SET), (z(), SSE, SET), (z(), WSSE, SET)], 2)
    assert [g.tolist() for g in got] == [[3.0, 1.5], [1.5, 1.5], [5.0, 14.0], [2.5, 7.0]]
    # row 0 alone feeds a FIRST_ROW output; NaN goes through MIN and MAX; an f32 state rounds the value
    t[1, 2] = float("nan")
    one = torch.zeros((), dtype=F32)
    got = O.rowsums_oracle(x.double() + 2.0 ** -30, t, None, 1.0,
                           [(one, WX, ADD | O.FIRST_ROW), (z(), TMIN, MIN), (z(), TMAX, MAX)], 2)
    assert got[0].tolist() == 6.0 and got[1][0] == 0.0 and got[2][0] == 5.0
    assert torch.isnan(got[1][1]) and torch.isnan(got[2][1])


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("op", [SET, ADD, MIN, MAX], ids=["set", "add", "min", "max"])
def test_every_statistic_with_every_op(op, dtype):
    outs = [Out(s, op, dtype, 1.5) for s in ALL]
    _run([Case(f"host-op{op}-{rows}x{n}-{weight}", "exact", rows, n, outs, weight=weight)
          for rows, n in ((1, 1), (3, 37), (1, 8192), (4, 2048)) for weight in ("tensor", 0.5, 3.0)])


def test_first_row_and_ring_slot_outputs():
    outs = [Out(WX, ADD, F64, 2.0, ring=True), Out(WSSE, SET, F32, 0.0, ring=True), Out(TMIN, MIN, F64, 0.0),
            Out(TMAX, MAX, F32, 0.0, first_row=True), Out(COUNT, ADD, F32, 4.0, first_row=True),
            Out(RANGE, SET, F64, 0.0), Out(W, ADD, F64, 0.0, first_row=True)]
    _run([Case(f"host-ring-{rows}-{weight}", "exact", rows, 129, outs, weight=weight)
          for rows in (1, 5) for weight in ("tensor", 2.0)])


@pytest.mark.parametrize("dt", rs._IN_DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_every_input_dtype(dt):
    outs = C.outs_for(ALL, "a")
    _run([Case(f"host-x-{dt}", "exact", 3, 100, outs, x_dtype=dt),
          Case(f"host-xtw-{dt}", "exact", 3, 100, C.outs_for(ALL, "b"), x_dtype=dt, t_dtype=dt, w_dtype=dt),
          Case(f"host-x-{dt}-scalar", "exact", 2, 77, outs, x_dtype=dt, weight=0.5),
          Case(f"host-x-{dt}-strided", "exact", 2, 77, outs, x_dtype=dt, transposed=True)])


def test_empty_rows():
    _run([Case(f"host-n0-{rows}-{weight}-{style}", "exact", rows, 0, C.outs_for(ALL, style), weight=weight)
          for rows in (1, 3) for weight in ("tensor", 2.0) for style in ("a", "b")])


@pytest.mark.parametrize("kind", ["nan", "min", "max"])
def test_special_target_at_every_place(kind):
    cases = [Case(f"host-{kind}-{rows}x{n}-{col}-{style}", "exact", rows, n, C.outs_for(C.SETS["psnr"], style),
                  weight=weight, edit=(kind, col))
             for rows, n in ((1, 768), (3, 101)) for col in (0, n // 2, n - 1)
             for style, weight in (("a", "tensor"), ("b", 2.0))]
    _run(cases)
    for c in cases:  # what the oracle says of these cases
        sse, tmin, tmax, _, rng = C.expected_states(c, *C.values(c))
        last = c.rows - 1
        if kind == "nan":
            assert all(bool(torch.isnan(v.reshape(-1)[last])) for v in (sse, tmin, tmax, rng)), c.id
        elif kind == "min":
            assert float(tmin[last]) == -100.0, c.id
        else:
            assert float(tmax[last]) == 100.0, c.id


def test_float_family_within_the_derived_bound():
    _run([Case(f"host-float-{rows}x{n}-{weight}", "float", rows, n, C.outs_for(ALL, "f"), weight=weight)
          for rows, n in ((1, 5), (3, 1000), (1, 8192)) for weight in ("tensor", 0.5)])


def test_offset_views():
    _run([Case(f"host-offset-{n}", "exact", 3, n, C.outs_for(ALL, "a"), offsets=(1, 2, 3)) for n in (5, 1001)])


@pytest.mark.parametrize("stats", [(WX,), (W,), (COUNT,), (WX, W, COUNT)], ids=["wx", "w", "count", "wx_w_count"])
def test_sets_that_read_no_target_need_none(stats):
    _run([Case(f"host-no-target-{weight}", "exact", 3, 100, C.outs_for(stats, "a"), weight=weight, has_t=False)
          for weight in ("tensor", 3.0)])


@pytest.mark.parametrize("stat", O.NEEDS_T, ids=[C.STAT_NAME[s] for s in O.NEEDS_T])
def test_a_statistic_that_reads_the_target_is_refused_without_one(stat):
    """row_sums_args: the host twin would take t as 0, the kernel would read through a null pointer."""
    x, w = torch.ones(2, 8), torch.ones(2, 8)
    state = torch.full((2,), 4.0, dtype=F64)
    code = rs.code(stat, SET if stat == RANGE else ADD)
    for weight in (None, w):
        with pytest.raises(RuntimeError, match="needs t"):
            native().row_sums(x, None, weight, 1.0, [state], [code], 2)
        with pytest.raises(RuntimeError, match="needs t"):
            torch.ops.torcheval_amd.row_sums(x, None, weight, 1.0, [state], [code], 2)
    # also next to outputs that need none, and nothing was written
    other = torch.zeros(2, dtype=F64)
    with pytest.raises(RuntimeError, match="needs t"):
        native().row_sums(x, None, None, 1.0, [other, state], [rs.code(WX, ADD), code], 2)
    assert state.tolist() == [4.0, 4.0] and other.tolist() == [0.0, 0.0]
    native().row_sums(x, x, None, 1.0, [state], [code], 2)  # with a target it is served
