"""K5b (csrc/kernels/rowsums.hip): every dispatch arm, called directly, against the float64 oracle
of tests/_rowsums_oracle.py.

The cases, the two data families and the launch geometry are in tests/_rowsums_cases.py.  The exact
family (small integers and half-integers: every FP64 partial sum is exact in any order) must match
the oracle bit for bit, so one element dropped, counted twice or read from the wrong place fails
whatever the row length; the float family is held to the worst-case reordering error of two FP64
summations.  The host twin runs the same comparison in tests/metrics/test_rowsums_oracle.py.

TORCHEVAL_AMD_K5B_GRID is read on every call and set per case; TORCHEVAL_AMD_K5B_MODE is read once
per process, so modes 1 and 2 run in one child process each.
"""

import json
import os
import subprocess
import sys

import pytest
import torch

from tests import _rowsums_cases as C
from tests._rowsums_oracle import ADD, COUNT, SET, W, WX

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _hold(cases, repeat=1):
    assert cases
    bad = C.run_cases(cases, DEV, repeat)
    assert not bad, (len(bad), bad[:8])


def test_this_process_runs_the_default_mode():
    assert C.process_mode() == 0 and C.GRID_ENV not in os.environ


def test_restated_geometry():
    """The block counts the cases below are built for, from the restated formulas."""
    assert C.geometry(0, 1, 32768) == (1, 0) and C.geometry(0, 1, 32769) == (9, 0)
    assert C.geometry(0, 1, 36865, 2) == (2, 0)
    assert C.geometry(0, 1, 32769, 4) == (4, 1)  # 9 chunks over 4 blocks of 3: the fourth holds nothing
    assert C.geometry(0, 2, C.N_66) == (66, 0)
    assert C.geometry(0, 1, C.N_1026, 2000) == (1026, 0) and C.N_1026 < 4_200_000
    assert C.geometry(2, 1, C.N_514, 2000) == (514, 0) and C.N_514 < 4_300_000
    assert C.geometry(1, 1, 32769) == (3, 0) and C.geometry(1, 3, 65537) == (5, 0)
    assert C.geometry(2, 1, 32769) == (5, 0) and C.geometry(2, 3, 65537) == (9, 0)


# ---------------------------------------------------------------- one block per row
@pytest.mark.parametrize("set_name", list(C.NAMED_SETS) + list(C.GENERIC_SETS))
def test_single_block_vector_path(set_name):
    cases = C.single_cases(set_name)
    assert {c.n for c in cases} == set(C.N_SINGLE) and {c.rows for c in cases} == {1, 3}
    assert {c.weight == "tensor" for c in cases} == {True, False}
    _hold(cases)


def test_vector_path_at_every_4_byte_alignment():
    cases = C.alignment_cases()
    assert {c.offsets for c in cases} == {(1, 2, 3), (2, 3, 1), (3, 1, 2)} and {c.n for c in cases} == {4097, 32769}
    _hold(cases)


def test_generic_path_dtypes_and_strides():
    cases = C.generic_cases()
    assert {c.x_dtype for c in cases} == set(C.GENERIC_DTYPES) | {torch.float32}
    assert {C.geometry(0, c.rows, c.n)[0] for c in cases} == {1, 10}
    _hold(cases)


@pytest.mark.parametrize("stats", [(W,), (COUNT,), (WX, W, COUNT)], ids=["w", "count", "wx_w_count"])
def test_sets_that_read_no_target_run_without_one(stats):
    """{W} and {COUNT} take the generic instantiation, which must not touch the absent target."""
    _hold([C.Case(f"no-target-n{n}-{weight}", "exact", 2, n, C.outs_for(stats, "a"), weight=weight, has_t=False)
           for n in (4097, 36865) for weight in ("tensor", 3.0)])


# ---------------------------------------------------------------- two launches
def test_grid_and_combine_one_row():
    cases = C.combine_cases()
    assert {c.blocks for c in cases} >= {2, 4, 1026} and any(c.empty == 1 for c in cases)
    _hold(cases)


def test_grid_and_combine_rows():
    cases = C.combine_rows_cases()
    assert {c.rows for c in cases} == {2, 3, 4, 5} and {c.blocks for c in cases} == {10, 66}
    _hold(cases)


# ---------------------------------------------------------------- extrema
@pytest.mark.parametrize("kind", ["nan", "min", "max"])
def test_special_target_at_every_place(kind):
    cases = C.extrema_cases(kind)
    assert {w for c in cases for w in [c.id.split("-")[5]]} >= {"first", "whole_chunk", "masked_chunk", "tail",
                                                                 "last_block_chunk", "last_block_tail"}
    for c in cases:  # what the oracle says of them: the value is not lost in the family's other targets
        sse, tmin, tmax, _, rng = C.expected_states(c, *C.values(c))
        last = c.rows - 1
        if kind == "nan":
            assert all(bool(torch.isnan(v.reshape(-1)[last])) for v in (sse, tmin, tmax, rng)), c.id
        elif kind == "min":
            assert float(tmin[last]) == -100.0, c.id
        else:
            assert float(tmax[last]) == 100.0, c.id
    _hold(cases)


# ---------------------------------------------------------------- deferred mode
@pytest.mark.parametrize("case", C.pend_cases(), ids=lambda c: c.id)
def test_deferred_updates_fold_together(case):
    bad = C.run_pend(case, DEV)
    assert not bad, bad[:8]


@pytest.mark.parametrize("n", [0, 1000, 32768, 36865])
def test_deferred_mode_declines(n):
    """row_sums_pend returns 0 and launches nothing for rows of one block, for empty rows, and
    (n = 36865) for an output that a fold could not add: a SET sum."""
    x = torch.ones(2, n, device=DEV)
    pend = torch.zeros(2 * C.PEND_STATS * C.PEND_BLOCKS, dtype=torch.float64, device=DEV)
    state = torch.full((2,), 4.0, dtype=torch.float64, device=DEV)
    op = SET if n == 36865 else ADD
    assert C.native().row_sums_pend(x, None, None, 1.0, [state], [WX * 8 + op], 2, pend) == 0
    assert state.tolist() == [4.0, 4.0] and int((pend != 0).sum()) == 0
    if n == 36865:  # the same call with an ADD output is taken
        assert C.native().row_sums_pend(x, None, None, 1.0, [state], [WX * 8 + ADD], 2, pend) == 10
        C.native().row_sums_fold(pend, 10, [state], [WX * 8 + ADD], 2)
        assert state.tolist() == [36869.0, 36869.0] and int((pend != 0).sum()) == 0


# ---------------------------------------------------------------- FP64 accumulation
@pytest.mark.parametrize("arm", ["single", "combine", "combine_rows", "pend"])
def test_float_family_within_the_derived_bound(arm):
    if arm == "pend":
        bad = C.run_pend(C.pend_float_case(), DEV)
        assert not bad, bad[:8]
        return
    cases = {"single": lambda: C.single_cases("all", "float"), "combine": lambda: C.combine_cases("float"),
             "combine_rows": lambda: C.combine_rows_cases("float")}[arm]()
    assert all(c.family == "float" for c in cases)
    _hold(cases)


# ---------------------------------------------------------------- modes 1 and 2
@pytest.mark.parametrize("mode", [1, 2])
def test_one_launch_modes(mode):
    """The fat-block fold (release fence and ticket) and the write-through partials with the
    last-block combine, each in a fresh child process; every case runs twice on one stream."""
    env = dict(os.environ, **{C.MODE_ENV: str(mode)})
    env.pop(C.GRID_ENV, None)
    child = f"from tests import _rowsums_cases as C; C.child_main({mode})"
    r = subprocess.run([sys.executable, "-c", child], env=env, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["mode"] == mode and res["cases"] == len(C.mode_cases(mode)) >= 32
    assert res["failures"] == [], (len(res["failures"]), res["failures"][:8])
