"""The CPU side of tests/gpu/test_k2_multilabel.py: the oracle of tests/_k2_cases.py against the
project's ATen chain where ATen is defined (no tie at rank k), and the conditions that give the
GPU fixtures their teeth.  The conditions are asserted, not measured: a fixture that stops telling
the top-k rule from the signed-zero model or from the highest-index model fails here.
"""

import functools

import pytest
import torch

from tests._k2_cases import (
    FIXTURES,
    N_ROWS,
    SCALAR_C,
    SCORE_DTYPES,
    VEC_C,
    VIEW_C,
    all_counts,
    boundary_tied,
    fixture,
    highest_index_model_pred,
    k2_targets,
    ks_for,
    odd_targets,
    signed_zero_model_pred,
    tie_free_rows,
    topk_pred,
    total,
)
from tests._threshold_edges import CRITERIA, dtype_id
from torcheval_amd.metrics.functional.classification.accuracy import _multilabel_update

_dt_ids = dict(ids=dtype_id)
ALL_C = tuple(sorted(set(SCALAR_C + VIEW_C + VEC_C)))


# ------------------------------------------------------------------ the oracle where ATen is defined
@pytest.mark.parametrize("c", [1, 3, 4, 64, 65, 256, 257, 260, 1000, 1024, 1028, 2047, 2048])
@pytest.mark.parametrize("dtype", SCORE_DTYPES, **_dt_ids)
def test_tie_free_oracle_matches_aten_chain(dtype, c):
    x = tie_free_rows(dtype, N_ROWS, c, seed=c)
    srt = torch.sort(x.double(), dim=1).values
    assert not (srt[:, 1:] == srt[:, :-1]).any(), "rows must be distinct"
    assert int(x.isnan().sum()) == 1 and int(x.isinf().sum()) == (2 if N_ROWS > 3 else 0)
    for k in sorted({min(k, c) for k in (1, 2, 5, c)}):
        pred = topk_pred(x, k)
        assert torch.equal(pred.sum(dim=1), torch.full((N_ROWS,), k))
        aten = torch.zeros(x.size()).scatter_(-1, x.topk(k=k, dim=-1).indices, 1.0)
        assert torch.equal(pred, aten.long()), f"k={k}: the rule and ATen's topk differ without a tie"
        t = k2_targets(pred, seed=c + k)
        for crit, want in all_counts(pred, t).items():
            got, tot = _multilabel_update(aten, t, crit)
            assert (int(got), int(tot)) == (want, total(t, crit)), f"k={k} {crit}"


def test_rule_on_the_documented_rows():
    x = torch.tensor([[-0.0, 0.0], [0.0, -0.0]])
    assert topk_pred(x, 1).tolist() == [[1, 0], [1, 0]]
    assert signed_zero_model_pred(x, 1).tolist() == [[0, 1], [1, 0]]
    assert highest_index_model_pred(x, 1).tolist() == [[0, 1], [0, 1]]
    x = torch.tensor([[0.0, -0.0, 0.0, -0.0, -1.0]])
    assert topk_pred(x, 2).tolist() == [[1, 1, 0, 0, 0]]
    nan, inf = float("nan"), float("inf")
    x = torch.tensor([[inf, -nan, 1.0, nan, inf]])
    assert topk_pred(x, 1).tolist() == [[0, 1, 0, 0, 0]]  # NaNs are equal whatever their sign
    assert topk_pred(x, 3).tolist() == [[1, 1, 0, 1, 0]]  # and rank above +inf


# ------------------------------------------------------------------ conditions on the GPU fixtures
@functools.lru_cache(maxsize=None)
def _case(kind, dtype, c, k):
    x = fixture(kind, dtype, c, k)
    pred = topk_pred(x, k)
    return x, pred, k2_targets(pred, seed=c + k)


def _differing(pred_a, pred_b, t):
    a, b = all_counts(pred_a, t), all_counts(pred_b, t)
    return [crit for crit in CRITERIA if a[crit] != b[crit]]


@pytest.mark.parametrize("c", ALL_C)
@pytest.mark.parametrize("dtype", SCORE_DTYPES, **_dt_ids)
def test_fixture_conditions(dtype, c):
    for k in ks_for(c):
        for kind in FIXTURES:
            x, pred, t = _case(kind, dtype, c, k)
            what = f"{kind} c={c} k={k}"
            assert x.shape == (N_ROWS, c) and x.dtype == dtype
            if kind == "tie_free":
                assert not boundary_tied(x, k).any(), what
            if kind == "tie" and k < c:
                assert 2 * int(boundary_tied(x, k).sum()) >= N_ROWS, what
            # with every label predicted (k == c) no {0, 1} target can break "contain": the
            # prediction does not depend on the scores there, and the other four are checked
            for crit, want in all_counts(pred, t).items():
                assert want < 2**24
                if k < c or crit != "contain":
                    assert 0 < want < total(t, crit), f"{what} {crit}: {want} of {total(t, crit)}"
            if k == c:
                continue  # one possible prediction: no model can differ
            if kind == "special":
                d = _differing(signed_zero_model_pred(x, k), pred, t)
                assert len(d) >= 3, f"{what}: the signed-zero model differs only in {d}"
            if kind in ("tie", "special"):
                d = _differing(highest_index_model_pred(x, k), pred, t)
                assert len(d) >= 3, f"{what}: the highest-index model differs only in {d}"


@pytest.mark.parametrize("tdtype", [torch.float32, torch.int64, torch.int32, torch.uint8], **_dt_ids)
def test_odd_targets_hold_their_values_and_stay_interior(tdtype):
    for c in (256, 257):
        x = fixture("tie", torch.float32, c, 3)
        pred = topk_pred(x, 3)
        t = odd_targets(pred, seed=c, dtype=tdtype)
        assert t.dtype == tdtype
        outside = ~((t == 0) | (t == 1))
        assert int(outside.sum()) > N_ROWS  # NaN counts as outside
        if tdtype == torch.uint8:
            assert int((t == 255).sum()) > 0
        if tdtype == torch.float32:
            assert int(t.isnan().sum()) > 0 and int(((t == 0) & torch.signbit(t)).sum()) > 0
        for crit, want in all_counts(pred, t).items():
            assert 0 < want < total(t, crit), f"c={c} {crit}: {want}"
