"""Normalized DCG on CPU tensors: functional and class API against sklearn.

Oracle: ``sklearn.metrics.ndcg_score`` (``ignore_ties=False``) in FP64, called per row.  The
scores handed to sklearn are the dense ranks from ``np.unique(row, return_inverse=True)``, which
keep the order and the ties of the row and spell out the order docs/parity.md defines for special
values: ``np.unique`` merges the NaNs and sorts them last, and merges ``-0.0`` with ``+0.0``.  For
``exponential_gain`` sklearn gets ``2^t - 1`` as ``y_true``; the relevance levels are the integers
0..4, so that is exact.  sklearn refuses ``C == 1``; that expectation is written by hand.

Tolerance: ``|got - float32(oracle)| <= 2^-23``.  Both sides compute in FP64 (error ~1e-15), each
rounds once to float32, and the values are at most 1, where float32 spacing is 2^-24: the two
roundings can land on neighbouring float32 values, never further apart.
"""

import functools
import math

import numpy as np
import pytest
import torch
from sklearn.metrics import ndcg_score

import torcheval_amd.metrics as M
import torcheval_amd.metrics.functional as MF
import torcheval_amd.metrics.functional.ranking as MFR
import torcheval_amd.metrics.ranking as MR
import torcheval_amd.ops as ops
from torcheval_amd.metrics import NormalizedDCG
from torcheval_amd.metrics.functional import normalized_dcg
from torcheval_amd.utils.test_utils import MetricClassTester
from torcheval_amd.utils.test_utils.dist_pool import run_distributed

TOL = 2.0**-23
KS = (None, 1, 2, 10, "C", "C+5")


def cutoff(k, c):
    """The parameter grid's k for a row width: None, a number, C or C + 5."""
    return c if k == "C" else c + 5 if k == "C+5" else k


# ----------------------------------------------------------------------------- oracle
def oracle(x: torch.Tensor, t: torch.Tensor, k=None, exponential_gain=False) -> np.ndarray:
    """FP64 NDCG@k per row of CPU tensors (any dtype), from sklearn."""
    xs, ts = x.double().numpy(), t.double().numpy()
    gains = np.exp2(ts) - 1.0 if exponential_gain else ts
    out = np.empty(xs.shape[0])
    for i in range(xs.shape[0]):
        if xs.shape[1] == 1:  # sklearn refuses one document: the item is the ideal list
            out[i] = 1.0 if gains[i, 0] > 0 else 0.0
            continue
        ranks = np.unique(xs[i], return_inverse=True)[1].reshape(-1).astype(np.float64)
        out[i] = ndcg_score(gains[i][None], ranks[None], k=k)
    return out


def rows(n: int, c: int, levels, seed: int):
    """(scores float32 [n, c], relevance int64 [n, c] in 0..4); ``levels`` score levels make
    tie groups that straddle the cutoffs, ``None`` gives continuous scores."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, 5, (n, c), generator=g)
    if levels is None:
        return torch.randn(n, c, generator=g), t
    return torch.randint(0, levels, (n, c), generator=g).float() / levels - 0.25, t


@functools.lru_cache(maxsize=None)
def _case(n, c, levels, seed):
    return rows(n, c, levels, seed)


def check(got, x, t, k=None, exponential_gain=False):
    want = oracle(x, t, k, exponential_gain)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    err = np.abs(got.double().cpu().numpy() - want.astype(np.float32).astype(np.float64))
    assert float(err.max(initial=0.0)) <= TOL, (float(err.max()), int(err.argmax()))


# ----------------------------------------------------------------------------- functional
@pytest.mark.parametrize("levels", [2, 5, None])
@pytest.mark.parametrize("c", [1, 2, 3, 63, 64, 65, 257])
def test_functional_against_sklearn(c, levels):
    x, t = _case(6, c, levels, 100 + c)
    for k in KS:
        kk = cutoff(k, c)
        check(normalized_dcg(x, t, k=kk), x, t, kk)
    check(normalized_dcg(x, t, k=2, exponential_gain=True), x, t, 2, True)
    check(normalized_dcg(x, t, exponential_gain=True), x, t, None, True)


def test_one_column_is_defined():
    x = torch.tensor([[0.3], [0.1], [math.nan]])
    t = torch.tensor([[2], [0], [1]])
    assert normalized_dcg(x, t).tolist() == [1.0, 0.0, 1.0]
    assert normalized_dcg(x, t, k=3, exponential_gain=True).tolist() == [1.0, 0.0, 1.0]


def test_value_written_out_by_hand():
    """Scores [.5, .5, .5, .1]: three items tie for positions 0..2, of which k = 2 count, so each
    carries (d0 + d1) / 3 = (1 + 1 / log2(3)) / 3; DCG = (3 + 2 + 0) (1 + 1 / log2 3) / 3, the ideal
    list 3, 2 gives IDCG = 3 + 2 / log2 3."""
    got = normalized_dcg(torch.tensor([[0.5, 0.5, 0.5, 0.1]]), torch.tensor([[3, 2, 0, 1]]), k=2)
    d1 = 1 / math.log2(3)
    want = (5 * (1 + d1) / 3) / (3 + 2 * d1)
    assert abs(want - 0.6378005) < 5e-8
    assert abs(float(got) - float(np.float32(want))) <= TOL


def test_all_equal_scores_and_all_zero_relevance():
    t = torch.tensor([[3, 0, 1, 2, 2], [0, 0, 0, 0, 0]])
    x = torch.full((2, 5), 0.25)
    for k in (None, 1, 3):
        got = normalized_dcg(x, t, k=k)
        check(got, x, t, k)
        assert float(got[1]) == 0.0
    # every item shares all positions: DCG = mean(gain) * D[K]
    kk = 3
    d = [1 / math.log2(r + 2) for r in range(kk)]
    want = (8 / 5) * sum(d) / (3 * d[0] + 2 * d[1] + 2 * d[2])
    assert abs(float(normalized_dcg(x, t, k=kk)[0]) - float(np.float32(want))) <= TOL


@pytest.mark.parametrize("c", [5, 64, 130])
def test_special_value_scores(c):
    specials = torch.tensor([math.nan, -math.nan, 0.0, -0.0, math.inf, -math.inf, 1.5, -1.5])
    g = torch.Generator().manual_seed(7 + c)
    x = specials[torch.randint(0, len(specials), (8, c), generator=g)]
    t = torch.randint(0, 5, (8, c), generator=g)
    for k in (None, 1, 2, 10):
        check(normalized_dcg(x, t, k=k), x, t, k)
    # NaN ranks above +inf, all NaNs tie, the zeros tie
    x3 = torch.tensor([[math.inf, math.nan, 1.0], [0.0, -0.0, -1.0]])
    t3 = torch.tensor([[0, 3, 1], [2, 0, 1]])
    got = normalized_dcg(x3, t3, k=1)
    assert float(got[0]) == 1.0
    assert abs(float(got[1]) - float(np.float32(0.5))) <= TOL  # (2 + 0) / 2 of d0, ideal 2 d0


@pytest.mark.parametrize("score_dtype", [torch.float32, torch.float16, torch.bfloat16, torch.float64])
@pytest.mark.parametrize("rel_dtype", [torch.float32, torch.int64, torch.uint8, torch.float64])
def test_dtypes(score_dtype, rel_dtype):
    x, t = _case(5, 37, 5, 11)
    xq, tq = x.to(score_dtype), t.to(rel_dtype)
    check(normalized_dcg(xq, tq, k=10), xq, tq, 10)


def test_fractional_relevance():
    g = torch.Generator().manual_seed(12)
    x, t = torch.randn(6, 40, generator=g), torch.rand(6, 40, generator=g) * 3
    for k in (None, 5):
        check(normalized_dcg(x, t, k=k), x, t, k)


def test_column_permutation_is_bit_identical():
    g = torch.Generator().manual_seed(13)
    for levels in (2, 5, None):
        x, _ = rows(7, 65, levels, 13)
        t = torch.rand(7, 65, generator=g) * 4  # fractional gains: sums that could depend on the order
        perm = torch.randperm(65, generator=g)
        for k in (None, 2, 10):
            a = normalized_dcg(x, t, k=k)
            b = normalized_dcg(x[:, perm], t[:, perm], k=k)
            assert torch.equal(a, b)


def test_views_with_row_strides():
    x, t = _case(6, 65, 5, 14)
    bx, bt = torch.zeros(6, 69), torch.zeros(6, 69, dtype=torch.int64)
    bx[:, 1:66], bt[:, 1:66] = x, t
    vx, vt = bx[:, 1:66], bt[:, 1:66]
    assert not vx.is_contiguous()
    assert torch.equal(normalized_dcg(vx, vt, k=10), normalized_dcg(x, t, k=10))
    assert torch.equal(normalized_dcg(x.t().contiguous().t(), t, k=10), normalized_dcg(x, t, k=10))


# ----------------------------------------------------------------------------- validation
def test_invalid_arguments():
    x, t = torch.rand(4, 6), torch.randint(0, 3, (4, 6))
    with pytest.raises(ValueError, match="two-dimensional"):
        normalized_dcg(x[0], t[0])
    with pytest.raises(ValueError, match="two-dimensional"):
        normalized_dcg(x[None], t[None])
    with pytest.raises(ValueError, match="same shape"):
        normalized_dcg(x, t[:, :5])
    for k in (0, -3):
        with pytest.raises(ValueError, match=f"k should be None or positive, got {k}."):
            normalized_dcg(x, t, k=k)
        with pytest.raises(ValueError, match=f"k should be None or positive, got {k}."):
            NormalizedDCG(k=k)
    with pytest.raises(ValueError, match="same shape"):
        NormalizedDCG().update(x, t[:3])


def test_negative_and_nan_relevance_raise():
    x = torch.rand(3, 5)
    neg = torch.tensor([[1, 0, 2, 0, 1], [0, -1, 2, 0, 1], [1, 0, 2, 0, 1]])
    nan = neg.float().clamp(min=0)
    nan[2, 4] = math.nan
    for t in (neg, neg.float(), nan):
        with pytest.raises(ValueError, match="NDCG.*negative or NaN relevance"):
            normalized_dcg(x, t)
        m = NormalizedDCG().update(x[:1], neg[:1])
        with pytest.raises(ValueError, match="NDCG.*negative or NaN relevance"):
            m.update(x, t)
        assert float(m.num_rows) == 1.0  # the refused batch left the states alone
        check(m.compute().reshape(1), x[:1], neg[:1])
    assert normalized_dcg(x, torch.tensor(-0.0).expand(3, 5)).tolist() == [0.0, 0.0, 0.0]  # -0.0 is not negative


def test_empty_inputs():
    out = normalized_dcg(torch.rand(0, 7), torch.zeros(0, 7))
    assert out.shape == (0,) and out.dtype == torch.float32
    out = normalized_dcg(torch.rand(3, 0), torch.zeros(3, 0), k=2)
    assert out.dtype == torch.float32 and out.tolist() == [0.0, 0.0, 0.0]
    m = NormalizedDCG().update(torch.rand(0, 7), torch.zeros(0, 7))
    assert float(m.num_rows) == 0.0 and m.compute().isnan()
    m.update(torch.rand(3, 0), torch.zeros(3, 0))
    assert float(m.num_rows) == 3.0 and float(m.compute()) == 0.0


# ----------------------------------------------------------------------------- class protocol
class TestNormalizedDCG(MetricClassTester):
    def test_class_suite(self) -> None:
        x, t = _case(8 * 4, 12, 5, 15)
        want = torch.tensor(oracle(x, t, 5).mean()).float()
        self.run_class_implementation_tests(
            metric=NormalizedDCG(k=5),
            state_names={"ndcg_sum", "num_rows"},
            update_kwargs={"input": x.reshape(8, 4, 12), "target": t.reshape(8, 4, 12)},
            compute_result=want,
            atol=TOL,
            rtol=0,
        )

    def test_class_suite_exponential_gain(self) -> None:
        x, t = _case(8 * 4, 12, 5, 15)
        want = torch.tensor(oracle(x, t, None, True).mean()).float()
        self.run_class_implementation_tests(
            metric=NormalizedDCG(exponential_gain=True),
            state_names={"ndcg_sum", "num_rows"},
            update_kwargs={"input": x.reshape(8, 4, 12), "target": t.reshape(8, 4, 12)},
            compute_result=want,
            atol=TOL,
            rtol=0,
        )


def test_mean_over_four_updates_equals_the_functional():
    x, t = _case(22, 65, 5, 16)
    m = NormalizedDCG(k=10)
    assert m.compute().isnan()
    for lo, hi in ((0, 1), (1, 9), (9, 10), (10, 22)):
        m.update(x[lo:hi], t[lo:hi])
    assert m.ndcg_sum.dtype == torch.float64 and m.num_rows.dtype == torch.float64
    assert float(m.num_rows) == 22.0
    got = m.compute()
    assert got.dtype == torch.float32 and got.shape == ()
    want = oracle(x, t, 10)
    assert abs(float(m.ndcg_sum) - want.sum()) <= 22 * 2.0**-50
    assert abs(float(got) - float(np.float32(want.mean()))) <= TOL
    assert abs(float(got) - float(normalized_dcg(x, t, k=10).double().mean())) <= 2 * TOL


def test_merge_reset_state_dict():
    x, t = _case(9, 20, 2, 17)
    a = NormalizedDCG(k=3).update(x[:4], t[:4])
    b = NormalizedDCG(k=3).update(x[4:], t[4:])
    a.merge_state([b])
    assert float(a.num_rows) == 9.0 and float(b.num_rows) == 5.0
    want = float(np.float32(oracle(x, t, 3).mean()))
    assert abs(float(a.compute()) - want) <= TOL
    c = NormalizedDCG(k=3)
    c.load_state_dict(a.state_dict())
    assert torch.equal(c.compute(), a.compute())
    a.reset()
    assert float(a.ndcg_sum) == 0.0 and float(a.num_rows) == 0.0 and a.compute().isnan()
    a.update(x, t)
    assert abs(float(a.compute()) - want) <= TOL


def _sync_job(rank: int, ws: int):
    from torcheval_amd.metrics.toolkit import sync_and_compute

    x, t = rows(9, 20, 5, 18)
    lo, hi = (0, 4) if rank == 0 else (4, 9)
    return sync_and_compute(NormalizedDCG(k=4).update(x[lo:hi], t[lo:hi]))


def test_two_rank_sync_and_compute():
    x, t = rows(9, 20, 5, 18)
    results = run_distributed(_sync_job, 2)
    assert results[0] is not None  # rank 0 is the recipient
    want = float(np.float32(oracle(x, t, 4).mean()))
    for got in results:
        if got is not None:
            assert abs(float(got) - want) <= TOL


# ----------------------------------------------------------------------------- exports, routing
def test_exports():
    for mod in (M, MR):
        assert mod.NormalizedDCG is NormalizedDCG
    for mod in (MF, MFR):
        assert mod.normalized_dcg is normalized_dcg
    assert "NormalizedDCG" in MR.__all__ and "normalized_dcg" in MFR.__all__
    # the top-level lists mirror the reference's public names, which have no NDCG
    assert "NormalizedDCG" not in M.__all__ and "normalized_dcg" not in MF.__all__


@pytest.mark.skipif(not ops.native_loaded(), reason="extension not built")
def test_wrapper_routes_to_the_dispatcher_op_when_compiling(monkeypatch):
    from torcheval_amd.ops import ndcg as K

    monkeypatch.setattr(ops, "compiling", lambda: True)
    meta = torch.device("meta")
    x, t = torch.empty(4, 9, device=meta), torch.empty(4, 9, dtype=torch.int64, device=meta)
    out = torch.empty(4, device=meta)
    s, n = torch.empty((), dtype=torch.float64, device=meta), torch.empty((), dtype=torch.float64, device=meta)
    err = torch.empty(1, dtype=torch.int32, device=meta)
    K.ndcg(x, t, 3, False, out)
    K.ndcg(x, t, 9, True, None, s, n, err)
    schema = str(torch.ops.torcheval_amd.ndcg.default._schema)
    for part in ("Tensor(a!)? out", "Tensor(b!)? ndcg_sum", "Tensor(c!)? num_rows", "Tensor(d!)? err"):
        assert part in schema
    assert K.max_columns() >= 64
