"""K13 (csrc/kernels/ndcg.hip) on MI355X: normalized DCG against the sklearn FP64 oracle of
tests/metrics/ranking/test_ndcg.py, under that file's tolerance (2^-23 after both sides round to
float32).  The widths sit at the edges of the two arms (a wave per row up to 64 columns, a
workgroup per row with power-of-two LDS padding above) and of the cap the extension exports;
one column past the cap must agree through the ATen form."""

import functools
import math

import numpy as np
import pytest
import torch

import torcheval_amd.ops as ops
from tests.metrics.ranking.test_ndcg import KS, TOL, check, cutoff, oracle, rows
from torcheval_amd.config import flags
from torcheval_amd.metrics import NormalizedDCG
from torcheval_amd.metrics.functional import normalized_dcg
from torcheval_amd.metrics.functional.ranking.ndcg import _ndcg_update
from torcheval_amd.ops import ndcg as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NS = (1, 5, 37)


def _cap():
    return K.max_columns()


def _widths():
    return (1, 2, 63, 64, 65, 255, 256, 257, 1000, "cap", "cap+1")


def _width(c):
    return _cap() if c == "cap" else _cap() + 1 if c == "cap+1" else c


@functools.lru_cache(maxsize=None)
def _case(n, c, levels, seed):
    """CPU rows of a case, shared by the tests that use it (never modified)."""
    return rows(n, c, levels, seed)


@functools.lru_cache(maxsize=None)
def _want(n, c, levels, seed, k, exponential_gain=False):
    x, t = _case(n, c, levels, seed)
    return oracle(x, t, k, exponential_gain)


def _close(got, want):
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == want.shape
    err = np.abs(got.double().cpu().numpy() - want.astype(np.float32).astype(np.float64))
    assert float(err.max(initial=0.0)) <= TOL, (float(err.max()), int(err.argmax()))


@pytest.fixture
def native_calls(monkeypatch):
    """Counts the launches through the K13 wrapper: the native path really ran."""
    calls = []
    real = K.ndcg

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(K, "ndcg", spy)
    return calls


# ----------------------------------------------------------------------------- shapes and ties
@pytest.mark.parametrize("levels", [2, 5])
@pytest.mark.parametrize("c", _widths())
def test_shapes_ties_and_cutoffs(c, levels, native_calls):
    c = _width(c)
    x, t = _case(37, c, levels, 200 + levels)
    xd, td = x.to(DEV), t.to(DEV)
    native = c <= _cap()
    assert K.supported(xd, td) == native
    for k in KS:
        kk = cutoff(k, c)
        want = _want(37, c, levels, 200 + levels, kk)
        for n in NS:
            _close(normalized_dcg(xd[:n], td[:n], k=kk), want[:n])
    assert len(native_calls) == (len(KS) * len(NS) if native else 0)


@pytest.mark.parametrize("c", [64, 65, 1000])
def test_continuous_scores_and_exponential_gain(c, native_calls):
    x, t = _case(5, c, None, 210)
    xd, td = x.to(DEV), t.to(DEV)
    for k in (None, 10):
        _close(normalized_dcg(xd, td, k=k), _want(5, c, None, 210, k))
        _close(normalized_dcg(xd, td, k=k, exponential_gain=True), _want(5, c, None, 210, k, True))
    assert len(native_calls) == 4


def test_fractional_relevance():
    g = torch.Generator().manual_seed(211)
    for c in (40, 300):
        x, t = torch.randn(6, c, generator=g), torch.rand(6, c, generator=g) * 3
        for k in (None, 5):
            check(normalized_dcg(x.to(DEV), t.to(DEV), k=k), x, t, k)
        check(normalized_dcg(x.to(DEV), t.to(DEV), exponential_gain=True), x, t, None, True)


# ----------------------------------------------------------------------------- dtypes, layouts
@pytest.mark.parametrize("c", [37, 300])
@pytest.mark.parametrize("rel_dtype", [torch.float32, torch.int64, torch.uint8])
@pytest.mark.parametrize("score_dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_dtypes(score_dtype, rel_dtype, c, native_calls):
    x, t = _case(5, c, 5, 220)
    xq, tq = x.to(score_dtype), t.to(rel_dtype)  # the oracle sees the values after the dtype's rounding
    check(normalized_dcg(xq.to(DEV), tq.to(DEV), k=10), xq, tq, 10)
    assert len(native_calls) == 1


@pytest.mark.parametrize("rel_dtype", [torch.int32, torch.int16, torch.int8, torch.float16, torch.bfloat16])
def test_remaining_relevance_dtypes(rel_dtype, native_calls):
    for c in (37, 300):
        x, t = _case(5, c, 5, 220)
        tq = t.to(rel_dtype)
        check(normalized_dcg(x.to(DEV), tq.to(DEV), k=10), x, tq, 10)
    assert len(native_calls) == 2


def test_float64_and_other_dtypes_take_the_aten_form(native_calls):
    x, t = _case(5, 37, 5, 220)
    got = normalized_dcg(x.double().to(DEV), t.to(DEV), k=10)
    assert got.dtype == torch.float32 and got.is_cuda
    check(got, x, t, 10)
    check(normalized_dcg(x.to(DEV), t.double().to(DEV), k=10), x, t, 10)
    check(normalized_dcg(x.to(DEV), (t > 2).to(DEV), k=10), x, (t > 2), 10)
    assert native_calls == []


@pytest.mark.parametrize("score_dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("c", [64, 65, 1000])
def test_views_off_alignment(c, score_dtype, native_calls):
    """Column offset of one element, row stride C + 3: no row starts on a 16-B boundary twice."""
    x, t = _case(5, c, 5, 230)
    xq = x.to(score_dtype)
    bx = torch.full((5, c + 3), 7.0, dtype=score_dtype, device=DEV)
    bt = torch.full((5, c + 3), 9, dtype=torch.int64, device=DEV)
    vx, vt = bx[:, 1 : c + 1], bt[:, 1 : c + 1]
    vx.copy_(xq)
    vt.copy_(t)
    assert not vx.is_contiguous() and vx.stride(0) == c + 3 and vx.data_ptr() % 16 != 0
    assert K.supported(vx, vt)
    for k in (None, 10):
        check(normalized_dcg(vx, vt, k=k), xq, t, k)
    bt8 = torch.full((5, c + 3), 9, dtype=torch.uint8, device=DEV)
    vt8 = bt8[:, 2 : c + 2]
    vt8.copy_(t)
    check(normalized_dcg(vx, vt8, k=10), xq, t, 10)
    assert len(native_calls) == 3


def test_broadcast_rows_and_a_non_unit_column_stride(native_calls):
    x, t = _case(5, 65, 5, 231)
    xd, td = x.to(DEV), t.to(DEV)
    same_scores = xd[:1].expand(5, 65)  # row stride 0
    check(normalized_dcg(same_scores, td, k=10), x[:1].expand(5, 65), t, 10)
    assert len(native_calls) == 1
    wide = torch.zeros(5, 130, device=DEV)
    wide[:, ::2] = xd
    assert not K.supported(wide[:, ::2], td)
    check(normalized_dcg(wide[:, ::2], td, k=10), x, t, 10)
    assert len(native_calls) == 1


# ----------------------------------------------------------------------------- special values
@pytest.mark.parametrize("c", [5, 64, 130, 1000])
def test_special_value_scores(c, native_calls):
    specials = torch.tensor([math.nan, -math.nan, 0.0, -0.0, math.inf, -math.inf, 1.5, -1.5])
    g = torch.Generator().manual_seed(240 + c)
    x = specials[torch.randint(0, len(specials), (8, c), generator=g)]
    t = torch.randint(0, 5, (8, c), generator=g)
    for k in (None, 1, 2, 10):
        check(normalized_dcg(x.to(DEV), t.to(DEV), k=k), x, t, k)
    xh = x.half()
    check(normalized_dcg(xh.to(DEV), t.to(DEV), k=2), xh, t, 2)
    assert len(native_calls) == 5


def test_special_rows():
    for c in (5, 64, 65, 300):
        t = torch.randint(0, 5, (3, c), generator=torch.Generator().manual_seed(c))
        t[1] = 0
        x = torch.full((3, c), 0.25)
        for k in (None, 1, 3):
            got = normalized_dcg(x.to(DEV), t.to(DEV), k=k)
            check(got, x, t, k)
            assert float(got[1]) == 0.0
        perfect = normalized_dcg(t.float().to(DEV), t.to(DEV), k=4)
        assert perfect.tolist() == [1.0, 0.0, 1.0]
    assert normalized_dcg(torch.rand(3, 0, device=DEV), torch.zeros(3, 0, device=DEV)).tolist() == [0.0] * 3
    assert normalized_dcg(torch.rand(0, 9, device=DEV), torch.zeros(0, 9, device=DEV)).shape == (0,)
    one = normalized_dcg(torch.tensor([[0.3], [0.1]], device=DEV), torch.tensor([[2], [0]], device=DEV))
    assert one.tolist() == [1.0, 0.0]


# ----------------------------------------------------------------------------- negative relevance
@pytest.mark.parametrize("c", [8, 64, 65, 300, "cap+1"])
def test_negative_relevance(c):
    c = _width(c)
    x, t = _case(5, c, 5, 250)
    bad = t.clone()
    bad[3, c // 2] = -1
    xd, bd = x.to(DEV), bad.to(DEV)
    got = normalized_dcg(xd, bd, k=10)  # validate is off: no raise, the row scores NaN
    assert got.isnan().tolist() == [False, False, False, True, False]
    keep = [0, 1, 2, 4]
    check(got[keep], x[keep], t[keep], 10)
    nan_rel = t.float()
    nan_rel[0, 0] = math.nan
    assert normalized_dcg(xd, nan_rel.to(DEV), k=10).isnan().tolist() == [True, False, False, False, False]
    with flags(validate=True):
        with pytest.raises(ValueError, match="NDCG.*negative or NaN relevance"):
            normalized_dcg(xd, bd, k=10)
        check(normalized_dcg(xd, t.to(DEV), k=10), x, t, 10)

    m = NormalizedDCG(k=10, device=DEV)
    m.update(xd, t.to(DEV))
    m.update(xd, bd)  # no raise at the update
    with pytest.raises(ValueError, match="NDCG.*negative or NaN relevance"):
        m.compute()
    assert float(m.num_rows) == 10.0  # the flag was cleared, nothing else reset
    assert m.compute().isnan()
    m.reset()
    m.update(xd, t.to(DEV))
    want = float(np.float32(oracle(x, t, 10).mean()))
    assert abs(float(m.compute()) - want) <= TOL


# ----------------------------------------------------------------------------- grid stride
@pytest.mark.parametrize("n,c", [(70000, 8), (20000, 65)])
def test_more_rows_than_the_grid(n, c, native_calls):
    x, t = _case(n, c, 5, 260)
    xd, td = x.to(DEV), t.to(DEV)
    got = normalized_dcg(xd, td, k=3)
    assert len(native_calls) == 1
    want, bad = _ndcg_update(xd, td, 3, False)  # the ATen form on the same device
    assert not bool(bad.any())
    assert float((got.double() - want.float().double()).abs().max()) <= TOL
    tail = slice(n - 7, n)
    check(got[tail], x[tail], t[tail], 3)
    m = NormalizedDCG(k=3, device=DEV).update(xd, td)
    assert float(m.num_rows) == float(n)
    # 2^-50 per row, the budget of test_class_states; plus the roundings of running sums <= n, each
    # at most n 2^-53: no more than 64 lie between a row value and either total (a wave adds
    # n / 8192 + 1 rows, then 4 waves, 8 partials per finish thread, a 6-step butterfly and 4 waves;
    # torch.sum is a tree of similar depth)
    assert abs(float(m.ndcg_sum) - float(want.sum())) <= n * 2.0**-50 + 64 * n * 2.0**-53
    assert abs(float(m.compute()) - float(want.mean().float())) <= TOL


# ----------------------------------------------------------------------------- determinism, class
def test_two_runs_are_bit_identical():
    for c in (37, 300):
        x, t = _case(37, c, 5, 270)
        xd, td = x.to(DEV), t.to(DEV)
        assert torch.equal(normalized_dcg(xd, td, k=10), normalized_dcg(xd, td, k=10))
        a, b = NormalizedDCG(k=10, device=DEV), NormalizedDCG(k=10, device=DEV)
        for lo, hi in ((0, 5), (5, 36), (36, 37)):
            a.update(xd[lo:hi], td[lo:hi])
            b.update(xd[lo:hi], td[lo:hi])
        assert torch.equal(a.ndcg_sum, b.ndcg_sum) and torch.equal(a.num_rows, b.num_rows)
        assert float(a.num_rows) == 37.0


@pytest.mark.parametrize("c", [37, 300])
def test_class_states(c, native_calls):
    from torcheval_amd.parallel.state_buffer import buffer_of

    x, t = _case(43, c, 5, 280)
    m = NormalizedDCG(k=10, device=DEV)
    sb = buffer_of(m)
    assert sb is not None
    ptrs = (m.ndcg_sum.data_ptr(), m.num_rows.data_ptr())
    for lo, hi in ((0, 5), (5, 42), (42, 43)):
        m.update(x[lo:hi].to(DEV), t[lo:hi].to(DEV))
    assert len(native_calls) == 3
    assert buffer_of(m, build=False) is sb and (m.ndcg_sum.data_ptr(), m.num_rows.data_ptr()) == ptrs
    assert m.ndcg_sum.dtype == torch.float64 and m.num_rows.dtype == torch.float64
    assert float(m.num_rows) == 43.0
    want = oracle(x, t, 10)
    assert abs(float(m.ndcg_sum) - float(want.sum())) <= 43 * 2.0**-50
    got = m.compute()
    assert got.dtype == torch.float32 and got.is_cuda and got.shape == ()
    assert abs(float(got) - float(np.float32(want.mean()))) <= TOL
    moved = m.to("cpu")
    assert moved.ndcg_sum.device.type == "cpu"
    assert abs(float(moved.compute()) - float(np.float32(want.mean()))) <= TOL
    m.reset()
    assert float(m.num_rows) == 0.0 and m.compute().isnan()


def test_class_merge_state_and_aten_cross_check(monkeypatch):
    x, t = _case(43, 300, 5, 280)
    xd, td = x.to(DEV), t.to(DEV)
    a = NormalizedDCG(device=DEV).update(xd[:10], td[:10])
    b = NormalizedDCG(device=DEV).update(xd[10:], td[10:])
    a.merge_state([b])
    assert float(a.num_rows) == 43.0 and float(b.num_rows) == 33.0
    want = float(np.float32(oracle(x, t).mean()))
    assert abs(float(a.compute()) - want) <= TOL
    native = normalized_dcg(xd, td)
    monkeypatch.setattr(ops, "DISABLE_HIP", True)

    def no_kernel(*a, **k):
        raise AssertionError("K13 launched with TORCHEVAL_AMD_DISABLE_HIP set")

    monkeypatch.setattr(K, "ndcg", no_kernel)
    aten = normalized_dcg(xd, td)
    assert aten.is_cuda
    check(aten, x, t)
    check(native, x, t)
    m = NormalizedDCG(device=DEV).update(xd, td)
    assert abs(float(m.compute()) - want) <= TOL


# ----------------------------------------------------------------------------- dispatcher
def _loop_data(i, c):
    g = torch.Generator(device=DEV).manual_seed(400 + i)
    x = torch.randint(0, 5, (256, c), device=DEV, generator=g).float()
    return x, torch.randint(0, 5, (256, c), device=DEV, generator=g)


@pytest.mark.parametrize("c", [32, 300])
def test_compiled_update_loop_matches_eager(c):
    eager, comp = NormalizedDCG(k=10, device=DEV), NormalizedDCG(k=10, device=DEV)
    torch._dynamo.reset()

    @torch.compile(fullgraph=True)
    def step(*args):
        comp.update(*args)

    for i in range(4):
        args = _loop_data(i, c)
        eager.update(*args)
        step(*args)
    assert torch.equal(comp.ndcg_sum, eager.ndcg_sum) and float(comp.num_rows) == 1024.0
    torch.testing.assert_close(comp.compute(), eager.compute(), rtol=0, atol=0)


def test_compiled_graph_holds_the_dispatcher_op():
    m = NormalizedDCG(device=DEV)
    seen = []

    def backend(gm, example_inputs):
        seen.extend(str(n.target) for n in gm.graph.nodes if n.op == "call_function")
        return gm

    torch._dynamo.reset()
    step = torch.compile(lambda x, y: m.update(x, y), backend=backend, fullgraph=True)
    x, t = _loop_data(0, 32)
    step(x, t)
    assert any("torcheval_amd.ndcg" in s for s in seen), seen
    want = float(np.float32(oracle(x.cpu(), t.cpu()).mean()))
    assert abs(float(m.compute()) - want) <= TOL
