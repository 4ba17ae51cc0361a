"""Kendall rank correlation on CPU tensors: functional and class API against scipy.

Oracle: ``scipy.stats.kendalltau(variant=...)`` in FP64, called per task on the values the metric
sees (a float16 / bfloat16 operand is widened after rounding, so the oracle sees the same ties),
with its warnings silenced.

Tolerance: ``|got - float32(oracle)| <= 2^-23``.  Both sides evaluate one FP64 expression of exact
integers (error of the order of 1e-16) and round once to float32; ``|tau| <= 1``, where float32
spacing is at most 2^-23 ... 2^-24, so the two roundings can land on neighbouring float32 values,
never further apart.  Float64 results are held to 2^-50.  NaN must match NaN.

The six integers of ``_kendall_counts`` are compared exactly with a plain O(n^2) count.
"""

import functools
import warnings

import numpy as np
import pytest
import torch
from scipy import stats

import torcheval_amd.metrics as M
import torcheval_amd.metrics.functional as MF
import torcheval_amd.metrics.functional.regression as MFR
import torcheval_amd.metrics.regression as MR
import torcheval_amd.ops as ops
from torcheval_amd.metrics import KendallRankCorrCoef
from torcheval_amd.metrics.functional import kendall_rank_corrcoef
from torcheval_amd.metrics.functional.regression.kendall import _kendall_counts
from torcheval_amd.utils.test_utils import MetricClassTester

TOL = 2.0**-23
SIZES = (2, 3, 64, 65, 2049)
VARIANTS = ("b", "c")


# ----------------------------------------------------------------------------- oracles
def oracle(x: torch.Tensor, y: torch.Tensor, variant: str) -> np.ndarray:
    """FP64 tau per task of CPU tensors (any dtype): ``[tasks]``, or 0-d for 1-D operands."""
    xs, ys = x.double().numpy(), y.double().numpy()
    flat = xs.ndim == 1
    xs, ys = np.atleast_2d(xs), np.atleast_2d(ys)
    out = np.full(xs.shape[0], np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in range(xs.shape[0]):
            if xs.shape[1] >= 2:
                out[i] = stats.kendalltau(xs[i], ys[i], variant=variant).statistic
    return out[0] if flat else out


def check(got: torch.Tensor, x: torch.Tensor, y: torch.Tensor, variant: str, dtype=torch.float32):
    want = np.asarray(oracle(x.cpu(), y.cpu(), variant))
    assert got.dtype == dtype and tuple(got.shape) == want.shape
    g = got.double().cpu().numpy()
    assert np.array_equal(np.isnan(g), np.isnan(want)), (g, want)
    if dtype == torch.float32:
        want, tol = want.astype(np.float32).astype(np.float64), TOL
    else:
        tol = 2.0**-50
    err = np.abs(g - want)[~np.isnan(want)]
    assert float(err.max(initial=0.0)) <= tol, float(err.max())


def both(x, y, tasks=1, dtype=torch.float32):
    for variant in VARIANTS:
        check(kendall_rank_corrcoef(x, y, num_tasks=tasks, variant=variant), x, y, variant, dtype)


def plain_counts(x: torch.Tensor, y: torch.Tensor):
    """(n1, n2, n3, Q, mx, my) of 1-D operands by comparing every pair."""
    xs, ys = x.double().numpy(), y.double().numpy()
    i, j = np.triu_indices(len(xs), 1)
    dx, dy = np.sign(xs[i] - xs[j]), np.sign(ys[i] - ys[j])
    return [int((dx == 0).sum()), int((dy == 0).sum()), int(((dx == 0) & (dy == 0)).sum()),
            int((dx * dy < 0).sum()), len(np.unique(xs)), len(np.unique(ys))]


@functools.lru_cache(maxsize=None)
def pair(n: int, levels, seed: int, tasks: int = 1):
    """Correlated float32 operands ``[n]`` (or ``[tasks, n]``); ``levels`` rounds both to that many
    distinct values (heavy ties), ``None`` leaves them continuous."""
    g = torch.Generator().manual_seed(seed)
    shape = (n,) if tasks == 1 else (tasks, n)
    x = torch.rand(shape, generator=g)
    y = 0.6 * x + 0.4 * torch.rand(shape, generator=g)
    if levels is not None:
        x, y = torch.floor(x * levels), torch.floor(y * levels)
    return x, y


# ----------------------------------------------------------------------------- functional
@pytest.mark.parametrize("tasks", [1, 3])
@pytest.mark.parametrize("levels", [None, 50, 3])
@pytest.mark.parametrize("n", SIZES)
def test_matches_scipy(n, levels, tasks):
    x, y = pair(n, levels, 100 + n, tasks)
    both(x, y, tasks)


@pytest.mark.parametrize("levels", [None, 50, 3, 1])
@pytest.mark.parametrize("n", [2, 3, 64, 65, 300])
def test_counts_equal_a_plain_pair_count(n, levels):
    x, y = pair(n, levels, 200 + n, 3)
    got = _kendall_counts(x, y)
    assert got.dtype == torch.int64 and got.shape == (3, 6)
    for t in range(3):
        assert got[t].tolist() == plain_counts(x[t], y[t])
    assert _kendall_counts(x[0], y[0]).tolist() == [plain_counts(x[0], y[0])]
    # the operands' roles: n1 / mx belong to input, n2 / my to target
    swapped = _kendall_counts(y, x)
    assert torch.equal(swapped, got[:, [1, 0, 2, 3, 5, 4]])


@pytest.mark.parametrize("n", SIZES)
def test_constant_operand_is_nan(n):
    x, _ = pair(n, None, 7)
    const = torch.full((n,), 2.5)
    for variant in VARIANTS:
        for a, b in ((const, x), (x, const), (const, const)):
            assert kendall_rank_corrcoef(a, b, variant=variant).isnan()
            check(kendall_rank_corrcoef(a, b, variant=variant), a, b, variant)


@pytest.mark.parametrize("n", [0, 1])
def test_fewer_than_two_samples_is_nan(n):
    for variant in VARIANTS:
        out = kendall_rank_corrcoef(torch.rand(n), torch.rand(n), variant=variant)
        assert out.shape == () and out.dtype == torch.float32 and out.isnan()
        out = kendall_rank_corrcoef(torch.rand(3, n), torch.rand(3, n), num_tasks=3, variant=variant)
        assert out.shape == (3,) and out.isnan().all()


@pytest.mark.parametrize("n", [3, 64, 65, 2049])
def test_signed_zeros_tie_in_either_operand(n):
    g = torch.Generator().manual_seed(n)
    z = torch.where(torch.rand(n, generator=g) < 0.5, -0.0, 0.0)
    z[n // 2:] = torch.floor(torch.rand(n - n // 2, generator=g) * 5) - 2.0
    _, y = pair(n, None, 11)
    both(z, y)
    both(y, z)
    assert torch.equal(_kendall_counts(z, y), _kendall_counts(z + 0.0, y))
    assert torch.equal(_kendall_counts(y, z), _kendall_counts(y, z + 0.0))
    if n <= 300:
        assert _kendall_counts(z, y).tolist() == [plain_counts(z, y)]


@pytest.mark.parametrize("n", [3, 64, 65, 2049])
def test_infinities_are_ordinary_values(n):
    x, y = (t.clone() - 0.5 for t in pair(n, None, 11))
    y[1], y[n // 2] = float("inf"), float("-inf")
    both(x, y)
    x[1], x[2] = float("-inf"), float("-inf")
    both(x, y)
    x[0] = float("inf")
    both(x, y)


@pytest.mark.parametrize("n", [2, 3, 65, 2049])
def test_nan_propagates_per_task(n):
    x, y = pair(n, 50, 12)
    bad = x.clone()
    bad[n // 2] = float("nan")
    for variant in VARIANTS:
        assert kendall_rank_corrcoef(bad, y, variant=variant).isnan()  # in input only
        assert kendall_rank_corrcoef(y, bad, variant=variant).isnan()  # in target only
    x3, y3 = (t.clone() for t in pair(n, 50, 13, 3))
    x3[1, n - 1] = float("nan")
    got = kendall_rank_corrcoef(x3, y3, num_tasks=3)
    assert got[1].isnan() and not got[0].isnan() and not got[2].isnan()
    both(x3, y3, 3)  # scipy propagates too; the other two tasks keep their values
    assert _kendall_counts(x3, y3)[1].tolist() == [-1] * 6  # no value, no counts
    y3[2, 0] = float("nan")
    both(x3, y3, 3)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("n", SIZES)
def test_narrow_floats_tie_where_they_round(dtype, n):
    x, y = (t.to(dtype) for t in pair(n, None, 14))
    if n == 2049:
        assert x.unique().numel() < n  # the narrow dtype made ties
    both(x, y)


@pytest.mark.parametrize("n", [3, 65, 2049])
def test_integer_float64_and_mixed_dtypes(n):
    x, y = pair(n, 50, 15)
    for a, b in ((x.long(), y.long()), (x.int(), y), (x.to(torch.int16), y.to(torch.uint8)), (x.half(), y.long()),
                 (x.to(torch.int8), y.bfloat16()), (x > 20, y)):
        both(a, b)
    xc, yc = pair(n, None, 16)
    both(xc.double(), yc.double(), dtype=torch.float64)
    both(xc.double(), yc, dtype=torch.float64)
    # int64 beyond 2^53 is compared as int64: as float64 the first three would tie
    big = torch.tensor([2**62, 2**62 + 1, 2**62 + 2, 5])
    other = torch.tensor([1.0, 2.0, 3.0, 0.0])
    assert _kendall_counts(big, other).tolist() == [[0, 0, 0, 0, 4, 4]]
    assert _kendall_counts(other, -big).tolist() == [[0, 0, 0, 6, 4, 4]]
    assert float(kendall_rank_corrcoef(big, other)) == 1.0 and float(kendall_rank_corrcoef(other, -big)) == -1.0


@pytest.mark.parametrize("n", [3, 65, 2049])
def test_non_contiguous_views(n):
    x, y = pair(n, 50, 17, 3)
    xt, yt = x.t().contiguous().t(), y.t().contiguous().t()  # [n, T].t()
    assert not xt.is_contiguous() and xt.stride(-1) == 3
    both(xt, yt, 3)
    wide = torch.zeros(3, 2 * n + 1)
    wide[:, 1::2] = x
    assert torch.equal(_kendall_counts(wide[:, 1::2], yt), _kendall_counts(x, y))
    assert torch.equal(_kendall_counts(wide[0, 1::2], y[0]), _kendall_counts(x[0], y[0]))


def test_invalid_arguments():
    x, y = torch.rand(3, 6), torch.rand(3, 6)
    with pytest.raises(ValueError, match="same shape"):
        kendall_rank_corrcoef(x[0], y[0, :5])
    with pytest.raises(ValueError, match="same shape"):
        kendall_rank_corrcoef(x, y[:2], num_tasks=3)
    with pytest.raises(ValueError, match="one-dimensional"):
        kendall_rank_corrcoef(x, y)
    with pytest.raises(ValueError, match="one-dimensional"):
        kendall_rank_corrcoef(torch.tensor(1.0), torch.tensor(2.0))
    with pytest.raises(ValueError, match=r"expected to be \(3, num_samples\)"):
        kendall_rank_corrcoef(x[0], y[0], num_tasks=3)
    with pytest.raises(ValueError, match=r"expected to be \(2, num_samples\)"):
        kendall_rank_corrcoef(x, y, num_tasks=2)
    with pytest.raises(ValueError, match=r"expected to be \(3, num_samples\)"):
        kendall_rank_corrcoef(x[None], y[None], num_tasks=3)
    with pytest.raises(ValueError, match="num_tasks"):
        kendall_rank_corrcoef(x[0], y[0], num_tasks=0)
    with pytest.raises(ValueError, match="num_tasks"):
        KendallRankCorrCoef(num_tasks=0)
    for bad in ("a", "B", "tau-b", None):
        with pytest.raises(ValueError, match="variant"):
            kendall_rank_corrcoef(x[0], y[0], variant=bad)
        with pytest.raises(ValueError, match="variant"):
            KendallRankCorrCoef(variant=bad)
    m = KendallRankCorrCoef(num_tasks=3)
    with pytest.raises(ValueError, match="same shape"):
        m.update(x, y[:, :5])
    with pytest.raises(ValueError, match="num_samples"):
        m.update(x[0], y[0])
    assert not m.inputs and not m.targets  # a refused update stores nothing


# ----------------------------------------------------------------------------- exactness
def test_sample_permutation_and_operand_swap_are_bit_identical():
    n = 4099
    g = torch.Generator().manual_seed(18)
    for levels in (3, 50, None):
        x, y = pair(n, levels, 18)
        perm = torch.randperm(n, generator=g)
        assert torch.equal(_kendall_counts(x[perm], y[perm]), _kendall_counts(x, y))
        for variant in VARIANTS:
            base = kendall_rank_corrcoef(x, y, variant=variant)
            assert torch.equal(kendall_rank_corrcoef(x[perm], y[perm], variant=variant), base)
        assert torch.equal(kendall_rank_corrcoef(y, x), kendall_rank_corrcoef(x, y))
    x, y = pair(n, 50, 19, 3)
    base = kendall_rank_corrcoef(x, y, num_tasks=3)
    perm = torch.randperm(n, generator=g)
    assert torch.equal(kendall_rank_corrcoef(x[:, perm], y[:, perm], num_tasks=3), base)
    assert torch.equal(kendall_rank_corrcoef(y, x, num_tasks=3), base)


def test_monotone_operands_give_exactly_one():
    x = torch.arange(1000.0)
    for variant in VARIANTS:  # without ties m = n and tau-c = 2 S / (n (n - 1)) as well
        assert float(kendall_rank_corrcoef(x, x**3, variant=variant)) == 1.0
        assert float(kendall_rank_corrcoef(x, -x, variant=variant)) == -1.0


def test_more_than_2_pow_32_discordant_pairs():
    n = 70001  # reversed: Q = n0 = 2 450 035 000
    up = torch.arange(n, dtype=torch.float32)
    assert _kendall_counts(up, -up).tolist() == [[0, 0, 0, n * (n - 1) // 2, n, n]]
    assert float(kendall_rank_corrcoef(up, -up)) == -1.0


# ----------------------------------------------------------------------------- class protocol
class TestKendallRankCorrCoef(MetricClassTester):
    def test_class_suite(self) -> None:
        x, y = pair(8 * 16, 50, 20)
        for variant in VARIANTS:
            self.run_class_implementation_tests(
                metric=KendallRankCorrCoef(variant=variant),
                state_names={"inputs", "targets"},
                update_kwargs={"input": x.reshape(8, 16), "target": y.reshape(8, 16)},
                compute_result=torch.tensor(float(oracle(x, y, variant))).float(),
                atol=TOL,
                rtol=0,
                num_processes=2,  # sync_and_compute on a 2-rank gloo world
            )

    def test_class_suite_three_tasks(self) -> None:
        x, y = pair(8 * 16, 50, 21, 3)
        ux, uy = (t.reshape(3, 8, 16).transpose(0, 1) for t in (x, y))  # update i is [3, 16]
        self.run_class_implementation_tests(
            metric=KendallRankCorrCoef(num_tasks=3),
            state_names={"inputs", "targets"},
            update_kwargs={"input": ux, "target": uy},
            compute_result=torch.tensor(oracle(x, y, "b")).float(),
            atol=TOL,
            rtol=0,
            num_processes=2,
        )


def test_compute_before_any_update_is_nan():
    out = KendallRankCorrCoef().compute()
    assert out.shape == () and out.dtype == torch.float32 and out.isnan()
    out = KendallRankCorrCoef(num_tasks=3, variant="c").compute()
    assert out.shape == (3,) and out.dtype == torch.float32 and out.isnan().all()


def test_updates_equal_the_functional_on_the_concatenation():
    x, y = pair(2049, 50, 22, 3)
    for variant in VARIANTS:
        m = KendallRankCorrCoef(num_tasks=3, variant=variant)
        for lo, hi in ((0, 1), (1, 65), (65, 2049)):
            m.update(x[:, lo:hi], y[:, lo:hi])
        assert torch.equal(m.compute(), kendall_rank_corrcoef(x, y, num_tasks=3, variant=variant))
        check(m.compute(), x, y, variant)


def test_merge_reset_state_dict_and_to():
    x, y = pair(65, 3, 23)
    a = KendallRankCorrCoef().update(x[:20], y[:20])
    b = KendallRankCorrCoef().update(x[20:40], y[20:40]).update(x[40:], y[40:])
    a.merge_state([b])
    assert len(b.inputs) == 2  # the merged metric is left alone
    want = kendall_rank_corrcoef(x, y)
    assert torch.equal(a.compute(), want)
    c = KendallRankCorrCoef()
    c.load_state_dict(a.state_dict())
    assert torch.equal(c.compute(), want)
    assert a.to("cpu") is a and torch.equal(a.compute(), want)
    a.reset()
    assert a.inputs == [] and a.targets == [] and a.compute().isnan()
    a.update(x, y)
    assert torch.equal(a.compute(), want)


# ----------------------------------------------------------------------------- exports, routing
def test_exports():
    for mod in (M, MR):
        assert mod.KendallRankCorrCoef is KendallRankCorrCoef
    for mod in (MF, MFR):
        assert mod.kendall_rank_corrcoef is kendall_rank_corrcoef
    assert "KendallRankCorrCoef" in MR.__all__ and "kendall_rank_corrcoef" in MFR.__all__
    # the top-level lists mirror the reference's public names, which have no Kendall
    assert "KendallRankCorrCoef" not in M.__all__ and "kendall_rank_corrcoef" not in MF.__all__


def test_cpu_tensors_take_the_aten_form():
    from torcheval_amd.ops import kendall as K

    x, y = pair(65, None, 24)
    assert not K.supported(x, y)


def test_traces_through_aot_autograd():
    """The functional under torch.compile with the AOT (functionalizing) tracer, as inductor uses it:
    1-D operands and a transposed view, whose first op is a view of a graph input."""
    x, y = pair(65, 50, 25, 3)
    torch._dynamo.reset()
    one = torch.compile(lambda a, b: kendall_rank_corrcoef(a, b, variant="c"), fullgraph=True, backend="aot_eager")
    assert torch.equal(one(x[0], y[0]), kendall_rank_corrcoef(x[0], y[0], variant="c"))
    torch._dynamo.reset()
    many = torch.compile(lambda a, b: kendall_rank_corrcoef(a, b, num_tasks=3), fullgraph=True, backend="aot_eager")
    assert torch.equal(many(x, y.t().contiguous().t()), kendall_rank_corrcoef(x, y, num_tasks=3))
    torch._dynamo.reset()


def test_tile_constant_equals_the_kernel_header():
    import os
    import re

    from torcheval_amd.ops import kendall as K

    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    with open(os.path.join(root, "csrc", "include", "tea_kernels.h")) as fh:
        header = fh.read()
    assert int(re.search(r"constexpr int kKendallTile = (\d+);", header).group(1)) == K.TILE


def test_native_op_surface_and_compiled_route(monkeypatch):
    """K19's two ops: their schemas, which dispatch keys hold a kernel, Meta kernels that return
    None, and the wrapper on meta tensors with ``compiling`` forced (both sorts then go through
    their dispatcher op as well)."""
    from torcheval_amd.ops import kendall as K

    names = sorted(n for n in torch._C._dispatch_get_all_op_names() if n.startswith("torcheval_amd_kendall::"))
    assert names == ["torcheval_amd_kendall::kendall_count", "torcheval_amd_kendall::kendall_prepare"]
    prepare = torch.ops.torcheval_amd_kendall.kendall_prepare.default
    count = torch.ops.torcheval_amd_kendall.kendall_count.default
    assert str(prepare._schema) == (
        "torcheval_amd_kendall::kendall_prepare(Tensor sorted, Tensor order, Tensor x, Tensor(a!) s, "
        "Tensor(b!) xg, Tensor(c!) part, Tensor(d!) flags) -> ()")
    assert str(count._schema) == (
        "torcheval_amd_kendall::kendall_count(Tensor sorted, Tensor carried, Tensor(a!) part, Tensor(b!) flags, "
        "int variant, Tensor(c!) out, Tensor(d!) counts) -> ()")
    for name in names:
        has = [k for k in ("CPU", "CUDA", "Meta") if torch._C._dispatch_has_kernel_for_dispatch_key(name, k)]
        assert has == ["CUDA", "Meta"]
    meta = torch.device("meta")
    f = torch.empty(3, 9, device=meta)
    i = torch.empty(3, 9, dtype=torch.int32, device=meta)
    part = torch.empty(3, 6, 1, dtype=torch.int64, device=meta)
    flags = torch.empty(3, 2, dtype=torch.int32, device=meta)
    assert prepare(f, i, f, i, f, part, flags) is None
    assert count(f, i, part, flags, 1, torch.empty(3, device=meta),
                 torch.empty(3, 6, dtype=torch.int64, device=meta)) is None
    monkeypatch.setattr(ops, "compiling", lambda: True)
    out, counts = K.kendall(torch.empty(3, 9, device=meta), torch.empty(3, 9, dtype=torch.float16, device=meta), True)
    assert out.shape == (3,) and out.dtype == torch.float32 and out.device.type == "meta"
    assert counts.shape == (3, 6) and counts.dtype == torch.int64 and counts.device.type == "meta"
