"""K19 (csrc/kernels/kendall.hip) on the GPU: Kendall's tau behind two K3a sorts.

Oracle and tolerance as in tests/metrics/regression/test_kendall.py: ``scipy.stats.kendalltau`` in
FP64 per task on the values the kernel sees, and ``|got - float32(oracle)| <= 2^-23`` (both sides
evaluate one FP64 expression of exact integers and round once to float32; ``|tau| <= 1``).  NaN
must match NaN.  On top of that the six integers ``_kendall_counts`` returns from the kernels must
equal, exactly, those the ATen form returns for CPU copies of the operands.

Shapes are the smallest at which each piece can go wrong: around a wave, around the tile ``T``
(read from ``ops.kendall``; it is also the span of the run kernels) and its multiples, K3a's 4096
edge, an unpaired run at a merge level (3T + 5), a one-element last tile (4T + 1), tie runs that
straddle a tile boundary or cover whole tiles, 35 tiles with odd run counts at several levels and
more than 2^32 discordant pairs, and row counts on both sides of K3a's onesweep limit of 8 rows.
"""

import functools
import warnings

import numpy as np
import pytest
import torch
from scipy import stats

from torcheval_amd.metrics import KendallRankCorrCoef
from torcheval_amd.metrics.functional import kendall_rank_corrcoef
from torcheval_amd.metrics.functional.regression.kendall import _kendall_counts
from torcheval_amd.ops import kendall as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TOL = 2.0**-23
T = K.TILE
EDGES = sorted({2, 3, 63, 64, 65, 4095, 4096, 4097}
               | {T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 5, 4 * T + 1})


def oracle(x: torch.Tensor, y: torch.Tensor, variant: str) -> np.ndarray:
    xs, ys = x.double().cpu().numpy(), y.double().cpu().numpy()
    flat = xs.ndim == 1
    xs, ys = np.atleast_2d(xs), np.atleast_2d(ys)
    out = np.full(xs.shape[0], np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in range(xs.shape[0]):
            out[i] = stats.kendalltau(xs[i], ys[i], variant=variant).statistic
    return out[0] if flat else out


def check_value(got: torch.Tensor, x: torch.Tensor, y: torch.Tensor, variant: str, dtype=torch.float32):
    want = np.asarray(oracle(x, y, variant))
    assert got.dtype == dtype and tuple(got.shape) == want.shape and got.device == x.device
    g = got.double().cpu().numpy()
    assert np.array_equal(np.isnan(g), np.isnan(want)), (g, want)
    if dtype == torch.float32:
        want = want.astype(np.float32).astype(np.float64)
    err = np.abs(g - want)[~np.isnan(want)]
    assert float(err.max(initial=0.0)) <= (TOL if dtype == torch.float32 else 2.0**-50), float(err.max())


def counts(x, y) -> torch.Tensor:
    assert K.supported(x, y)
    return _kendall_counts(x, y).cpu()


def check(x: torch.Tensor, y: torch.Tensor, tasks: int = 1) -> torch.Tensor:
    """Both variants against scipy and the counts against the ATen form on CPU copies; the counts."""
    assert K.supported(x, y)
    for variant in ("b", "c"):
        check_value(kendall_rank_corrcoef(x, y, num_tasks=tasks, variant=variant), x, y, variant)
    got = counts(x, y)
    want = _kendall_counts(x.cpu(), y.cpu())
    assert got.dtype == torch.int64 and torch.equal(got, want), (got, want)
    return got


@functools.lru_cache(maxsize=None)
def pair(n: int, levels, seed: int, tasks: int = 1):
    """Correlated float32 operands on the GPU; ``levels`` rounds both to that many values.  Shared
    between tests: never modified in place."""
    g = torch.Generator().manual_seed(seed)
    shape = (n,) if tasks == 1 else (tasks, n)
    x = torch.rand(shape, generator=g)
    y = 0.6 * x + 0.4 * torch.rand(shape, generator=g)
    if levels is not None:
        x, y = torch.floor(x * levels), torch.floor(y * levels)
    return x.to(DEV), y.to(DEV)


# ----------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("levels", [None, 50, 3])
@pytest.mark.parametrize("n", EDGES)
def test_small_sizes_and_tile_edges(n, levels):
    check(*pair(n, levels, n))


# ----------------------------------------------------------------------------- merge edge cases
@pytest.mark.parametrize("n", [65, T + 1, 3 * T + 5, 70001])
def test_sorted_operands_have_no_or_only_discordant_pairs(n):
    up = torch.arange(n, dtype=torch.float32, device=DEV)
    n0 = n * (n - 1) // 2
    assert check(up, up * 3 + 1)[0].tolist() == [0, 0, 0, 0, n, n]
    assert check(up, -up)[0].tolist() == [0, 0, 0, n0, n, n]  # n = 70001: Q = 2.45e9 > 2^32
    assert float(kendall_rank_corrcoef(up, up)) == 1.0 and float(kendall_rank_corrcoef(up, -up)) == -1.0
    assert float(kendall_rank_corrcoef(up, -up, variant="c")) == -1.0  # m = n: 2 S = -n (n - 1)


@pytest.mark.parametrize("levels", [None, 50])
def test_35_tiles_with_odd_run_counts(levels):
    check(*pair(70001, levels, 4))


def test_66_tiles_the_finish_wave_takes_a_second_round():
    check(*pair(65 * T + 5, 50, 5))


def test_tie_runs_straddle_one_tile_boundary():
    n = 2 * T + 4
    g = torch.Generator().manual_seed(1)
    x = torch.arange(n, dtype=torch.float32)
    x[T - 48:T + 52] = float(T)  # sorted (either direction) the run crosses position T
    order = torch.randperm(n, generator=g)
    x = x[order].to(DEV)
    _, y = pair(n, 50, 2)
    check(x, y)  # a run of input
    check(y, x)  # a run of target
    both = torch.arange(n, dtype=torch.float32)
    both[T - 48:T + 52] = float(T)
    both = both[order].to(DEV)
    check(x, both)  # a run of both, on the same items
    half = both.clone()
    half[half == float(T)] = torch.arange(100, dtype=torch.float32, device=DEV).remainder(2) + float(T)
    check(x, half)  # joint runs that split an input run at the boundary


def test_tie_runs_cover_whole_tiles():
    n = 3 * T + 5
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(n, generator=g) < 0.5).float().to(DEV)  # two values: two runs of ~1.5 tiles
    y = (torch.rand(n, generator=g) < 0.9).float().to(DEV)  # one run of ~2.7 tiles
    check(x, y)
    check(y, x)
    check(x, x)
    one = torch.zeros(n, device=DEV)
    one[n // 3] = -1.0  # all equal but one element
    check(one, y)
    check(y, -one)
    check(one, one)
    const = torch.full((n,), 7.0, device=DEV)
    for variant in ("b", "c"):
        for a, b in ((const, y), (y, const), (const, const)):
            assert kendall_rank_corrcoef(a, b, variant=variant).isnan()
    check(const, y)


# ----------------------------------------------------------------------------- special values
@pytest.mark.parametrize("n", [65, T + 1, 2 * T + 1])
def test_signed_zeros_tie(n):
    """A -0.0 / +0.0 mix inside one tie group of an operand whose partner's values differ.  A sort
    that ordered the two zeros by bit pattern would split the group and carry its target runs out of
    order (false inversions, a wrong n3); K3a folds -0.0 into +0.0 in its keys, and this holds it to
    that."""
    g = torch.Generator().manual_seed(n)
    z = torch.where(torch.rand(n, generator=g) < 0.5, -0.0, 0.0)
    z[n // 2:] = torch.floor(torch.rand(n - n // 2, generator=g) * 5) - 2.0  # -2 .. 2, zeros of one sign among them
    z = z[torch.randperm(n, generator=g)].to(DEV)
    zeros = torch.signbit(z[z == 0])
    assert zeros.numel() > 2 and bool(zeros.any()) and not bool(zeros.all())
    _, other = pair(n, None, 8)
    _, tied = pair(n, 3, 8)
    for o in (other, tied):
        want = counts(z + 0.0, o)  # the same values with one zero
        assert torch.equal(check(z, o), want)
        want = counts(o, z + 0.0)
        assert torch.equal(check(o, z), want)


@pytest.mark.parametrize("n", [3, 65, T + 1])
def test_infinities_are_ordinary_values(n):
    x, y = (t.clone() - 0.5 for t in pair(n, None, 8))
    y[1], y[n // 2] = float("inf"), float("-inf")
    check(x, y)
    x[1], x[2] = float("-inf"), float("-inf")
    check(x, y)
    x[0] = float("inf")
    check(x, y)


@pytest.mark.parametrize("n", [2, 65, T + 1, 2 * T + 1])
def test_nan_propagates_per_task(n):
    x, y = pair(n, 50, 9)
    bad = x.clone()
    bad[n - 1] = float("nan")  # at T + 1 / 2 T + 1: the only element past the tile edge
    for variant in ("b", "c"):
        assert kendall_rank_corrcoef(bad, y, variant=variant).isnan()  # input only
        assert kendall_rank_corrcoef(y, bad, variant=variant).isnan()  # target only
    assert counts(bad, y).tolist() == [[-1] * 6] and counts(y, bad).tolist() == [[-1] * 6]
    x3, y3 = (t.clone() for t in pair(n, 50, 10, 3))
    x3[1, n - 1] = float("nan")
    got = kendall_rank_corrcoef(x3, y3, num_tasks=3)
    assert got[1].isnan() and not got[0].isnan() and not got[2].isnan()
    check(x3, y3, 3)
    y3[2, n // 2] = float("nan")
    check(x3, y3, 3)


# ----------------------------------------------------------------------------- tasks
@pytest.mark.parametrize("tasks", [3, 4, 8, 9])
def test_rows_around_the_onesweep_limit(tasks):
    for n in (65, T + 1):
        check(*pair(n, 50, 5, tasks), tasks)
    check(*pair(2 * T + 1, None, 6, tasks), tasks)


def test_many_short_rows():
    check(*pair(257, 50, 7, 100), 100)


# ----------------------------------------------------------------------------- dtypes, layouts
NATIVE_DTYPES = (torch.float32, torch.float16, torch.bfloat16, torch.int8, torch.uint8, torch.int16)


@pytest.mark.parametrize("n", [65, T + 1])
def test_native_dtype_grid(n):
    xf, yf = pair(n, None, 11, 3)
    for dx in NATIVE_DTYPES:
        for dy in NATIVE_DTYPES:
            x = (xf * 100).to(dx) if not dx.is_floating_point else xf.to(dx)
            y = (yf * 100).to(dy) if not dy.is_floating_point else yf.to(dy)
            check(x, y, 3)


def test_float64_and_int64_take_the_aten_form():
    x, y = pair(T + 1, 50, 12)
    for a, b, dtype in ((x.double(), y.double(), torch.float64), (x.double(), y, torch.float64),
                        (x.long(), y.long(), torch.float32), (x, y.long(), torch.float32),
                        (x.int(), y, torch.float32)):
        assert not K.supported(a, b)
        for variant in ("b", "c"):
            check_value(kendall_rank_corrcoef(a, b, variant=variant), a, b, variant, dtype)
        assert torch.equal(_kendall_counts(a, b).cpu(), counts(x, y))
    assert not K.supported(x[:1], y[:1]) and kendall_rank_corrcoef(x[:1], y[:1]).isnan()
    assert K.supported(x, y) and not K.supported(x, y.cpu())


@pytest.mark.parametrize("n", [65, T + 1, 2 * T + 3])
def test_strided_views_and_an_unaligned_base(n):
    x, y = pair(n, 50, 13, 3)
    want = check(x, y, 3)
    buf = torch.zeros(n + 1, device=DEV)
    buf[1:] = x[0]
    assert buf[1:].data_ptr() % 16 == 4
    assert torch.equal(counts(buf[1:], y[0]), want[:1])
    xt, yt = x.t().contiguous().t(), y.t().contiguous().t()  # [n, tasks].t()
    assert xt.stride(-1) == 3
    assert torch.equal(counts(xt, yt), want) and torch.equal(counts(xt, y), want)
    wide = torch.zeros(3, 2 * n + 1, device=DEV)
    wide[:, 1::2] = x
    assert torch.equal(counts(wide[:, 1::2], yt.half()), want)  # x[::2]-style rows; 50 levels are exact in f16
    assert torch.equal(counts(torch.cat([x[0], x[0]])[::2], torch.cat([y[0], y[0]])[::2]),
                       _kendall_counts(torch.cat([x[0], x[0]])[::2].cpu(), torch.cat([y[0], y[0]])[::2].cpu()))


# ----------------------------------------------------------------------------- exactness
def test_bit_identical_under_permutation_and_operand_swap():
    n = 70001
    g = torch.Generator().manual_seed(14)
    x, y = pair(n, 50, 14)
    base = {v: kendall_rank_corrcoef(x, y, variant=v) for v in ("b", "c")}
    c = counts(x, y)
    perm = torch.randperm(n, generator=g).to(DEV)
    assert torch.equal(counts(x[perm], y[perm]), c)
    for v in ("b", "c"):
        assert torch.equal(kendall_rank_corrcoef(x[perm], y[perm], variant=v), base[v])
    assert torch.equal(kendall_rank_corrcoef(y, x), base["b"])
    assert counts(y, x)[0].tolist() == [c[0, i].item() for i in (1, 0, 2, 3, 5, 4)]


# ----------------------------------------------------------------------------- class, compile
def test_class_updates_equal_the_functional_on_the_concatenation():
    x, y = pair(T + 1, 50, 16, 3)
    for variant in ("b", "c"):
        m = KendallRankCorrCoef(num_tasks=3, variant=variant, device=DEV)
        assert m.compute().isnan().all() and m.compute().device == DEV
        for lo, hi in ((0, 1), (1, 65), (65, T + 1)):
            m.update(x[:, lo:hi], y[:, lo:hi])
        assert torch.equal(m.compute(), kendall_rank_corrcoef(x, y, num_tasks=3, variant=variant))
    check_value(m.compute(), x, y, "c")


def test_class_merge_state():
    x, y = pair(2 * T + 4, None, 17)
    a = KendallRankCorrCoef(device=DEV).update(x[:1000], y[:1000])
    b = KendallRankCorrCoef(device=DEV).update(x[1000:3000], y[1000:3000]).update(x[3000:], y[3000:])
    a.merge_state([b])
    assert torch.equal(a.compute(), kendall_rank_corrcoef(x, y))
    check_value(a.compute(), x, y, "b")
    a.reset()
    assert a.compute().isnan()


def test_compiled_functional_matches_eager():
    x, y = pair(T + 1, 50, 18, 3)
    torch._dynamo.reset()
    for variant in ("b", "c"):
        fn = torch.compile(lambda a, b: kendall_rank_corrcoef(a, b, num_tasks=3, variant=variant), fullgraph=True)
        assert torch.equal(fn(x, y), kendall_rank_corrcoef(x, y, num_tasks=3, variant=variant))
    yt = y.t().contiguous().t()  # the tiled transpose stays in the graph as its dispatcher op
    assert torch.equal(fn(x, yt), kendall_rank_corrcoef(x, y, num_tasks=3, variant="c"))
    torch._dynamo.reset()
    one = torch.compile(lambda a, b: kendall_rank_corrcoef(a, b), fullgraph=True)  # 1-D: a view of a graph input
    assert torch.equal(one(x[0], y[0]), kendall_rank_corrcoef(x[0], y[0]))
