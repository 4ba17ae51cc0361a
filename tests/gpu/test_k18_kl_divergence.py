"""K18 (csrc/kernels/kl_divergence.hip) on the GPU: KL divergence of logit or weight rows in one
pass over both operands.

Oracle: tests/_kl_oracle.py, numpy FP64 of the definition in docs/parity.md, on the values the
kernel sees (16-bit operands widened exactly).

* Row values (``"none"``) and ``"mean"`` (the K12 / K15 rule): the GPU result lies within ``MULT`` x
  the error of the float32 ATen form (``DISABLE_HIP``, same device tensors) against the oracle, plus
  1e-6; both errors are against the oracle, never against each other, and for the rows both are the
  largest over the rows of the case.  Inputs are drawn with ``|logit| <= 8``, so one float32 ulp of
  the largest intermediate (9.5e-7) stays under the floor.  ``inf`` must match ``inf`` and NaN must
  match NaN exactly.
* ``"sum"``, ``"mean"`` and the class states against the ``"none"`` values of the same call: the
  kernel adds the FP64 row values, ``"none"`` stores their float32, so the FP64 sum of the stored
  rows is within ``n 2^-24 max|row|`` of the state and the float32 results within one float32 ulp.

Shapes are the smallest at which each piece of the walk can go wrong: widths around a lane's step
of 16, a wave's step of 1024 and the unrolled pair of steps (1023, 1040, 2053, 2064), one vocabulary
row pair at 50257; one row, a block's four waves, one more, and a few more rows than the capped grid
covers at one row per wave; row starts 1-3 elements off an allocation's alignment.
"""

import contextlib
import functools

import numpy as np
import pytest
import torch

import torcheval_amd.ops as ops
from tests import _kl_oracle as O
from torcheval_amd.metrics import KLDivergence
from torcheval_amd.metrics.functional import kl_divergence
from torcheval_amd.ops import kl_divergence as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
MULT, FLOOR = 4.0, 1e-6
CS = (1, 2, 15, 16, 17, 63, 64, 65, 1023, 1040, 2053, 2064)
NS = (1, 4, 5)
DTYPES = (torch.float32, torch.float16, torch.bfloat16)


@pytest.fixture
def native_calls(monkeypatch):
    """Counts the calls through the K18 wrapper: the native path really ran."""
    calls = []
    for name in ("kl_update", "kl_batch"):
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
def pair(n: int, c: int, seed: int, logits: bool, dtype: torch.dtype):
    """Seeded CPU ``(input, target)`` in ``dtype``: logits within [-8, 8], or positive weights that
    do not sum to 1.  Shared between tests, never modified."""
    g = torch.Generator().manual_seed(seed)
    if logits:
        x = (torch.randn(n, c, generator=g, dtype=torch.float64) * 3).clamp(-8, 8)
        t = (x + torch.randn(n, c, generator=g, dtype=torch.float64)).clamp(-8, 8)
    else:
        x = torch.randn(n, c, generator=g, dtype=torch.float64)
        t = x + 0.5 * torch.randn(n, c, generator=g, dtype=torch.float64)
        x, t = torch.softmax(x, -1) * 3.0, torch.softmax(t, -1) * 0.5
    return x.to(dtype), t.to(dtype)


@functools.lru_cache(maxsize=None)
def oracle_rows(n: int, c: int, seed: int, logits: bool, dtype: torch.dtype):
    x, t = pair(n, c, seed, logits, dtype)
    return O.rows(x.double().numpy(), t.double().numpy(), logits)


def ulp32(v: float) -> float:
    return float(np.spacing(np.float32(abs(v))))


def check_rows(got: torch.Tensor, aten: torch.Tensor, want: np.ndarray, what: str):
    """The rule on a set of row values: NaN and inf exact, the largest finite error within the bound."""
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and got.device == DEV
    g, a = got.double().cpu().numpy(), aten.double().cpu().numpy()
    assert np.array_equal(np.isnan(g), np.isnan(want)), (what, g, want)
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(g), inf) and np.array_equal(g[inf], want[inf]), (what, g, want)
    fin = np.isfinite(want)
    err = float(np.abs(g[fin] - want[fin]).max(initial=0.0))
    aten_err = float(np.abs(a[fin] - want[fin]).max(initial=0.0))
    print(f"k18 {what}: gpu / aten error {err:.2e} / {aten_err:.2e}")
    assert err <= MULT * aten_err + FLOOR, (what, err, aten_err)


def check(xd, td, want: np.ndarray, logits: bool, what: str, maskd=None):
    """The three reductions and one class update of device operands against the oracle's row
    values ``want`` (0 for uncounted rows), with the ATen form of the same tensors as yardstick."""
    kw = dict(from_logits=logits, mask=maskd)
    got = kl_divergence(xd, td, reduction="none", **kw)
    total, mean = kl_divergence(xd, td, reduction="sum", **kw), kl_divergence(xd, td, reduction="mean", **kw)
    m = KLDivergence(from_logits=logits, device=DEV).update(xd, td, mask=maskd)
    with aten_form():
        aten = kl_divergence(xd, td, reduction="none", **kw)
        aten_mean = kl_divergence(xd, td, reduction="mean", **kw)
    check_rows(got, aten, want, what)
    count = want.size if maskd is None else int(maskd.sum())
    assert m.num_rows.dtype == torch.float64 and float(m.num_rows) == count
    for v in (total, mean, m.compute()):
        assert v.dtype == torch.float32 and v.shape == () and v.device == DEV
    if maskd is not None:
        assert bool((got[~maskd] == 0).all())
    rows = got.double()
    s = float(rows.sum())
    if not np.isfinite(want).all():  # by the arithmetic: NaN wins, else inf
        for v in (total, mean, m.kl_sum, m.compute()):
            assert (np.isnan(s) and bool(v.isnan())) or float(v) == s, (what, float(v), s)
        return
    assert abs(float(m.kl_sum) - s) <= max(count, 1) * 2.0**-24 * float(rows.abs().max()), (what, float(m.kl_sum), s)
    assert abs(float(total) - s) <= ulp32(s), (what, float(total), s)
    if count == 0:
        assert bool(mean.isnan()) and bool(m.compute().isnan())
        return
    assert abs(float(mean) - s / count) <= ulp32(s / count), (what, float(mean), s / count)
    assert abs(float(m.compute()) - s / count) <= ulp32(s / count)
    want_mean = float(want.sum()) / count
    err, aten_err = abs(float(mean) - want_mean), abs(float(aten_mean) - want_mean)
    assert err <= MULT * aten_err + FLOOR, (what, "mean", err, aten_err)


# ----------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("logits", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_widths_rows_and_dtypes(dtype, logits, native_calls):
    for n in NS:
        for c in CS:
            x, t = pair(n, c, 100 + c, logits, dtype)
            before = len(native_calls)
            check(x.to(DEV), t.to(DEV), oracle_rows(n, c, 100 + c, logits, dtype), logits, f"{n}x{c} {dtype}")
            assert len(native_calls) == before + 4  # three functional calls, one update


@pytest.mark.parametrize("logits", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_vocabulary_row_pair(dtype, logits, native_calls):
    x, t = pair(1, 50257, 50257, logits, dtype)
    check(x.to(DEV), t.to(DEV), oracle_rows(1, 50257, 50257, logits, dtype), logits, f"1x50257 {dtype}")
    assert len(native_calls) == 4


@pytest.mark.parametrize("logits", [True, False])
def test_more_rows_than_the_grid_covers_and_two_runs(logits, native_calls):
    """4101 rows at 33 columns: the capped grid's waves take a second row.  Two runs on the same
    tensors are bit-identical, in every reduction and in the states."""
    n = K.ROWS_PER_LAUNCH + 5
    assert n == 4101
    x, t = pair(n, 33, 33, logits, torch.float32)
    xd, td = x.to(DEV), t.to(DEV)
    check(xd, td, oracle_rows(n, 33, 33, logits, torch.float32), logits, f"{n}x33")
    assert len(native_calls) == 4
    for red in ("none", "sum", "mean"):
        a = kl_divergence(xd, td, from_logits=logits, reduction=red)
        b = kl_divergence(xd, td, from_logits=logits, reduction=red)
        assert torch.equal(a, b)
    a = KLDivergence(from_logits=logits, device=DEV).update(xd, td).update(xd, td)
    b = KLDivergence(from_logits=logits, device=DEV).update(xd, td).update(xd, td)
    assert torch.equal(a.kl_sum, b.kl_sum) and torch.equal(a.num_rows, b.num_rows) and float(a.num_rows) == 2 * n


@pytest.mark.parametrize("logits", [True, False])
@pytest.mark.parametrize("n", [257, 4096])
def test_finish_runs_full_short_and_empty(n, logits, native_calls):
    """The finish launch's fold over runs of blocks (tea_partials.h run_fold) at three columns.
    257 rows are 65 blocks: 32 runs of two, one of a single block, 31 empty.  4096 rows are the
    capped 1024 blocks with no row left over: 64 runs of exactly one round of 16 loads.  (One block
    and the capped grid with grid-stride rows are reached by the tests above.)  At 257 rows also
    with every third row masked off, so that the count is not the number of rows."""
    x, t = pair(n, 3, 3000 + n, logits, torch.float32)
    want = oracle_rows(n, 3, 3000 + n, logits, torch.float32)
    xd, td = x.to(DEV), t.to(DEV)
    check(xd, td, want, logits, f"{n}x3")
    assert len(native_calls) == 4
    if n == 257:
        mask = torch.arange(n) % 3 != 0
        check(xd, td, np.where(mask.numpy(), want, 0.0), logits, f"{n}x3 masked", mask.to(DEV))
        assert len(native_calls) == 8


def test_nearly_equal_distributions_keep_sign_and_size(native_calls):
    """KL about 1e-6: the bound's floor is absolute, so this checks sign and size only (no value is
    negative beyond the floor and none exceeds 1e-5)."""
    x, _ = pair(5, 1040, 1140, True, torch.float32)
    t = x + 2e-3 * torch.sin(torch.arange(1040.0))
    want = O.rows(x.double().numpy(), t.double().numpy(), True)
    assert 0 < want.max() < 5e-6
    xd, td = x.to(DEV), t.to(DEV)
    got = kl_divergence(xd, td, reduction="none")
    assert len(native_calls) == 1
    with aten_form():
        aten = kl_divergence(xd, td, reduction="none")
    check_rows(got, aten, want, "5x1040 nearly equal")
    assert float(got.min()) > -FLOOR and float(got.max()) < 1e-5


# ----------------------------------------------------------------------------- alignment and layout
def offset_view(v: torch.Tensor, k: int, pad: int = 5) -> torch.Tensor:
    """``v`` ``[n, c]`` on the GPU as columns ``k : k + c`` of a fresh ``[n, c + pad]`` parent."""
    n, c = v.shape
    parent = torch.zeros(n, c + pad, dtype=v.dtype, device=DEV)
    parent[:, k:k + c] = v.to(DEV)
    return parent[:, k:k + c]


@pytest.mark.parametrize("logits", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_off_the_alignment(dtype, logits, native_calls):
    """Views that start 1, 2 and 3 elements into a parent.  Both operands offset alike run the
    kernel (every row another head: the parent's width is odd); offset differently they take the
    ATen form and give the same values."""
    for i, (n, c) in enumerate(((5, 2053), (4, 65), (5, 17))):
        k = 1 + i
        x, t = pair(n, c, 100 + c, logits, dtype)
        want = oracle_rows(n, c, 100 + c, logits, dtype)
        xv, tv = offset_view(x, k), offset_view(t, k)
        assert xv.data_ptr() % 16 != 0 and xv.data_ptr() % 16 == tv.data_ptr() % 16 and not xv.is_contiguous()
        before = len(native_calls)
        check(xv, tv, want, logits, f"{n}x{c} {dtype} both off by {k}")
        assert len(native_calls) == before + 4
        other = offset_view(t, k % 3 + 1)
        assert other.data_ptr() % 16 != xv.data_ptr() % 16
        assert not K.supported(xv, other)
        before = len(native_calls)
        check(xv, other, want, logits, f"{n}x{c} {dtype} off by {k} and {k % 3 + 1}")
        assert len(native_calls) == before  # the fallback


@pytest.mark.parametrize("logits", [True, False])
def test_row_strides_and_batched_inputs(logits, native_calls):
    x, t = pair(5, 1023, 1123, logits, torch.float32)
    want = oracle_rows(5, 1023, 1123, logits, torch.float32)
    # padded rows; the strides differ by a whole number of 16-B units (8 elements), then by 3 elements
    xv, tv = offset_view(x, 0, pad=1), offset_view(t, 0, pad=9)
    check(xv, tv, want, logits, "5x1023 strides 1024 and 1032")
    assert len(native_calls) == 4
    tv = offset_view(t, 0, pad=4)
    assert not K.supported(xv, tv)
    check(xv, tv, want, logits, "5x1023 strides 1024 and 1027")
    assert len(native_calls) == 4
    # every second row of a taller buffer
    tall_x, tall_t = torch.zeros(10, 1023, device=DEV), torch.zeros(10, 1023, device=DEV)
    tall_x[::2], tall_t[::2] = x.to(DEV), t.to(DEV)
    check(tall_x[::2], tall_t[::2], want, logits, "5x1023 every second row")
    assert len(native_calls) == 8
    # [B, S, C] with a [B, S] mask, contiguous and as a padded view whose leading dimensions flatten
    x, t = pair(6, 65, 165, logits, torch.bfloat16)
    mask = torch.tensor([[True, False, True], [True, True, False]])
    want = np.where(mask.numpy(), oracle_rows(6, 65, 165, logits, torch.bfloat16).reshape(2, 3), 0.0)
    check(x.to(DEV).reshape(2, 3, 65), t.to(DEV).reshape(2, 3, 65), want, logits, "2x3x65", mask.to(DEV))
    check(offset_view(x, 0, pad=8).unflatten(0, (2, 3)), offset_view(t, 0, pad=8).unflatten(0, (2, 3)), want, logits,
          "2x3x65 padded", mask.to(DEV))
    assert len(native_calls) == 16
    # leading dimensions that do not flatten: the ATen form
    big = torch.zeros(2, 4, 65, dtype=torch.bfloat16, device=DEV)
    big[:, :3] = x.to(DEV).reshape(2, 3, 65)
    assert not K.supported(big[:, :3], t.to(DEV).reshape(2, 3, 65))
    check(big[:, :3], t.to(DEV).reshape(2, 3, 65), want, logits, "2x3x65 of 2x4x65", mask.to(DEV))
    assert len(native_calls) == 16


@pytest.mark.parametrize("logits", [True, False])
def test_mask_with_first_last_and_a_whole_block_off(logits, native_calls):
    """Rows 0, 12 and 4-7 (the second block's four waves) are off and full of NaN."""
    x, t = pair(13, 65, 265, logits, torch.float32)
    mask = torch.ones(13, dtype=torch.bool)
    mask[[0, 4, 5, 6, 7, 12]] = False
    want = np.where(mask.numpy(), oracle_rows(13, 65, 265, logits, torch.float32), 0.0)
    xd, td = x.to(DEV), t.to(DEV)
    xd[~mask.to(DEV)], td[~mask.to(DEV)] = float("nan"), float("nan")
    check(xd, td, want, logits, "13x65 masked", mask.to(DEV))
    assert len(native_calls) == 4
    none = torch.zeros(13, dtype=torch.bool, device=DEV)
    check(xd, td, np.zeros(13), logits, "13x65 all masked", none)
    m = KLDivergence(from_logits=logits, device=DEV).update(xd, td, mask=mask.to(DEV))
    before = (m.kl_sum.clone(), m.num_rows.clone())
    m.update(xd, td, mask=none)  # no counted row: a no-op
    assert torch.equal(m.kl_sum, before[0]) and torch.equal(m.num_rows, before[1])


# ----------------------------------------------------------------------------- special values
@pytest.mark.parametrize("logits", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values_in_head_body_and_tail(dtype, logits, native_calls):
    """Every special-value row of the definition with its entry in the scalar head (column 0), the
    16-B body (1000) and the scalar tail (2052) of a 2053-column row that starts one element off the
    alignment, and a masked row full of NaN.  The dtype's lowest finite value, the usual fill of masked
    vocabulary entries, is an ordinary logit: its rows are finite, and the one with it in ``input``
    alone is about ``p_j |lowest|``, so it is held to the rule apart from the rows of ordinary size."""
    xs, ts, lowest = [], [], []
    for at in (0, 1000, 2052):
        for name, x, t, _ in O.special_rows(logits, 2053, at, seed=at, low=float(torch.finfo(dtype).min)):
            lowest.append(name == "lowest finite value in input")
            xs.append(torch.from_numpy(x))
            ts.append(torch.from_numpy(t))
    xs.append(torch.full((2053,), float("nan")))
    ts.append(torch.full((2053,), float("nan")))
    x, t = torch.stack(xs).to(dtype), torch.stack(ts).to(dtype)
    mask = torch.ones(len(xs), dtype=torch.bool)
    mask[-1] = False
    want = O.rows(x.double().numpy(), t.double().numpy(), logits, mask.numpy())
    assert np.isnan(want).sum() >= 27 and np.isinf(want).sum() == 3 and np.isfinite(want).sum() >= 7
    xv, tv, maskd = offset_view(x, 1), offset_view(t, 1), mask.to(DEV)
    got = kl_divergence(xv, tv, from_logits=logits, mask=maskd, reduction="none")
    with aten_form():
        aten = kl_divergence(xv, tv, from_logits=logits, mask=maskd, reduction="none")
    assert len(native_calls) == 1
    large = np.array(lowest + [False])
    assert int(large.sum()) == (3 if logits else 0) and np.isfinite(want[large]).all()
    small = torch.from_numpy(~large).to(DEV)
    check_rows(got[small], aten[small], want[~large], f"special rows {dtype}")
    if logits:
        assert bool(torch.isfinite(got[~small]).all())
        check_rows(got[~small], aten[~small], want[large], f"special rows {dtype}, lowest finite value in input")
    # a reduced value takes NaN from its rows, and inf where no row is NaN
    assert bool(kl_divergence(xv, tv, from_logits=logits, mask=maskd).isnan())
    keep = torch.from_numpy(~np.isnan(want)).to(DEV) & maskd
    for red in ("sum", "mean"):
        assert float(kl_divergence(xv, tv, from_logits=logits, mask=keep, reduction=red)) == float("inf")
    m = KLDivergence(from_logits=logits, device=DEV).update(xv, tv, mask=keep)
    assert float(m.compute()) == float("inf") and float(m.num_rows) == float(keep.sum())
    fin = torch.from_numpy(np.isfinite(want) & ~large).to(DEV) & maskd
    check(xv, tv, np.where(fin.cpu().numpy(), want, 0.0), logits, f"special rows {dtype}, the finite ones", fin)


def test_the_op_refuses_rows_at_different_offsets():
    """The wrapper sends such a pair to the ATen form.  A traced call cannot see addresses and calls
    the op, which checks them on the host before any launch and raises."""
    x, t = pair(5, 65, 165, True, torch.float32)
    xv, tv = offset_view(x, 1), offset_view(t, 2)
    assert not K.supported(xv, tv)
    out = torch.empty(5, device=DEV)
    with pytest.raises(RuntimeError, match="one offset from a 16-byte boundary"):
        torch.ops.torcheval_amd_kldiv.kl_batch(xv, tv, None, True, 0, out)
    s, n = torch.zeros((), dtype=torch.float64, device=DEV), torch.zeros((), dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="one offset from a 16-byte boundary"):
        torch.ops.torcheval_amd_kldiv.kl_update(xv, tv, None, True, s, n)
    assert float(s) == 0.0 and float(n) == 0.0


# ----------------------------------------------------------------------------- class
@pytest.mark.parametrize("c", [10, 300])
def test_class_update_is_one_native_op_and_no_aten_op(c, native_calls):
    """What an update dispatches: the K18 op (its two launches) and nothing else.  The states after
    four updates equal those of one update with all rows to FP64 rounding."""
    from torch.utils._python_dispatch import TorchDispatchMode

    from torcheval_amd.parallel.state_buffer import buffer_of

    seen = []

    class Recorder(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    x, t = pair(43, c, 400 + c, True, torch.float32)
    xd, td = x.to(DEV), t.to(DEV)
    mask = (torch.arange(43, device=DEV) % 5) != 0
    m = KLDivergence(device=DEV)
    sb = buffer_of(m)
    assert sb is not None
    ptrs = (m.kl_sum.data_ptr(), m.num_rows.data_ptr())
    parts = [(xd[lo:hi], td[lo:hi], mask[lo:hi]) for lo, hi in ((0, 4), (4, 5), (5, 42), (42, 43))]
    with Recorder():
        for i, (px, pt, pm) in enumerate(parts):
            m.update(px, pt, mask=pm if i % 2 == 0 else None)
    assert seen == ["torcheval_amd_kldiv.kl_update.default"] * 4, seen
    assert len(native_calls) == 4
    assert buffer_of(m, build=False) is sb and (m.kl_sum.data_ptr(), m.num_rows.data_ptr()) == ptrs
    used = torch.cat([pm if i % 2 == 0 else torch.ones_like(pm) for i, (_, _, pm) in enumerate(parts)])
    whole = KLDivergence(device=DEV).update(xd, td, mask=used)
    assert torch.equal(m.num_rows, whole.num_rows) and float(m.num_rows) == float(used.sum())
    torch.testing.assert_close(m.kl_sum, whole.kl_sum, rtol=2.0**-45, atol=0)
    got = m.compute()
    assert got.dtype == torch.float32 and got.is_cuda and got.shape == ()
    assert abs(float(got) - float(kl_divergence(xd, td, mask=used))) <= ulp32(float(got))
    moved = m.to("cpu")
    assert moved.kl_sum.device.type == "cpu" and float(moved.compute()) == float(got)
    m.reset()
    assert float(m.num_rows) == 0.0 and m.compute().isnan()


def _loop_data(i: int, c: int):
    g = torch.Generator(device=DEV).manual_seed(500 + i)
    x = torch.randn(256, c, device=DEV, generator=g) * 3
    t = x + torch.randn(256, c, device=DEV, generator=g)
    return x, t, torch.rand(256, device=DEV, generator=g) < 0.8


@pytest.mark.parametrize("c", [10, 300])
def test_compiled_update_loop_matches_eager(c):
    eager, comp = KLDivergence(device=DEV), KLDivergence(device=DEV)
    torch._dynamo.reset()

    @torch.compile(fullgraph=True)
    def step(x, t, mask):
        comp.update(x, t, mask=mask)

    counted = 0.0
    for i in range(4):
        x, t, mask = _loop_data(i, c)
        step(x, t, mask)
        eager.update(x, t, mask=mask)
        counted += float(mask.sum())
    assert torch.equal(comp.kl_sum, eager.kl_sum) and torch.equal(comp.num_rows, eager.num_rows)
    assert float(comp.num_rows) == counted
    torch.testing.assert_close(comp.compute(), eager.compute(), rtol=0, atol=0)


def test_compiled_graph_holds_the_dispatcher_op():
    m = KLDivergence(device=DEV)
    seen = []

    def backend(gm, example_inputs):
        seen.extend(str(n.target) for n in gm.graph.nodes if n.op == "call_function")
        return gm

    torch._dynamo.reset()
    step = torch.compile(lambda x, t: m.update(x, t), backend=backend, fullgraph=True)
    x, t, _ = _loop_data(0, 32)
    step(x, t)
    assert any("torcheval_amd_kldiv.kl_update" in s for s in seen), seen
    assert float(m.num_rows) == 256.0
