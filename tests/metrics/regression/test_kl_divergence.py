"""KL divergence on the CPU (the ATen form) against the numpy FP64 oracle of the definition
(tests/_kl_oracle.py, docs/parity.md "Not in the reference").

Tolerance.  The float32 form sums ``p_j (log p_j - log q_j)`` with weights ``p_j`` that sum to 1.
Inputs are drawn with ``|logit| <= 8`` and at most 1000 columns, so every log-probability lies in
``(-32, 0]`` and its float32 is within one ulp of that range, 2^-19 = 1.9e-6, of the exact value.
Two of them meet in every term, so a row is within 3.8e-6 of the oracle plus the rounding of the
products and of the sum, which is relative: ``ATOL = 4e-6``, ``RTOL = 1e-6``.  Float64 operands are
held to 1e-12.  ``inf`` must match ``inf`` and NaN must match NaN exactly.
"""

import math
import os
import re

import numpy as np
import pytest
import torch

import torcheval_amd.metrics as M
import torcheval_amd.metrics.functional as MF
import torcheval_amd.metrics.functional.regression as MFR
import torcheval_amd.metrics.regression as MR
import torcheval_amd.ops as ops
from tests import _kl_oracle as O
from torcheval_amd.metrics import KLDivergence
from torcheval_amd.metrics.functional import kl_divergence
from torcheval_amd.utils.test_utils import MetricClassTester
from torcheval_amd.utils.test_utils.dist_pool import run_distributed

ATOL, RTOL = 4e-6, 1e-6
INF, NAN = math.inf, math.nan
REDUCTIONS = ("none", "sum", "mean")


def case(shape, seed: int, logits: bool = True, dtype=torch.float32):
    """Seeded ``(input, target)`` of ``shape``: logits within [-8, 8], or weights that do not sum
    to 1, already in ``dtype``."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(*shape, generator=g, dtype=torch.float64) * 3).clamp(-8, 8)
    t = (x + torch.randn(*shape, generator=g, dtype=torch.float64)).clamp(-8, 8)
    if not logits:
        x, t = torch.softmax(x, -1) * 3.0, torch.softmax(t, -1) * 0.5
    return x.to(dtype), t.to(dtype)


def check(got: torch.Tensor, want, dtype=torch.float32):
    """Exact on NaN and inf, within the tolerance elsewhere, and of the promised dtype and shape."""
    want = np.asarray(want, dtype=np.float64)
    assert got.dtype == dtype and tuple(got.shape) == want.shape, (got.dtype, got.shape, want.shape)
    g = got.double().numpy()
    assert np.array_equal(np.isnan(g), np.isnan(want)), (g, want)
    assert np.array_equal(np.isinf(g), np.isinf(want)) and np.array_equal(g[np.isinf(g)], want[np.isinf(want)])
    fin = np.isfinite(want)
    tol = (1e-12, 1e-12) if dtype == torch.float64 else (ATOL, RTOL)
    assert np.all(np.abs(g[fin] - want[fin]) <= tol[0] + tol[1] * np.abs(want[fin])), (g, want)


# ----------------------------------------------------------------------------- values
def test_rows_worked_by_hand():
    # p = (1/2, 1/2), q = (1/4, 3/4): (1/2) ln 2 + (1/2) ln (2/3)
    t = torch.tensor([[0.5, 0.5], [0.25, 0.75], [0.0, 1.0]])
    x = torch.tensor([[0.25, 0.75], [0.25, 0.75], [0.5, 0.5]])
    want = [0.5 * math.log(2) + 0.5 * math.log(2 / 3), 0.0, math.log(2)]
    check(kl_divergence(x, t, from_logits=False, reduction="none"), want)
    check(kl_divergence(x, t, from_logits=False, reduction="sum"), sum(want))
    check(kl_divergence(x, t, from_logits=False), sum(want) / 3)
    # the same distributions as logits: log of the weights, -inf for the zero
    check(kl_divergence(x.log(), t.log(), reduction="none"), want)
    # unnormalised weights: (1, 1) against (1, 3)
    check(kl_divergence(torch.tensor([1.0, 3.0]), torch.tensor([1.0, 1.0]), from_logits=False), want[0])
    # the direction: KL(P || Q) with P from target, as F.kl_div(log q, p)
    ref = torch.nn.functional.kl_div(x[:2].log(), t[:2], reduction="none").sum(-1)
    check(kl_divergence(x[:2], t[:2], from_logits=False, reduction="none"), ref.numpy())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16, torch.float64])
@pytest.mark.parametrize("logits", [True, False])
def test_modes_reductions_and_dtypes_against_the_oracle(logits, dtype):
    out_dtype = torch.float64 if dtype == torch.float64 else torch.float32
    for shape, seed in (((1, 1), 1), ((5, 2), 2), ((37, 3), 3), ((64, 33), 4), ((64, 1000), 5)):
        x, t = case(shape, seed, logits, dtype)
        g = torch.Generator().manual_seed(seed)
        mask = torch.rand(shape[0], generator=g) < 0.7
        for m in (None, mask):
            for red in REDUCTIONS:
                want = O.value(x.double().numpy(), t.double().numpy(), logits, None if m is None else m.numpy(), red)
                check(kl_divergence(x, t, from_logits=logits, mask=m, reduction=red), want, out_dtype)


def test_mixed_dtypes_promote():
    x, t = case((9, 17), 6)
    want = O.value(x.half().double().numpy(), t.double().numpy(), True)
    check(kl_divergence(x.half(), t), want)
    check(kl_divergence(x.half(), t.double()), want, torch.float64)


def test_log_probabilities_in_logits_mode_equal_probabilities():
    x, t = case((12, 40), 7)
    p, q = torch.softmax(t, -1), torch.softmax(x, -1)
    a = kl_divergence(q.log(), p.log(), reduction="none")
    b = kl_divergence(q, p, from_logits=False, reduction="none")
    c = kl_divergence(x, t, reduction="none")
    want = O.rows(x.numpy(), t.numpy(), True)
    for got in (a, b, c):
        check(got, want)


def test_nearly_equal_distributions_keep_sign_and_size():
    """KL about 1e-6: the tolerance's floor is absolute, so this checks sign and size only (the
    value is not negative beyond the tolerance and stays below 1e-5)."""
    x, _ = case((8, 100), 8)
    t = x + 2e-3 * torch.sin(torch.arange(100.0))
    want = O.rows(x.numpy(), t.numpy(), True)
    assert 0 < want.max() < 5e-6
    got = kl_divergence(x, t, reduction="none")
    check(got, want)
    assert float(got.min()) > -ATOL and float(got.max()) < 1e-5


# ----------------------------------------------------------------------------- special values
@pytest.mark.parametrize("logits", [True, False])
def test_special_values_one_row_each(logits):
    for name, x, t, want in O.special_rows(logits, 6, 2):
        x, t = torch.from_numpy(x), torch.from_numpy(t)
        got = kl_divergence(x[None], t[None], from_logits=logits, reduction="none")
        check(got, [want])
        # next to an ordinary row, the reduced values take the special one by the arithmetic
        gx, gt = case((1, 6), 11, logits)
        x2, t2 = torch.cat([gx, x[None]]), torch.cat([gt, t[None]])
        for red in ("sum", "mean"):
            check(kl_divergence(x2, t2, from_logits=logits, reduction=red),
                  O.value(x2.numpy(), t2.numpy(), logits, None, red))
        m = KLDivergence(from_logits=logits).update(x2, t2)
        check(m.compute(), O.value(x2.numpy(), t2.numpy(), logits))


@pytest.mark.parametrize("logits", [True, False])
def test_masked_rows_full_of_nan_change_nothing(logits):
    x, t = case((6, 9), 12, logits)
    mask = torch.tensor([True, False, True, True, False, True])
    dirty_x, dirty_t = x.clone(), t.clone()
    dirty_x[~mask], dirty_t[~mask] = NAN, -INF
    for red in REDUCTIONS:
        a = kl_divergence(x, t, from_logits=logits, mask=mask, reduction=red)
        b = kl_divergence(dirty_x, dirty_t, from_logits=logits, mask=mask, reduction=red)
        assert torch.equal(a, b) and not a.isnan().any()
        check(a, O.value(x.numpy(), t.numpy(), logits, mask.numpy(), red))
    assert kl_divergence(x, t, from_logits=logits, mask=mask, reduction="none")[~mask].eq(0).all()
    m = KLDivergence(from_logits=logits).update(dirty_x, dirty_t, mask=mask)
    assert float(m.num_rows) == 4.0
    check(m.compute(), O.value(x.numpy(), t.numpy(), logits, mask.numpy()))


# ----------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("logits", [True, False])
def test_strided_and_batched_inputs(logits):
    x, t = case((12, 7), 13, logits)
    want = kl_divergence(x, t, from_logits=logits, reduction="none")
    big_x, big_t = torch.zeros(12, 11), torch.zeros(24, 9)
    big_x[:, 2:9] = x
    big_t[::2, 1:8] = t
    assert torch.equal(kl_divergence(big_x[:, 2:9], big_t[::2, 1:8], from_logits=logits, reduction="none"), want)
    xt = x.t().contiguous().t()  # a column-major view
    assert torch.equal(kl_divergence(xt, t, from_logits=logits, reduction="none"), want)
    x3, t3 = x.reshape(3, 4, 7), t.reshape(3, 4, 7)
    mask = torch.rand(3, 4, generator=torch.Generator().manual_seed(1)) < 0.6
    got = kl_divergence(x3, t3, from_logits=logits, mask=mask, reduction="none")
    assert got.shape == (3, 4)
    check(got, O.rows(x3.numpy(), t3.numpy(), logits, mask.numpy()))
    check(kl_divergence(x3, t3, from_logits=logits, mask=mask),
          O.value(x3.numpy(), t3.numpy(), logits, mask.numpy()))
    # one row: [C] operands, a scalar result and a scalar mask
    one = kl_divergence(x[0], t[0], from_logits=logits, reduction="none")
    assert one.shape == () and torch.equal(one, want[0])
    assert float(kl_divergence(x[0], t[0], from_logits=logits, mask=torch.tensor(False), reduction="sum")) == 0.0


# ----------------------------------------------------------------------------- validation
def test_invalid_arguments():
    x, t = case((4, 6), 14)
    with pytest.raises(ValueError, match="same shape"):
        kl_divergence(x, t[:3])
    with pytest.raises(ValueError, match="same shape"):
        KLDivergence().update(x, t[:, :5])
    with pytest.raises(ValueError, match="at least one dimension"):
        kl_divergence(torch.tensor(1.0), torch.tensor(1.0))
    with pytest.raises(ValueError, match="at least one column"):
        kl_divergence(torch.rand(3, 0), torch.rand(3, 0))
    for bad in (torch.ones(4, dtype=torch.int64), torch.ones(3, dtype=torch.bool), torch.ones(4, 6, dtype=torch.bool),
                torch.ones(4)):
        with pytest.raises(ValueError, match="`mask` should be a bool tensor"):
            kl_divergence(x, t, mask=bad)
        with pytest.raises(ValueError, match="`mask` should be a bool tensor"):
            KLDivergence().update(x, t, mask=bad)
    with pytest.raises(ValueError, match="`reduction` should be one of"):
        kl_divergence(x, t, reduction="batchmean")
    for cast in (torch.int64, torch.int32, torch.bool, torch.uint8):
        with pytest.raises(ValueError, match="floating-point"):
            kl_divergence(x.to(cast), t)
        with pytest.raises(ValueError, match="floating-point"):
            kl_divergence(x, t.to(cast))
        with pytest.raises(ValueError, match="floating-point"):
            KLDivergence().update(x.to(cast), t.to(cast))


def test_empty_inputs():
    for shape in ((0, 5), (0, 0), (2, 0, 5)):
        e = torch.rand(*shape)
        out = kl_divergence(e, e)
        assert out.dtype == torch.float32 and out.shape == () and out.isnan()
        assert float(kl_divergence(e, e, reduction="sum")) == 0.0
        assert kl_divergence(e, e, reduction="none").shape == shape[:-1]
    x, t = case((5, 4), 15)
    none = torch.zeros(5, dtype=torch.bool)
    assert kl_divergence(x, t, mask=none).isnan() and float(kl_divergence(x, t, mask=none, reduction="sum")) == 0.0
    m = KLDivergence()
    assert m.compute().isnan() and m.compute().dtype == torch.float32
    m.update(x, t)
    before = m.state_dict()
    m.update(torch.rand(0, 4), torch.rand(0, 4))
    m.update(x, t, mask=none)  # no counted row: a no-op
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k])


# ----------------------------------------------------------------------------- class protocol
class TestKLDivergence(MetricClassTester):
    def _run(self, logits: bool, masked: bool) -> None:
        x, t = case((8, 6, 7), 16, logits)
        kwargs = {"input": x, "target": t}
        mask = None
        if masked:
            mask = torch.rand(8, 6, generator=torch.Generator().manual_seed(2)) < 0.7
            kwargs["mask"] = mask
        want = O.value(x.numpy(), t.numpy(), logits, None if mask is None else mask.numpy())
        self.run_class_implementation_tests(
            metric=KLDivergence(from_logits=logits),
            state_names={"kl_sum", "num_rows"},
            update_kwargs=kwargs,
            compute_result=torch.tensor(want).float(),
            atol=ATOL,
            rtol=RTOL,
        )

    def test_class_suite_logits(self) -> None:
        self._run(True, False)

    def test_class_suite_weights_masked(self) -> None:
        self._run(False, True)


@pytest.mark.parametrize("logits", [True, False])
def test_four_updates_equal_one_functional_call(logits):
    x, t = case((22, 65), 17, logits)
    mask = torch.rand(22, generator=torch.Generator().manual_seed(3)) < 0.8
    m = KLDivergence(from_logits=logits)
    for lo, hi in ((0, 1), (1, 9), (9, 10), (10, 22)):
        m.update(x[lo:hi], t[lo:hi], mask=mask[lo:hi])
    assert all(s.dtype == torch.float64 and s.shape == () for s in (m.kl_sum, m.num_rows))
    assert float(m.num_rows) == float(mask.sum())
    got = m.compute()
    assert got.dtype == torch.float32 and got.shape == ()
    check(got, O.value(x.numpy(), t.numpy(), logits, mask.numpy()))
    assert abs(float(got) - float(kl_divergence(x, t, from_logits=logits, mask=mask))) <= 2.0**-22


def test_merge_reset_state_dict():
    x, t = case((30, 6), 18)
    want = O.value(x.numpy(), t.numpy(), True)
    a = KLDivergence().update(x[:11], t[:11])
    b = KLDivergence().update(x[11:], t[11:])
    a.merge_state([b])
    assert float(a.num_rows) == 30.0 and float(b.num_rows) == 19.0
    check(a.compute(), want)
    c = KLDivergence()
    c.load_state_dict(a.state_dict())
    assert torch.equal(c.compute(), a.compute())
    assert set(a.state_dict()) == {"kl_sum", "num_rows"}
    a.reset()
    assert float(a.kl_sum) == 0.0 and float(a.num_rows) == 0.0 and a.compute().isnan()
    check(a.update(x, t).compute(), want)
    assert a._state_merge_kinds() == {"kl_sum": "sum", "num_rows": "sum"}


def _sync_job(rank: int, ws: int):
    from torcheval_amd.metrics.toolkit import sync_and_compute

    x, t = case((30, 6), 19)
    m = KLDivergence()
    if rank == 0:
        m.update(x, t)  # rank 1 never updates
    return sync_and_compute(m)


def test_two_rank_sync_and_compute_with_an_idle_rank():
    x, t = case((30, 6), 19)
    results = run_distributed(_sync_job, 2)
    assert results[0] is not None  # rank 0 is the recipient
    for got in results:
        if got is not None:
            check(got, O.value(x.numpy(), t.numpy(), True))


# ----------------------------------------------------------------------------- exports, routing
def test_exports():
    for mod in (M, MR):
        assert mod.KLDivergence is KLDivergence
        assert "KLDivergence" not in mod.__all__
    for mod in (MF, MFR):
        assert mod.kl_divergence is kl_divergence
        assert "kl_divergence" not in mod.__all__
    assert MR.__doc_extras__ == ["KLDivergence"] and MFR.__doc_extras__ == ["kl_divergence"]


def test_wrapper_constants_match_the_header():
    from torcheval_amd.ops import kl_divergence as K

    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    with open(os.path.join(root, "csrc", "include", "tea_kernels.h")) as fh:
        header = fh.read()
    with open(os.path.join(root, "csrc", "kernels", "kl_divergence.hip")) as fh:
        kernel = fh.read()
    assert K.MAX_BLOCKS == int(re.search(r"constexpr int kKlMaxBlocks = (\d+);", header).group(1))
    block = int(re.search(r"constexpr int kB = (\d+);", kernel).group(1))
    assert K.WAVES_PER_BLOCK == block // 64
    assert K.ROWS_PER_LAUNCH == K.MAX_BLOCKS * K.WAVES_PER_BLOCK


@pytest.mark.skipif(not ops.native_loaded(), reason="extension not built")
def test_native_op_surface_and_compiled_route(monkeypatch):
    """K18's two ops: their schemas, which dispatch keys hold a kernel, Meta kernels that return
    None, and the wrapper on meta tensors with ``compiling`` forced."""
    from torcheval_amd.ops import kl_divergence as K

    ns = "torcheval_amd_kldiv::"
    names = sorted(n for n in torch._C._dispatch_get_all_op_names() if n.startswith(ns))
    assert names == [ns + "kl_batch", ns + "kl_update"]
    lib = torch.ops.torcheval_amd_kldiv
    assert str(lib.kl_update.default._schema) == (
        ns + "kl_update(Tensor input, Tensor target, Tensor? mask, bool from_logits, Tensor(a!) kl_sum, "
        "Tensor(b!) num_rows) -> ()")
    assert str(lib.kl_batch.default._schema) == (
        ns + "kl_batch(Tensor input, Tensor target, Tensor? mask, bool from_logits, int reduction, "
        "Tensor(a!) out) -> ()")
    for name in names:
        has = [k for k in ("CPU", "CUDA", "Meta") if torch._C._dispatch_has_kernel_for_dispatch_key(name, k)]
        assert has == ["CUDA", "Meta"]
    monkeypatch.setattr(ops, "compiling", lambda: True)
    meta = torch.device("meta")
    x, t = torch.empty(4, 5, 9, device=meta), torch.empty(4, 5, 9, device=meta)
    mask = torch.empty(4, 5, dtype=torch.bool, device=meta)
    s = [torch.empty((), dtype=torch.float64, device=meta) for _ in range(2)]
    assert K.kl_update(x, t, mask, True, *s) is None
    for red, shape in (("none", (4, 5)), ("sum", ()), ("mean", ())):
        out = K.kl_batch(x, t, None, False, red)
        assert out.shape == shape and out.dtype == torch.float32 and out.device.type == "meta"
