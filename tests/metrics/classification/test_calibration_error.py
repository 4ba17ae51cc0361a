"""Multiclass calibration error on the CPU (the ATen form) against the numpy FP64 oracle of the
definition (tests/_calibration_oracle.py, docs/parity.md "Not in the reference").

The oracle bins the float32 confidence it is given: for probabilities that is an input value, for
logits the float32 softmax maximum, so bin counts and correct counts must match exactly.  The three
values are at most 1 and both sides form them in FP64 from equal integer counts and confidence sums
that differ by FP64 rounding only, so ``|got - float32(oracle)| <= 2^-23``.
"""

import math
import os
import re

import numpy as np
import pytest
import torch

import torcheval_amd.metrics as M
import torcheval_amd.metrics.classification as MC
import torcheval_amd.metrics.functional as MF
import torcheval_amd.metrics.functional.classification as MFC
import torcheval_amd.ops as ops
from tests import _calibration_oracle as O
from torcheval_amd.metrics import MulticlassCalibrationError
from torcheval_amd.metrics.functional import multiclass_calibration_error
from torcheval_amd.utils.test_utils import MetricClassTester
from torcheval_amd.utils.test_utils.dist_pool import run_distributed

TOL = 2.0**-23
NORMS = ("l1", "max", "l2")
BINS = (1, 2, 10, 15, 100)


def case(n: int, c: int, seed: int, logits: bool = False, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, generator=g) * 3
    if not logits:
        x = torch.softmax(x, dim=1)
    x = x.to(dtype)
    # about half the rows labelled with their prediction, so that both outcomes fill the bins
    t = torch.where(torch.rand(n, generator=g) < 0.5, x.float().argmax(1), torch.randint(0, c, (n,), generator=g))
    return x, t


def oracle_states(x: torch.Tensor, t: torch.Tensor, n_bins: int, from_logits: bool):
    """The oracle on the float32 confidence as given (float64 input: its FP64 confidence)."""
    wide = x.dtype == torch.float64
    xs = x if wide else x.float()
    conf = torch.softmax(xs, dim=1).max(dim=1).values if from_logits else xs.max(dim=1).values
    return O.states(conf.numpy(), O.argmax_first(xs.numpy()), t.numpy(), n_bins)


def check_value(got: torch.Tensor, want: float):
    assert got.dtype == torch.float32 and got.shape == ()
    if math.isnan(want):
        assert got.isnan()
    else:
        assert abs(float(got) - float(np.float32(want))) <= TOL, (float(got), want)


def check_states(m: MulticlassCalibrationError, want):
    assert np.array_equal(m.bin_count.numpy(), want[0])
    assert np.array_equal(m.correct_sum.numpy(), want[1])
    np.testing.assert_allclose(m.conf_sum.numpy(), want[2], rtol=2.0**-45, atol=0)


# ----------------------------------------------------------------------------- values
def test_value_worked_by_hand():
    # confidences .75 .75 .5 1 .25, correct 1 0 1 0 1; two bins (0, .5] and (.5, 1]:
    # bin 0 holds rows 2, 4 (count 2, correct 2, conf .75), bin 1 rows 0, 1, 3 (3, 1, 2.5)
    x = torch.tensor([[0.75, 0.25, 0, 0], [0.25, 0.75, 0, 0], [0.5, 0.5, 0, 0], [0, 0, 1.0, 0], [0.25] * 4])
    t = torch.tensor([0, 0, 0, 3, 0])
    assert float(multiclass_calibration_error(x, t, n_bins=2)) == pytest.approx((1.25 + 1.5) / 5, abs=TOL)
    assert float(multiclass_calibration_error(x, t, n_bins=2, norm="max")) == 0.625
    want = math.sqrt(1.25**2 / (2 * 5) + 1.5**2 / (3 * 5))
    assert float(multiclass_calibration_error(x, t, n_bins=2, norm="l2")) == pytest.approx(want, abs=TOL)
    m = MulticlassCalibrationError(n_bins=2).update(x, t)
    assert m.bin_count.tolist() == [2.0, 3.0] and m.correct_sum.tolist() == [2.0, 1.0]
    assert m.conf_sum.tolist() == [0.75, 2.5]


@pytest.mark.parametrize("from_logits", [False, True])
@pytest.mark.parametrize("n_bins", BINS)
def test_norms_and_bins_against_the_oracle(n_bins, from_logits):
    for n, c, seed in ((1, 1, 1), (5, 2, 2), (37, 3, 3), (300, 17, 4), (64, 1000, 5)):
        x, t = case(n, c, seed, from_logits)
        want = oracle_states(x, t, n_bins, from_logits)
        m = MulticlassCalibrationError(n_bins=n_bins, from_logits=from_logits).update(x, t)
        check_states(m, want)
        assert m.bin_count.sum() == n
        for norm in NORMS:
            check_value(multiclass_calibration_error(x, t, n_bins=n_bins, norm=norm, from_logits=from_logits),
                        O.value(*want, norm))


@pytest.mark.parametrize("n_bins", [10, 15, 100])
def test_rows_on_the_edges_and_next_to_them(n_bins):
    """Every edge, the float32 above it and the one below it as a row's maximum: the table decides,
    where ``ceil(conf * n_bins) - 1`` in float32 would misplace some of them."""
    e = O.edges(n_bins)
    v = np.concatenate([e, np.nextafter(e, np.float32(2)), np.nextafter(e, np.float32(-1))])
    v = v[(v >= 0) & (v <= 1)]
    x = torch.zeros(len(v), 3)
    x[:, 1] = torch.from_numpy(v)
    t = torch.ones(len(v), dtype=torch.int64)
    t[::3] = 0
    m = MulticlassCalibrationError(n_bins=n_bins).update(x, t)
    check_states(m, O.states(v, O.argmax_first(x.numpy()), t.numpy(), n_bins))  # the all-zero row predicts 0
    naive = np.clip(np.ceil(v * np.float32(n_bins)).astype(np.int64) - 1, 0, n_bins - 1)
    if n_bins == 100:
        assert (naive != O.bins_of(v, n_bins)).sum() > 0  # the case the rule above exists for


def test_ties_take_the_lowest_index():
    x = torch.tensor([[0.4, 0.4, 0.2], [0.2, 0.4, 0.4]])
    m = MulticlassCalibrationError(n_bins=5).update(x, torch.tensor([0, 2]))
    assert m.correct_sum.sum() == 1.0  # row 0 predicts 0, row 1 predicts 1
    x = torch.tensor([[1.0, 1.0, -math.inf], [-math.inf, 0.0, 0.0]])
    m = MulticlassCalibrationError(n_bins=4, from_logits=True).update(x, torch.tensor([0, 1]))
    assert m.bin_count.tolist() == [0.0, 2.0, 0.0, 0.0] and m.correct_sum.tolist() == [0.0, 2.0, 0.0, 0.0]
    assert m.conf_sum.tolist() == [0.0, 1.0, 0.0, 0.0]  # -inf logits contribute 0: both rows 1 / 2


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64])
@pytest.mark.parametrize("from_logits", [False, True])
def test_score_dtypes(dtype, from_logits):
    x, t = case(50, 9, 6, from_logits, dtype)
    want = oracle_states(x, t, 15, from_logits)
    for tt in (t, t.int(), t.to(torch.int16), t.to(torch.uint8)):
        m = MulticlassCalibrationError(from_logits=from_logits).update(x, tt)
        check_states(m, want)
        check_value(multiclass_calibration_error(x, tt, from_logits=from_logits), O.value(*want, "l1"))


def test_sixteen_bit_probabilities_widen_exactly():
    x, t = case(40, 5, 7, False, torch.float16)
    assert torch.equal(multiclass_calibration_error(x, t), multiclass_calibration_error(x.float(), t))


def test_views_with_strides():
    x, t = case(12, 7, 8)
    big = torch.zeros(12, 11)
    big[:, 2:9] = x
    assert torch.equal(multiclass_calibration_error(big[:, 2:9], t), multiclass_calibration_error(x, t))
    assert torch.equal(multiclass_calibration_error(x.t().contiguous().t(), t), multiclass_calibration_error(x, t))


# ----------------------------------------------------------------------------- validation
def test_invalid_arguments():
    x, t = case(4, 6, 9)
    for bad in (0, -2, 2.5, True):
        with pytest.raises(ValueError, match="`n_bins` should be a positive integer"):
            multiclass_calibration_error(x, t, n_bins=bad)
        with pytest.raises(ValueError, match="`n_bins` should be a positive integer"):
            MulticlassCalibrationError(n_bins=bad)
    with pytest.raises(ValueError, match="`norm` should be one of"):
        multiclass_calibration_error(x, t, norm="linf")
    with pytest.raises(ValueError, match="`norm` should be one of"):
        MulticlassCalibrationError(norm="L1")
    with pytest.raises(ValueError, match="two-dimensional"):
        multiclass_calibration_error(x[0], t)
    with pytest.raises(ValueError, match="two-dimensional"):
        multiclass_calibration_error(x[None], t)
    with pytest.raises(ValueError, match="one-dimensional"):
        multiclass_calibration_error(x, t[:, None])
    with pytest.raises(ValueError, match="same first dimension"):
        multiclass_calibration_error(x, t[:3])
    with pytest.raises(ValueError, match="same first dimension"):
        MulticlassCalibrationError().update(x, t[:3])
    for tt in (t.float(), t.bool()):
        with pytest.raises(ValueError, match="integer labels"):
            multiclass_calibration_error(x, tt)
    with pytest.raises(ValueError, match="at least one class"):
        multiclass_calibration_error(torch.rand(3, 0), torch.zeros(3, dtype=torch.int64))


def test_bad_rows_raise_and_leave_the_states():
    x, t = case(6, 4, 10)
    lx, _ = case(6, 4, 10, True)
    nan, inf, ninf, big = x.clone(), lx.clone(), lx.clone(), x.clone()
    nan[2, 3] = math.nan
    inf[1, 0] = math.inf
    ninf[4] = -math.inf
    big[0, 1] = 1.5
    cases = [
        (x, t.clone().index_fill_(0, torch.tensor([3]), 4), False, "label outside"),
        (x, t.clone().index_fill_(0, torch.tensor([3]), -1), False, "label outside"),
        (nan, t, False, "confidence is not in"),
        (nan, t, True, "confidence is not in"),
        (inf, t, True, "confidence is not in"),
        (ninf, t, True, "confidence is not in"),
        (big, t, False, "confidence is not in"),
    ]
    for xi, ti, from_logits, msg in cases:
        with pytest.raises(ValueError, match=msg):
            multiclass_calibration_error(xi, ti, from_logits=from_logits)
        m = MulticlassCalibrationError(from_logits=from_logits).update(lx if from_logits else x, t)
        before = m.state_dict()
        with pytest.raises(ValueError, match=msg):
            m.update(xi, ti)
        for k, v in m.state_dict().items():
            assert torch.equal(v, before[k])
        assert not m.compute().isnan()
    both = nan.clone()
    with pytest.raises(ValueError, match="label outside.*; .*confidence is not in"):
        multiclass_calibration_error(both, torch.full((6,), 9))


def test_empty_inputs():
    for c in (0, 5):
        out = multiclass_calibration_error(torch.rand(0, c), torch.zeros(0, dtype=torch.int64))
        assert out.dtype == torch.float32 and out.shape == () and out.isnan()
    m = MulticlassCalibrationError()
    assert m.compute().isnan()
    x, t = case(9, 5, 11)
    m.update(x, t)
    before = m.state_dict()
    m.update(torch.rand(0, 5), torch.zeros(0, dtype=torch.int64))
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k])


# ----------------------------------------------------------------------------- class protocol
class TestMulticlassCalibrationError(MetricClassTester):
    def _run(self, norm: str, from_logits: bool) -> None:
        x, t = case(8 * 6, 7, 12, from_logits)
        want = torch.tensor(O.value(*oracle_states(x, t, 10, from_logits), norm)).float()
        self.run_class_implementation_tests(
            metric=MulticlassCalibrationError(n_bins=10, norm=norm, from_logits=from_logits),
            state_names={"bin_count", "correct_sum", "conf_sum"},
            update_kwargs={"input": x.reshape(8, 6, 7), "target": t.reshape(8, 6)},
            compute_result=want,
            atol=TOL,
            rtol=0,
        )

    def test_class_suite_ece(self) -> None:
        self._run("l1", False)

    def test_class_suite_mce_from_logits(self) -> None:
        self._run("max", True)

    def test_class_suite_rms(self) -> None:
        self._run("l2", False)


@pytest.mark.parametrize("norm", NORMS)
def test_four_updates_equal_one_functional_call(norm):
    x, t = case(22, 65, 13, True)
    m = MulticlassCalibrationError(norm=norm, from_logits=True)
    for lo, hi in ((0, 1), (1, 9), (9, 10), (10, 22)):
        m.update(x[lo:hi], t[lo:hi])
    assert all(s.dtype == torch.float64 and s.shape == (15,) for s in (m.bin_count, m.correct_sum, m.conf_sum))
    check_states(m, oracle_states(x, t, 15, True))
    got = m.compute()
    assert got.dtype == torch.float32 and got.shape == ()
    assert abs(float(got) - float(multiclass_calibration_error(x, t, norm=norm, from_logits=True))) <= TOL


def test_merge_reset_state_dict():
    x, t = case(30, 6, 14)
    want = O.value(*oracle_states(x, t, 15, False), "l1")
    a = MulticlassCalibrationError().update(x[:11], t[:11])
    b = MulticlassCalibrationError().update(x[11:], t[11:])
    a.merge_state([b])
    assert a.bin_count.sum() == 30 and b.bin_count.sum() == 19
    check_value(a.compute(), want)
    c = MulticlassCalibrationError()
    c.load_state_dict(a.state_dict())
    assert torch.equal(c.compute(), a.compute())
    a.reset()
    assert a.bin_count.sum() == 0 and a.conf_sum.sum() == 0 and a.compute().isnan()
    check_value(a.update(x, t).compute(), want)
    assert a._state_merge_kinds() == {"bin_count": "sum", "correct_sum": "sum", "conf_sum": "sum"}


def _sync_job(rank: int, ws: int):
    from torcheval_amd.metrics.toolkit import sync_and_compute

    x, t = case(30, 6, 15, True)
    lo, hi = (0, 13) if rank == 0 else (13, 30)
    return sync_and_compute(MulticlassCalibrationError(norm="l2", from_logits=True).update(x[lo:hi], t[lo:hi]))


def test_two_rank_sync_and_compute():
    x, t = case(30, 6, 15, True)
    results = run_distributed(_sync_job, 2)
    assert results[0] is not None  # rank 0 is the recipient
    want = O.value(*oracle_states(x, t, 15, True), "l2")
    for got in results:
        if got is not None:
            check_value(got, want)


# ----------------------------------------------------------------------------- exports, routing
def test_exports():
    for mod in (M, MC):
        assert mod.MulticlassCalibrationError is MulticlassCalibrationError
    for mod in (MF, MFC):
        assert mod.multiclass_calibration_error is multiclass_calibration_error
    # the top-level lists mirror the reference's public names and are built from the family lists
    for mod in (M, MC):
        assert "MulticlassCalibrationError" not in mod.__all__
    for mod in (MF, MFC):
        assert "multiclass_calibration_error" not in mod.__all__


def test_wrapper_constants_match_the_header():
    from torcheval_amd.ops import calibration as K

    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    with open(os.path.join(root, "csrc", "include", "tea_kernels.h")) as fh:
        header = fh.read()

    def const(name):
        return int(re.search(rf"constexpr int {name} = (\d+);", header).group(1))

    assert K.max_bins() == K.MAX_BINS == const("kCalibMaxBins")
    assert K.THREAD_ARM_MAX_COLUMNS == const("kCalibNarrowMaxC")
    assert K.rows_per_launch(33) == K.WAVE_ARM_ROWS_PER_LAUNCH == const("kCalibMaxBlocks") * 4
    assert K.rows_per_launch(32) == K.THREAD_ARM_ROWS_PER_LAUNCH == const("kCalibMaxBlocks") * 256


@pytest.mark.skipif(not ops.native_loaded(), reason="extension not built")
def test_native_op_surface_and_compiled_route(monkeypatch):
    """K15's three ops: their schemas, which dispatch keys hold a kernel, Meta kernels that return
    None, and the wrapper on meta tensors with ``compiling`` forced."""
    from torcheval_amd.ops import calibration as K

    names = sorted(n for n in torch._C._dispatch_get_all_op_names() if n.startswith("torcheval_amd_calibration::"))
    ns = "torcheval_amd_calibration::"
    assert names == [ns + "calibration_error", ns + "calibration_update", ns + "calibration_value"]
    lib = torch.ops.torcheval_amd_calibration
    assert str(lib.calibration_update.default._schema) == (
        ns + "calibration_update(Tensor input, Tensor target, int n_bins, bool from_logits, Tensor(a!) bin_count, "
        "Tensor(b!) correct_sum, Tensor(c!) conf_sum, Tensor(d!)? err) -> ()")
    assert str(lib.calibration_error.default._schema) == (
        ns + "calibration_error(Tensor input, Tensor target, int n_bins, bool from_logits, int norm, "
        "Tensor(a!) out, Tensor(b!)? err) -> ()")
    assert str(lib.calibration_value.default._schema) == (
        ns + "calibration_value(Tensor bin_count, Tensor correct_sum, Tensor conf_sum, int norm, Tensor(a!) out) -> ()")
    for name in names:
        has = [k for k in ("CPU", "CUDA", "Meta") if torch._C._dispatch_has_kernel_for_dispatch_key(name, k)]
        assert has == ["CUDA", "Meta"]
    monkeypatch.setattr(ops, "compiling", lambda: True)
    meta = torch.device("meta")
    x, t = torch.empty(4, 9, device=meta), torch.empty(4, dtype=torch.int64, device=meta)
    s = [torch.empty(15, dtype=torch.float64, device=meta) for _ in range(3)]
    err = torch.empty(1, dtype=torch.int32, device=meta)
    assert K.calibration_update(x, t, 15, True, *s, err) is None
    for out in (K.calibration_error(x, t, 15, False, "max", None), K.calibration_value(*s, "l2")):
        assert out.shape == () and out.dtype == torch.float32 and out.device.type == "meta"
