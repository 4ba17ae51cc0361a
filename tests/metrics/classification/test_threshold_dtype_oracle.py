"""Threshold decisions of the binary / multilabel metrics on the CPU, per score dtype.

ATen compares ``input < threshold`` in the input's dtype: the Python threshold is cast to it
first, so ``bf16(0.69921875) < 0.7`` is False (bf16(0.7) == 0.69921875).  The oracle
(tests/_threshold_edges.py) is that plain ATen expression plus int64 counts; the package's CPU
paths - the host twins and, with ``ops.DISABLE_HIP`` set, the ATen chains - must equal it.  The
edge inputs are also checked to tell that semantics apart from a float32 compare, which is what
the GPU tests (tests/gpu/test_threshold_dtype_edges.py) rely on.
"""

import pytest
import torch

import torcheval_amd.ops as ops
from tests._threshold_edges import (
    CRITERIA,
    FLOAT_DTYPES,
    INT_DTYPES,
    THRESHOLDS,
    binary_formulas,
    binary_targets,
    dtype_id,
    edge_scores,
    float32_model_pred,
    multilabel_formula,
    multilabel_targets,
    oracle_pred,
)
from torcheval_amd import metrics as M
from torcheval_amd.metrics import functional as F

N = 4099
BINARY = {
    "accuracy": (F.binary_accuracy, M.BinaryAccuracy),
    "precision": (F.binary_precision, M.BinaryPrecision),
    "recall": (F.binary_recall, M.BinaryRecall),
    "f1_score": (F.binary_f1_score, M.BinaryF1Score),
    "confusion_matrix": (F.binary_confusion_matrix, M.BinaryConfusionMatrix),
}
ML_SHAPES = ((1, 1), (37, 5), (129, 101))
_EXACT_IN_F32 = (0.5, 0.0, 1.0, -0.25)


def _check(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    # counts stay below 2**24, so the oracle's int64 counts are exact in the package's dtype
    torch.testing.assert_close(got.cpu(), want.to(got.dtype), msg=lambda m: f"{what}: {m}")


# ------------------------------------------------------------------ the inputs themselves
@pytest.mark.parametrize("dtype", FLOAT_DTYPES + INT_DTYPES, ids=dtype_id)
@pytest.mark.parametrize("n", [1, 63, 4099])
def test_edge_scores_shape_and_content(dtype, n):
    x = edge_scores(dtype, 0.7, n, seed=3)
    assert x.dtype == dtype and x.shape == (n,) and x.is_contiguous()
    assert torch.equal(x.view(torch.uint8), edge_scores(dtype, 0.7, n, seed=3).view(torch.uint8))  # seeded
    if n >= 63:
        if dtype.is_floating_point:
            tv = torch.tensor(0.7, dtype=dtype)
            up = torch.tensor(float("inf"), dtype=dtype)
            for v in (tv, torch.nextafter(tv, up), torch.nextafter(tv, -up), torch.tensor(1.0, dtype=dtype), up, -up):
                assert bool((x == v).any()), float(v)
            assert bool(x.isnan().any())
            assert bool(((x == 0) & x.signbit()).any()) and bool(((x == 0) & ~x.signbit()).any())  # -0.0, 0.0
        else:
            assert bool((x == 0).any()) and bool((x == 1).any())


@pytest.mark.parametrize("dtype,thr", [
    (torch.bfloat16, 0.7), (torch.bfloat16, 0.9), (torch.float16, 0.1), (torch.float16, 0.9),
    (torch.float64, 0.7), (torch.float64, 0.3),
], ids=lambda v: dtype_id(v) if isinstance(v, torch.dtype) else str(v))
def test_edges_tell_a_float32_compare_from_aten(dtype, thr):
    x = edge_scores(dtype, thr, 63, seed=11)
    assert not torch.equal(float32_model_pred(x, thr), oracle_pred(x, thr))
    tv = torch.tensor(thr, dtype=dtype)
    if dtype != torch.float64:
        # the predicted place: x == dtype(thr) is positive in ATen, negative in float32
        at = x == tv
        assert bool(at.any()) and bool((oracle_pred(x, thr)[at] == 1).all())
        assert bool((float32_model_pred(x, thr)[at] == 0).all())


@pytest.mark.parametrize("thr", THRESHOLDS, ids=str)
@pytest.mark.parametrize("dtype", FLOAT_DTYPES, ids=dtype_id)
def test_float32_compare_agrees_where_it_should(dtype, thr):
    """A float32 compare is ATen's for float32 scores at every threshold, and for bf16 / f16
    scores at thresholds every dtype holds exactly.  float64 scores at such a threshold: the two
    can only differ on scores float32 does not hold (the float64 neighbours of the threshold,
    which round onto it), and they do differ there - a float32 compare of float64 scores is
    wrong at every threshold, not only at the inexact ones."""
    x = edge_scores(dtype, thr, 63, seed=12)
    differ = float32_model_pred(x, thr) != oracle_pred(x, thr)
    if dtype == torch.float32:
        assert not bool(differ.any())
    elif thr in _EXACT_IN_F32:
        if dtype == torch.float64:
            held = x.float().double() == x
            assert not bool((differ & held).any())
            assert bool(differ.any())
        else:
            assert not bool(differ.any())


# ------------------------------------------------------------------ the package's CPU paths
@pytest.fixture(params=["native", "aten"])
def cpu_path(request, monkeypatch):
    """Each case once as is (host twins where they apply) and once on the ATen chains."""
    monkeypatch.setattr(ops, "DISABLE_HIP", request.param == "aten")
    return request.param


@pytest.mark.parametrize("thr", THRESHOLDS, ids=str)
@pytest.mark.parametrize("dtype", FLOAT_DTYPES, ids=dtype_id)
def test_binary_cpu_paths_equal_oracle(dtype, thr, cpu_path):
    x = edge_scores(dtype, thr, N, seed=21)
    t = binary_targets(N, seed=21)
    want = binary_formulas(oracle_pred(x, thr), t)
    half = N // 2
    for name, (fn, cls) in BINARY.items():
        _check(fn(x, t, threshold=thr), want[name], f"binary_{name}")
        m = cls(threshold=thr)
        m.update(x[:half], t[:half])
        m.update(x[half:], t[half:])
        _check(m.compute(), want[name], cls.__name__)


@pytest.mark.parametrize("dtype", INT_DTYPES, ids=dtype_id)
def test_binary_cpu_integer_scores_equal_oracle(dtype, cpu_path):
    # integer / bool scores against a Python float promote to float32 in ATen
    for thr in (0.5, 0.0, 1.0, -0.25):
        x = edge_scores(dtype, thr, 257, seed=22)
        t = binary_targets(257, seed=22)
        want = binary_formulas(oracle_pred(x, thr), t)
        _check(F.binary_accuracy(x, t, threshold=thr), want["accuracy"], "binary_accuracy")


@pytest.mark.parametrize("thr", THRESHOLDS, ids=str)
@pytest.mark.parametrize("dtype", FLOAT_DTYPES, ids=dtype_id)
def test_multilabel_cpu_paths_equal_oracle(dtype, thr, cpu_path):
    for shape in ML_SHAPES:
        n = shape[0] * shape[1]
        x = edge_scores(dtype, thr, n, seed=31).view(shape)
        pred = oracle_pred(x, thr)
        for tdt in (torch.int64, torch.bool):
            t = multilabel_targets(pred, seed=31, dtype=tdt)
            for criteria in CRITERIA:
                if tdt == torch.bool and criteria in ("contain", "belong"):
                    continue  # the CPU chain subtracts the target, which ATen refuses for bool (as the reference)
                want = multilabel_formula(pred, t, criteria)
                what = f"{criteria} {shape} {dtype_id(tdt)}"
                got = F.multilabel_accuracy(x, t, threshold=thr, criteria=criteria)
                torch.testing.assert_close(got, want, rtol=0, atol=1e-6, msg=lambda m: f"functional {what}: {m}")
                m = M.MultilabelAccuracy(threshold=thr, criteria=criteria)
                h = shape[0] // 2
                if h:
                    m.update(x[:h], t[:h])
                m.update(x[h:], t[h:])
                torch.testing.assert_close(m.compute(), want, rtol=0, atol=1e-6, msg=lambda m: f"class {what}: {m}")
