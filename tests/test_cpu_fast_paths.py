"""The small-batch CPU host calls (csrc/runtime/cpu_metrics.cpp: cpu_class_metric,
cpu_class_average, cpu_confusion, cpu_moments_update) and the no-context append / compute
paths, differential against the reference itself on random batches with missing classes, NaN
scores, ties, int32 targets and both input forms.  The reference's side of every comparison is
recorded in tests/golden/cpu_fast_paths.pt (tests/parity/gen_goldens.py writes it from
tests/parity/cpu_fast_cases.py, which also builds the inputs used here)."""

import logging
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "parity"))

import cpu_fast_cases as cases  # noqa: E402

from torcheval_amd import metrics as M  # noqa: E402
from torcheval_amd.metrics import functional as F  # noqa: E402
from torcheval_amd.ops import native_loaded  # noqa: E402

pytestmark = pytest.mark.skipif(not native_loaded(), reason="native build absent")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cpu_fast_paths.pt")
_batches = cases.batches


@pytest.fixture(scope="module")
def ref():
    """The reference's recorded results, by case key."""
    return torch.load(GOLDEN, weights_only=True)


def _same(a: torch.Tensor, b: torch.Tensor) -> None:
    assert a.dtype == b.dtype and a.shape == b.shape, (a, b)
    torch.testing.assert_close(a, b, equal_nan=True, rtol=2e-6, atol=1e-7)


@pytest.mark.parametrize("seed", cases.MACRO_WEIGHTED_SEEDS)
@pytest.mark.parametrize("fn,averages", cases.MACRO_WEIGHTED)
def test_macro_weighted_functionals_match_reference(ref, seed, fn, averages, caplog):
    calls = list(cases.macro_weighted_inputs(seed, averages))
    recorded = ref[f"macro_weighted/{fn}/{seed}"]
    assert len(recorded) == len(calls)
    for (avg, inp, tgt), rec in zip(calls, recorded):
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            ours = getattr(F, fn)(inp, tgt, num_classes=6, average=avg)
        ours_log = [r.getMessage() for r in caplog.records]
        if "raises" in rec:
            # the reference's recall divides the masked tp by the unmasked labels and
            # crashes once a class has neither labels nor predictions (docs/parity.md)
            assert fn == "multiclass_recall" and rec["raises"] == "RuntimeError"
            theirs, theirs_log = _masked_recall(inp, tgt, avg), ours_log
        else:
            theirs, theirs_log = rec["value"], rec["log"]
        _same(ours, theirs)
        assert ours_log == theirs_log


def _masked_recall(inp, tgt, avg):
    pred = inp.argmax(1) if inp.ndim == 2 else inp
    tp = torch.zeros(6).index_add_(0, tgt, (pred == tgt).float())
    lab = torch.zeros(6).index_add_(0, tgt, torch.ones(len(tgt)))
    prd = torch.zeros(6).index_add_(0, pred, torch.ones(len(pred)))
    mask = (lab != 0) | (prd != 0)
    r = torch.nan_to_num(tp[mask] / lab[mask])
    return r.mean() if avg == "macro" else (r * (lab[mask] / lab.sum())).sum()


@pytest.mark.parametrize("k", cases.TOP_K)
def test_macro_accuracy_top_k(ref, k):
    scores, target, _ = _batches(11)
    _same(F.multiclass_accuracy(scores, target, average="macro", num_classes=6, k=k), ref[f"top_k/{k}"])


def test_out_of_range_labels_still_raise_the_reference_errors():
    scores, target, labels = _batches(1)
    bad = target.clone()
    bad[3] = 6
    for fn in ("multiclass_f1_score", "multiclass_precision", "multiclass_recall"):
        with pytest.raises(Exception):
            getattr(F, fn)(scores, bad, num_classes=6, average="macro")
    with pytest.raises(ValueError, match="larger than the number of classes"):
        F.multiclass_confusion_matrix(scores, bad, num_classes=6)
    with pytest.raises(ValueError, match="too large for the number of classes"):
        F.multiclass_confusion_matrix(torch.tensor([0, 7]), torch.tensor([0, 1]), num_classes=6)
    with pytest.raises(RuntimeError):  # empty batch: the reference's torch.max raises too
        F.multiclass_confusion_matrix(torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.long), num_classes=6)


@pytest.mark.parametrize("seed", cases.CONFUSION_SEEDS)
def test_confusion_functionals_match_reference(ref, seed):
    calls = list(cases.confusion_inputs(seed))
    recorded = ref[f"confusion/{seed}"]
    assert len(recorded) == len(calls) == 7
    for (name, args, kwargs), theirs in zip(calls, recorded):
        _same(getattr(F, name)(*args, **kwargs), theirs)


@pytest.mark.parametrize("cls,kw", cases.CLASS_CASES)
def test_class_computes_match_reference(ref, cls, kw):
    ours, recorded = getattr(M, cls)(**kw), iter(ref[cases.class_key(cls, kw)])
    first, second = cases.class_updates(cls)
    assert len(first) == 3 and len(second) == 1 and len(ref[cases.class_key(cls, kw)]) == 4
    for run in (first, second):
        for scores, target in run:
            ours.update(scores, target)
            _same(ours.compute(), next(recorded).to(ours.compute().dtype))
        ours.reset()


def test_confusion_compute_is_not_aliased_into_a_state_buffer():
    m = M.MulticlassConfusionMatrix(4)
    m.update(torch.tensor([0, 1, 2]), torch.tensor([0, 1, 1]))
    out = m.compute()
    assert out is m.confusion_matrix  # the reference hands out the state itself
    assert out.sum().item() == 3


@pytest.mark.parametrize("shape", cases.REGRESSION_SHAPES)
@pytest.mark.parametrize("weighted", [False, True])
def test_regression_class_updates_match_reference(ref, shape, weighted):
    rec = ref[cases.regression_key(shape, weighted)]
    ours_mse, ours_r2 = M.MeanSquaredError(), M.R2Score()
    for x, t, w in cases.regression_updates(shape, weighted):
        if weighted:
            ours_mse.update(x, t, sample_weight=w)
        else:
            ours_mse.update(x, t)
        if shape[0] >= 2:
            ours_r2.update(x, t)
    for a, b in ((ours_mse.sum_squared_error, rec["sum_squared_error"]), (ours_mse.sum_weight, rec["sum_weight"])):
        _same(a, torch.as_tensor(b).to(a.dtype))
    _same(ours_mse.compute(), rec["mse"])
    assert ("r2" in rec) == (shape[0] >= 2)
    if shape[0] >= 2:
        for name in cases.R2_STATES:
            a = getattr(ours_r2, name)
            _same(a, torch.as_tensor(rec[name]).to(a.dtype))
        _same(ours_r2.compute(), rec["r2"])


@pytest.mark.parametrize("cls", cases.SAMPLE_STORE_CLASSES)
def test_sample_store_appends_keep_the_callers_tensors(ref, cls):
    ours = getattr(M, cls)()
    for x, y in cases.sample_store_updates():
        ours.update(x, y)
        assert ours.inputs[-1] is x and ours.targets[-1] is y  # the reference's no-op .to
    _same(ours.compute(), ref[f"sample_store/{cls}"])
    with pytest.raises(ValueError):
        ours.update(torch.rand(3), torch.rand(4))
    state = ours.state_dict()
    assert len(state["inputs"]) == 4


def test_binary_auroc_unweighted_placeholder_is_shared_and_not_an_inference_tensor():
    m = M.BinaryAUROC()
    with torch.inference_mode():
        m.update(torch.rand(4), torch.randint(0, 2, (4,)))
    m.update(torch.rand(4), torch.randint(0, 2, (4,)))
    assert m.weights[0] is m.weights[1]
    assert m.weights[0].numel() == 0 and not m.weights[0].is_inference()
    m.compute()
