"""Segmentation mean IoU and Dice on the CPU (the ATen form) against the numpy oracle of the
definition (tests/_segmentation_oracle.py, docs/parity.md "Not in the reference").

The three counts are integers and must match exactly.  The values are at most 1 and both sides
form them in FP64 from equal counts, so ``|got - float32(oracle)| <= 2^-23``, NaN matching NaN.
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
from tests import _segmentation_oracle as O
from torcheval_amd.metrics import DiceScore, MeanIoU
from torcheval_amd.metrics.functional import dice_score, mean_iou
from torcheval_amd.utils.test_utils import MetricClassTester
from torcheval_amd.utils.test_utils.dist_pool import run_distributed

TOL = 2.0**-23
AVERAGES = ("macro", "micro", "none")
KINDS = ((mean_iou, MeanIoU, False), (dice_score, DiceScore, True))
STATES = ("intersection", "pred_count", "target_count")


def case(n: int, c: int, spatial, seed: int, dtype=torch.float32, ignore=None, classes_used=None):
    """Seeded scores and labels; about half the pixels labelled with their prediction, a tenth
    with ``ignore`` when given, and only the first ``classes_used`` classes ever labelled."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, c, *spatial, generator=g) * 3).to(dtype)
    used = c if classes_used is None else classes_used
    if used < c:
        x[:, used:] = -100.0
    pred = x.float().argmax(1)
    t = torch.where(torch.rand(pred.shape, generator=g) < 0.5, pred, torch.randint(0, used, pred.shape, generator=g))
    if ignore is not None:
        t = torch.where(torch.rand(pred.shape, generator=g) < 0.1, ignore, t)
    return x, t


def check_value(got: torch.Tensor, want, dtype=torch.float32):
    want = np.asarray(want, dtype=np.float64)
    assert got.dtype == dtype and tuple(got.shape) == want.shape, (got.dtype, got.shape)
    g = got.double().numpy()
    w = want.astype(np.float32).astype(np.float64) if dtype == torch.float32 else want
    assert np.array_equal(np.isnan(g), np.isnan(w)), (g, w)
    assert (np.abs(g - w)[~np.isnan(w)] <= TOL).all(), (g, w)


def check_counts(m, want):
    for name, w in zip(STATES, want):
        s = getattr(m, name)
        assert s.dtype == torch.float64 and np.array_equal(s.numpy(), w.astype(np.float64)), (name, s, w)


# ----------------------------------------------------------------------------- values
def test_value_worked_by_hand():
    # pred 0 0 1 1 2 2, target 0 1 1 1 2 255 (ignored); class 3 absent from both maps
    p = torch.tensor([[0, 0, 1, 1, 2, 2]])
    t = torch.tensor([[0, 1, 1, 1, 2, 255]])
    m = MeanIoU(num_classes=4, ignore_index=255).update(p, t)
    assert m.intersection.tolist() == [1.0, 2.0, 1.0, 0.0]
    assert m.pred_count.tolist() == [2.0, 2.0, 1.0, 0.0] and m.target_count.tolist() == [1.0, 3.0, 1.0, 0.0]
    iou = mean_iou(p, t, num_classes=4, ignore_index=255, average=None)
    assert iou[:3].tolist() == [0.5, pytest.approx(2 / 3, abs=TOL), 1.0] and iou[3].isnan()
    assert float(mean_iou(p, t, num_classes=4, ignore_index=255)) == pytest.approx((0.5 + 2 / 3 + 1) / 3, abs=TOL)
    assert float(mean_iou(p, t, num_classes=4, ignore_index=255, average="micro")) == pytest.approx(4 / 6, abs=TOL)
    dice = dice_score(p, t, num_classes=4, ignore_index=255, average="none")
    assert dice[:3].tolist() == [pytest.approx(2 / 3, abs=TOL), pytest.approx(0.8, abs=TOL), 1.0] and dice[3].isnan()
    assert float(dice_score(p, t, num_classes=4, ignore_index=255, average="micro")) == pytest.approx(0.8, abs=TOL)


@pytest.mark.parametrize("ignore", [None, 255, -100, 2])
def test_scores_against_the_oracle(ignore):
    for n, c, spatial, seed, used in ((1, 1, (3,), 1, None), (2, 2, (), 2, None), (3, 19, (7, 9), 3, None),
                                      (2, 33, (4, 5, 3), 4, 20), (1, 150, (17, 11), 5, 100)):
        x, t = case(n, c, spatial, seed, ignore=ignore, classes_used=used)
        want = O.counts(O.argmax_first(x.numpy()), t.numpy(), c, ignore)
        for fn, cls, dice in KINDS:
            m = cls(num_classes=c, ignore_index=ignore).update(x, t)
            check_counts(m, want)
            for average in AVERAGES:
                w = O.value(*want, dice, average)
                check_value(fn(x, t, num_classes=c, ignore_index=ignore, average=average), w)
                m.average = average
                check_value(m.compute(), w)
            check_value(fn(x, t, num_classes=c, ignore_index=ignore, average=None), O.value(*want, dice, "none"))


@pytest.mark.parametrize("ignore", [None, 255])
def test_values_against_scikit_learn(ignore):
    x, t = case(3, 19, (16, 12), 6, ignore=ignore, classes_used=15)
    pred = x.argmax(1)
    for fn, _, dice in KINDS:
        per_class, labels, micro = O.sklearn_values(pred.numpy(), t.numpy(), 19, ignore, dice)
        got = fn(x, t, num_classes=19, ignore_index=ignore, average="none")
        absent = np.setdiff1d(np.arange(19), labels)
        assert len(absent) > 0 and got[absent].isnan().all()
        check_value(got[labels], per_class)
        check_value(fn(x, t, num_classes=19, ignore_index=ignore), per_class.mean())
        check_value(fn(x, t, num_classes=19, ignore_index=ignore, average="micro"), micro)
        check_value(fn(pred, t, num_classes=19, ignore_index=ignore, average="micro"), micro)


def test_argmax_rule():
    nan, inf = math.nan, math.inf
    # one pixel per row of classes: ties, zeros of both signs, NaNs first / middle / last / several, infinities
    rows = [[1, 3, 3, 2], [-0.0, 0.0, -1, -2], [0.0, -0.0, 0.0, -0.0], [nan, 5, 1, 2], [1, nan, 9, 2], [1, 2, 9, nan],
            [1, nan, inf, nan], [inf, 1, inf, 2], [-inf, -inf, -inf, -inf], [-inf, 2, inf, inf], [-inf, -inf, 3, 3]]
    want = [1, 0, 0, 0, 1, 3, 1, 0, 0, 2, 2]
    x = torch.tensor(rows, dtype=torch.float32).t().reshape(1, 4, len(rows))
    assert O.argmax_first(x.numpy()).reshape(-1).tolist() == want
    for dtype in (torch.float32, torch.float16, torch.bfloat16, torch.float64):
        m = MeanIoU(num_classes=4).update(x.to(dtype), torch.tensor([want]))
        assert m.intersection.sum() == len(rows) and torch.equal(m.pred_count, m.target_count)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64])
def test_score_and_target_dtypes(dtype):
    x, t = case(2, 9, (6, 7), 7, dtype, ignore=255)
    want = O.counts(O.argmax_first(x.double().numpy()), t.numpy(), 9, 255)
    out = torch.float64 if dtype == torch.float64 else torch.float32
    for tt in (t, t.int(), t.to(torch.int16), t.to(torch.uint8)):
        check_counts(MeanIoU(num_classes=9, ignore_index=255).update(x, tt), want)
        check_value(mean_iou(x, tt, num_classes=9, ignore_index=255), O.value(*want, False, "macro"), out)
        check_value(dice_score(x, tt, num_classes=9, ignore_index=255, average=None), O.value(*want, True, "none"), out)
    # label-map predictions of every integer dtype
    pred = x.double().argmax(1)
    for pp in (pred, pred.int(), pred.to(torch.int16), pred.to(torch.uint8)):
        check_counts(DiceScore(num_classes=9, ignore_index=255).update(pp, t), want)


def test_ignore_index_outside_the_target_dtype_ignores_nothing():
    x, t = case(2, 5, (8,), 8)
    want = O.counts(O.argmax_first(x.numpy()), t.numpy(), 5)
    for ignore in (-1, 256, -100):
        check_counts(MeanIoU(num_classes=5, ignore_index=ignore).update(x, t.to(torch.uint8)), want)
    check_counts(MeanIoU(num_classes=5, ignore_index=2**40).update(x, t.int()), want)


def test_views_with_strides():
    x, t = case(2, 5, (6, 8), 9)
    want = mean_iou(x, t, num_classes=5)
    assert torch.equal(mean_iou(x.contiguous(memory_format=torch.channels_last), t, num_classes=5), want)
    big = torch.zeros(4, 8, 6, 10)
    big[::2, 2:7, :, 1:9] = x
    assert torch.equal(mean_iou(big[::2, 2:7, :, 1:9], t, num_classes=5), want)
    assert torch.equal(mean_iou(x, t.transpose(1, 2).contiguous().transpose(1, 2), num_classes=5), want)


def test_every_pixel_ignored_and_empty_inputs():
    x, t = case(2, 5, (4, 4), 10)
    for fn, cls, _ in KINDS:
        for average, shape in (("macro", ()), ("micro", ()), ("none", (5,))):
            out = fn(x, torch.full_like(t, 255), num_classes=5, ignore_index=255, average=average)
            assert out.dtype == torch.float32 and out.shape == shape and out.isnan().all()
            out = fn(torch.rand(0, 5, 4), torch.zeros(0, 4, dtype=torch.int64), num_classes=5, average=average)
            assert out.dtype == torch.float32 and out.shape == shape and out.isnan().all()
            out = fn(torch.rand(2, 5, 0), torch.zeros(2, 0, dtype=torch.int64), num_classes=5, average=average)
            assert out.shape == shape and out.isnan().all()
            assert cls(num_classes=5, average=average).compute().isnan().all()
            assert cls(num_classes=5, average=average).compute().shape == shape
        m = cls(num_classes=5).update(x, t)
        before = m.state_dict()
        m.update(torch.rand(0, 5, 4, 4), torch.zeros(0, 4, 4, dtype=torch.int64))
        m.update(torch.rand(2, 5, 0, 4), torch.zeros(2, 0, 4, dtype=torch.int64))
        for k, v in m.state_dict().items():
            assert torch.equal(v, before[k])


# ----------------------------------------------------------------------------- validation
def test_invalid_arguments():
    x, t = case(2, 5, (4, 6), 11)
    for fn, cls, _ in KINDS:
        for bad in (0, -3, 2.5, True):
            with pytest.raises(ValueError, match="`num_classes` should be a positive integer"):
                fn(x, t, num_classes=bad)
            with pytest.raises(ValueError, match="`num_classes` should be a positive integer"):
                cls(num_classes=bad)
        with pytest.raises(ValueError, match="`average` should be one of"):
            fn(x, t, num_classes=5, average="weighted")
        with pytest.raises(ValueError, match="`average` should be one of"):
            cls(num_classes=5, average="Macro")
        with pytest.raises(ValueError, match="`ignore_index` should be an integer"):
            fn(x, t, num_classes=5, ignore_index=2.0)
        with pytest.raises(ValueError, match="num_classes=6"):
            fn(x, t, num_classes=6)
        with pytest.raises(ValueError, match="num_classes=4"):
            cls(num_classes=4).update(x, t)
        with pytest.raises(ValueError, match="agree in num_sample"):
            fn(x, t[:1], num_classes=5)
        with pytest.raises(ValueError, match="agree in num_sample"):
            fn(x, t[:, :3], num_classes=5)
        with pytest.raises(ValueError, match="agree in num_sample"):
            cls(num_classes=5).update(x, t.transpose(1, 2))
        with pytest.raises(ValueError, match=r"\(num_sample, num_classes, \*spatial\)"):
            fn(x, t[:, 0], num_classes=5)
        with pytest.raises(ValueError, match="shape of `target`"):
            fn(t, t[:, :3], num_classes=5)
        for tt in (t.float(), t.bool(), t.double()):
            with pytest.raises(ValueError, match="integer labels"):
                fn(x, tt, num_classes=5)
        with pytest.raises(ValueError, match="scores or integer labels"):
            fn(t.bool(), t, num_classes=5)


def test_bad_labels_raise_and_leave_the_states():
    x, t = case(2, 5, (4, 6), 12)
    high, low, ignored = t.clone(), t.clone(), t.clone()
    high[1, 2, 3] = 5
    low[0, 0, 0] = -1
    ignored[1, 2, 3] = 255
    pred = x.argmax(1)
    bad_pred = pred.clone()
    bad_pred[0, 1, 1] = 7
    cases = [(x, high, None, "`target` holds"), (x, low, None, "`target` holds"), (x, ignored, -100, "`target` holds"),
             (bad_pred, t, None, "label-map `input` holds"), (bad_pred, high, None, "`target` holds.*; .*`input` holds")]
    for xi, ti, ignore, msg in cases:
        with pytest.raises(ValueError, match=msg):
            mean_iou(xi, ti, num_classes=5, ignore_index=ignore)
        m = DiceScore(num_classes=5, ignore_index=ignore).update(x, t)
        before = m.state_dict()
        with pytest.raises(ValueError, match=msg):
            m.update(xi, ti)
        for k, v in m.state_dict().items():
            assert torch.equal(v, before[k])
        assert not m.compute().isnan()
    # an ignored pixel is not examined: neither its target nor its prediction
    bad_pred[0, 1, 1] = pred[0, 1, 1]
    bad_pred[1, 2, 3] = 9
    want = O.counts(pred.numpy(), ignored.numpy(), 5, 255)
    check_counts(MeanIoU(num_classes=5, ignore_index=255).update(bad_pred, ignored), want)


# ----------------------------------------------------------------------------- class protocol
class TestMeanIoU(MetricClassTester):
    def _run(self, cls, dice: bool, average: str, ignore) -> None:
        x, t = case(8 * 2, 7, (5, 6), 13, ignore=ignore, classes_used=6)
        want = O.value(*O.counts(O.argmax_first(x.numpy()), t.numpy(), 7, ignore), dice, average)
        self.run_class_implementation_tests(
            metric=cls(num_classes=7, ignore_index=ignore, average=average),
            state_names=set(STATES),
            update_kwargs={"input": x.reshape(8, 2, 7, 5, 6), "target": t.reshape(8, 2, 5, 6)},
            compute_result=torch.tensor(want).float(),
            atol=TOL,
            rtol=0,
        )

    def test_class_suite_mean_iou_macro(self) -> None:
        self._run(MeanIoU, False, "macro", 255)

    def test_class_suite_dice_micro(self) -> None:
        self._run(DiceScore, True, "micro", None)

    def test_class_suite_mean_iou_per_class(self) -> None:
        self._run(MeanIoU, False, "none", 255)


def test_merge_of_halves_equals_one_pass_bit_for_bit():
    x, t = case(6, 19, (9, 7), 14, ignore=255)
    want = O.counts(O.argmax_first(x.numpy()), t.numpy(), 19, 255)
    for fn, cls, dice in KINDS:
        whole = cls(num_classes=19, ignore_index=255).update(x, t)
        a = cls(num_classes=19, ignore_index=255).update(x[:3], t[:3])
        b = cls(num_classes=19, ignore_index=255).update(x[3:], t[3:])
        a.merge_state([b])
        check_counts(a, want)
        for name in STATES:
            assert torch.equal(getattr(a, name), getattr(whole, name))
        assert torch.equal(a.compute(), whole.compute())
        assert torch.equal(a.compute(), fn(x, t, num_classes=19, ignore_index=255))
        check_value(a.compute(), O.value(*want, dice, "macro"))


def test_updates_accumulate_reset_and_state_dict():
    x, t = case(5, 6, (8,), 15)
    want = O.counts(O.argmax_first(x.numpy()), t.numpy(), 6)
    m = MeanIoU(num_classes=6)
    for lo, hi in ((0, 1), (1, 4), (4, 5)):
        m.update(x[lo:hi], t[lo:hi])
    check_counts(m, want)
    check_value(m.compute(), O.value(*want, False, "macro"))
    c = MeanIoU(num_classes=6)
    c.load_state_dict(m.state_dict())
    assert torch.equal(c.compute(), m.compute())
    m.reset()
    assert all(getattr(m, name).sum() == 0 for name in STATES) and m.compute().isnan()
    check_value(m.update(x, t).compute(), O.value(*want, False, "macro"))
    assert m._state_merge_kinds() == {name: "sum" for name in STATES}


def _sync_job(rank: int, ws: int):
    from torcheval_amd.metrics.toolkit import sync_and_compute

    x, t = case(6, 5, (7, 3), 16, ignore=255)
    lo, hi = (0, 2) if rank == 0 else (2, 6)
    return sync_and_compute(DiceScore(num_classes=5, ignore_index=255).update(x[lo:hi], t[lo:hi]))


def test_two_rank_sync_and_compute():
    x, t = case(6, 5, (7, 3), 16, ignore=255)
    results = run_distributed(_sync_job, 2)
    assert results[0] is not None  # rank 0 is the recipient
    want = O.value(*O.counts(O.argmax_first(x.numpy()), t.numpy(), 5, 255), True, "macro")
    for got in results:
        if got is not None:
            check_value(got, want)


# ----------------------------------------------------------------------------- exports, routing
def test_exports():
    for mod in (M, MC):
        assert mod.MeanIoU is MeanIoU and mod.DiceScore is DiceScore
    for mod in (MF, MFC):
        assert mod.mean_iou is mean_iou and mod.dice_score is dice_score
    # the top-level lists mirror the reference's public names and are built from the family lists
    for mod in (M, MC):
        assert "MeanIoU" not in mod.__all__ and "DiceScore" not in mod.__all__
    for mod in (MF, MFC):
        assert "mean_iou" not in mod.__all__ and "dice_score" not in mod.__all__


def test_wrapper_constants_match_the_header():
    from torcheval_amd.ops import segmentation as K

    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    with open(os.path.join(root, "csrc", "include", "tea_kernels.h")) as fh:
        header = fh.read()

    def const(name):
        return int(re.search(rf"constexpr int {name} = (\d+);", header).group(1))

    assert K.SPAN == const("kSegSpan")
    assert K.max_blocks() == K.MAX_BLOCKS == const("kSegMaxBlocks")
    assert K.max_classes() == K.MAX_CLASSES == const("kSegMaxClasses")
    # three u32 histograms of the 8 blocks of 256 threads a CU can hold fit its 160 KiB of LDS
    assert 8 * 3 * 4 * K.max_classes() <= 160 * 1024


def test_arm_of_a_layout():
    from torcheval_amd.ops import segmentation as K

    x = torch.zeros(2, 24, 6, 8)
    assert K.arm(x) == K.arm(x[:, :19]) == K.arm(x[::2]) == K.arm(x[:, :, 0]) == "plane"
    assert K.arm(x.to(memory_format=torch.channels_last)) == "element"
    assert K.arm(x[..., 1:-1]) == "" and K.arm(x[:, :, 1:-1]) == "plane"
    assert K.arm(x.half()) == "plane" and K.arm(torch.zeros(2, 5, 3, 3).half()) == "element"
    assert K.arm(torch.zeros(2, 1, 3, 3).half()) == "plane"
    assert K.arm(torch.zeros(2, 5, 1, 1).bfloat16()) == "element" and K.arm(torch.zeros(2, 5, 1, 1)) == "plane"
    assert K.arm(torch.zeros(2, 5)) == "plane" and K.arm(torch.zeros(2, 5, dtype=torch.int32)) == "label"


@pytest.mark.skipif(not ops.native_loaded(), reason="extension not built")
def test_native_op_surface_and_compiled_route(monkeypatch):
    """K17's three ops: their schemas, which dispatch keys hold a kernel, Meta kernels that return
    None, and the wrapper on meta tensors with ``compiling`` forced."""
    from torcheval_amd.ops import segmentation as K

    ns = "torcheval_amd_segmentation::"
    names = sorted(n for n in torch._C._dispatch_get_all_op_names() if n.startswith(ns))
    assert names == [ns + "segmentation_batch", ns + "segmentation_update", ns + "segmentation_value"]
    lib = torch.ops.torcheval_amd_segmentation
    assert str(lib.segmentation_update.default._schema) == (
        ns + "segmentation_update(Tensor input, Tensor target, int num_classes, int arm, int? ignore_index, "
        "Tensor(a!) intersection, Tensor(b!) pred_count, Tensor(c!) target_count, Tensor(d!)? err) -> ()")
    assert str(lib.segmentation_batch.default._schema) == (
        ns + "segmentation_batch(Tensor input, Tensor target, int num_classes, int arm, int? ignore_index, "
        "bool dice, int average, Tensor(a!) out, Tensor(b!)? err) -> ()")
    assert str(lib.segmentation_value.default._schema) == (
        ns + "segmentation_value(Tensor intersection, Tensor pred_count, Tensor target_count, bool dice, "
        "int average, Tensor(a!) out) -> ()")
    for name in names:
        has = [k for k in ("CPU", "CUDA", "Meta") if torch._C._dispatch_has_kernel_for_dispatch_key(name, k)]
        assert has == ["CUDA", "Meta"]
    monkeypatch.setattr(ops, "compiling", lambda: True)
    meta = torch.device("meta")
    x, t = torch.empty(2, 9, 4, 6, device=meta), torch.empty(2, 4, 6, dtype=torch.int64, device=meta)
    s = [torch.empty(9, dtype=torch.float64, device=meta) for _ in range(3)]
    err = torch.empty(1, dtype=torch.int32, device=meta)
    assert K.segmentation_update(x, t, 9, 255, *s, err) is None
    assert K.segmentation_update(t, t, 9, None, *s, None) is None
    for average, shape in (("macro", ()), ("micro", ()), ("none", (9,))):
        for out in (K.segmentation_batch(x, t, 9, None, True, average, None), K.segmentation_value(*s, False, average)):
            assert out.shape == shape and out.dtype == torch.float32 and out.device.type == "meta"
