"""K17 (csrc/kernels/segmentation.hip) on the GPU: segmentation mean IoU and Dice in one pass.

Oracle: tests/_segmentation_oracle.py, numpy int64 counts and FP64 values of the definition in
docs/parity.md.  The three counts must equal the oracle's exactly; the values, at most 1 and formed
in FP64 from equal counts on both sides, lie within ``2^-23`` of the oracle rounded to float32.

Shapes are the smallest at which each piece can go wrong: one image and three; class counts below,
at and above the kAhead = 8 classes whose loads the walk keeps in flight (1, 2, 19, 33, 150) and the
cap; pixel counts below one group (1, 3), across groups of 4 and 8 (5, 7, 9) and around a span
(``SPAN`` - 1, ``SPAN``, ``SPAN`` + 1); plane bases off 16 bytes by 1-3 elements; every layout an
arm takes and one that none does; a few more spans than the grid has blocks.
"""

import functools
import math

import numpy as np
import pytest
import torch

from tests import _segmentation_oracle as O
from torcheval_amd.config import flags
from torcheval_amd.metrics import DiceScore, MeanIoU
from torcheval_amd.metrics.functional import dice_score, mean_iou
from torcheval_amd.ops import segmentation as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TOL = 2.0**-23
STATES = ("intersection", "pred_count", "target_count")
COMBOS = tuple((dice, average) for dice in (False, True) for average in ("macro", "micro", "none"))
SCORE_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
TARGET_DTYPES = (torch.int64, torch.int32, torch.int16, torch.uint8)


@pytest.fixture
def native_calls(monkeypatch):
    """Counts the calls through the K17 wrapper: the native path really ran."""
    calls = []
    for name in ("segmentation_update", "segmentation_batch"):
        real = getattr(K, name)

        def spy(*a, _real=real, **k):
            calls.append(1)
            return _real(*a, **k)

        monkeypatch.setattr(K, name, spy)
    return calls


@functools.lru_cache(maxsize=None)
def scores(n: int, c: int, spatial: tuple, seed: int, dtype: torch.dtype):
    """Seeded CPU scores, their oracle predictions and int64 labels (about half of them the
    prediction); shared between tests, never modified."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, c, *spatial, generator=g) * 3).to(dtype)
    pred = torch.from_numpy(O.argmax_first(x.double().numpy()))
    t = torch.where(torch.rand(pred.shape, generator=g) < 0.5, pred, torch.randint(0, c, pred.shape, generator=g))
    return x, pred, t


def with_ignored(t: torch.Tensor, ignore) -> torch.Tensor:
    """A copy of ``t`` with every tenth label (from the fourth) set to ``ignore``."""
    if ignore is None:
        return t
    flat = t.clone().reshape(-1)
    flat[3::10] = ignore
    return flat.reshape(t.shape)


def check_value(got: torch.Tensor, want):
    want = np.asarray(want, dtype=np.float64)
    assert got.dtype == torch.float32 and got.device == DEV and tuple(got.shape) == want.shape, (got.dtype, got.shape)
    g, w = got.double().cpu().numpy(), want.astype(np.float32).astype(np.float64)
    assert np.array_equal(np.isnan(g), np.isnan(w)), (g, w)
    assert (np.abs(g - w)[~np.isnan(w)] <= TOL).all(), (g, w)


def check_states(m, want):
    for name, w in zip(STATES, want):
        got = getattr(m, name).cpu().numpy()
        assert np.array_equal(got, w.astype(np.float64)), (name, got, w)


def check(xd, td, pred, t, c, ignore, combos=COMBOS):
    """One class update (the counts, exactly) and functional values of device tensors against the
    oracle on the CPU prediction and labels."""
    want = O.counts(pred.numpy(), t.numpy(), c, ignore)
    m = MeanIoU(num_classes=c, ignore_index=ignore, device=DEV).update(xd, td)
    check_states(m, want)
    check_value(m.compute(), O.value(*want, False, "macro"))
    for dice, average in combos:
        fn = dice_score if dice else mean_iou
        check_value(fn(xd, td, num_classes=c, ignore_index=ignore, average=average), O.value(*want, dice, average))
    return want


# ----------------------------------------------------------------------------- shapes
PIXELS = (1, 3, 5, 7, 9, K.SPAN - 1, K.SPAN, K.SPAN + 1)


@pytest.mark.parametrize("dtype", SCORE_DTYPES)
def test_shapes_score_dtypes_and_target_dtypes(dtype, native_calls):
    i = 0
    for n in (1, 3):
        for c in (1, 2, 19, 33, 150):
            for spatial in [()] + [(p,) for p in PIXELS]:
                x, pred, t = scores(n, c, spatial, 1000 * c + (spatial[0] if spatial else 0), dtype)
                ignore = (None, 255, -100, c // 2)[i % 4]
                tdt = TARGET_DTYPES[i % 4 if ignore != -100 else i % 3]  # -100 is no uint8 value
                ti = with_ignored(t, ignore)
                before = len(native_calls)
                check(x.to(DEV), ti.to(tdt).to(DEV), pred, ti, c, ignore, combos=(COMBOS[i % 6],))
                assert len(native_calls) == before + 2  # one update, one functional call
                i += 1


def test_every_value_of_one_batch(native_calls):
    x, pred, t = scores(3, 19, (37, 53), 1, torch.float32)
    ti = with_ignored(t, 255)
    check(x.to(DEV), ti.to(DEV), pred, ti, 19, 255)
    assert len(native_calls) == 7
    m = DiceScore(num_classes=19, ignore_index=255, device=DEV).update(x.to(DEV), ti.to(DEV))
    want = O.counts(pred.numpy(), ti.numpy(), 19, 255)
    for average in ("macro", "micro", "none"):
        m.average = average
        check_value(m.compute(), O.value(*want, True, average))


def test_classes_at_the_cap_and_one_above(native_calls):
    cap = K.max_classes()
    for n, spatial, dtype in ((1, (7,), torch.bfloat16), (3, (K.SPAN + 1,), torch.float32), (2, (3, 8), torch.float16)):
        x, pred, t = scores(n, cap, spatial, 2, dtype)
        before = len(native_calls)
        check(x.to(DEV), t.to(torch.int16).to(DEV), pred, t, cap, None, combos=(COMBOS[0], COMBOS[5]))
        assert len(native_calls) == before + 3
    x, pred, t = scores(3, cap + 1, (5,), 3, torch.float32)
    before = len(native_calls)
    check(x.to(DEV), t.to(DEV), pred, t, cap + 1, None, combos=(COMBOS[0],))  # the ATen form: no native call
    assert len(native_calls) == before


def test_three_spatial_dims(native_calls):
    for dtype in SCORE_DTYPES:
        x, pred, t = scores(2, 19, (3, 5, 8), 4, dtype)
        ti = with_ignored(t, 255)
        check(x.to(DEV), ti.to(DEV), pred, ti, 19, 255, combos=(COMBOS[0], COMBOS[4]))
    assert len(native_calls) == 9


# ----------------------------------------------------------------------------- layouts
def _offset_copy(x: torch.Tensor, k: int) -> torch.Tensor:
    """``x`` on the device, starting ``k`` elements into a fresh allocation."""
    buf = torch.zeros(x.numel() + k, dtype=x.dtype, device=DEV)
    view = buf[k:].view(x.shape)
    view.copy_(x)
    return view


@pytest.mark.parametrize("dtype", SCORE_DTYPES)
def test_plane_bases_off_sixteen_bytes(dtype, native_calls):
    """A storage offset of 1-3 elements under planes of whole 16-byte units (the 16-bit plane arm's
    head and tail, within a span and across two) and planes of an odd size (every class plane at
    another alignment: the plane arm for float32, the element arm for 16-bit scores)."""
    wide = dtype == torch.float32
    for k, spatial, arm in ((1, (4, 8), "plane"), (2, (K.SPAN + 24,), "plane"), (3, (5, 16), "plane"),
                            (1, (5, 7), "plane" if wide else "element"), (3, (K.SPAN + 3,), "plane" if wide else "element")):
        x, pred, t = scores(3, 19, spatial, 5, dtype)
        view = _offset_copy(x, k)
        assert view.data_ptr() % 16 == k * x.element_size() and K.arm(view) == arm
        before = len(native_calls)
        check(view, t.to(DEV), pred, t, 19, None, combos=(COMBOS[0],))
        assert len(native_calls) == before + 2


@pytest.mark.parametrize("dtype", SCORE_DTYPES)
def test_views_every_arm_takes_and_one_none_does(dtype, native_calls):
    x, pred, t = scores(3, 19, (6, 16), 6, dtype)
    td = t.to(DEV)
    parent = torch.zeros(3, 24, 6, 16, dtype=dtype, device=DEV)
    parent[:, :19] = x.to(DEV)
    tall = torch.zeros(6, 19, 6, 16, dtype=dtype, device=DEV)
    tall[::2] = x.to(DEV)
    last = x.to(DEV).contiguous(memory_format=torch.channels_last)
    assert last.stride(1) == 1 and last.stride(3) == 19
    for view, arm in ((parent[:, :19], "plane"), (tall[::2], "plane"), (last, "element")):
        assert K.arm(view) == arm and not view.is_contiguous()
        before = len(native_calls)
        check(view, td, pred, t, 19, None, combos=(COMBOS[1], COMBOS[3]))
        assert len(native_calls) == before + 3
    # a cropped view does not flatten to one pixel stride: the ATen form
    xp, predp, tp = scores(3, 19, (6, 18), 7, dtype)
    crop = xp.to(DEV)[..., 1:-1]
    assert K.arm(crop) == ""
    before = len(native_calls)
    check(crop, tp[..., 1:-1].to(DEV), predp[..., 1:-1], tp[..., 1:-1], 19, None, combos=(COMBOS[0],))
    assert len(native_calls) == before
    # a target that is not contiguous is copied on the host side of the op
    tt = t.transpose(1, 2).contiguous().to(DEV).transpose(1, 2)
    assert not tt.is_contiguous()
    check(x.to(DEV), tt, pred, t, 19, None, combos=(COMBOS[0],))
    assert len(native_calls) == before + 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_more_spans_than_blocks(dtype, native_calls):
    """Images of one pixel are one span each: the persistent grid loops."""
    n = K.max_blocks() + 7
    x, pred, t = scores(n, 5, (), 8, dtype)
    check(x.to(DEV), t.to(DEV), pred, t, 5, None, combos=(COMBOS[0],))
    x, pred, t = scores(n, 5, (1, 1), 9, dtype)
    ti = with_ignored(t, 2)
    check(x.to(DEV), ti.to(DEV), pred, ti, 5, 2, combos=(COMBOS[2],))
    assert len(native_calls) == 4


# ----------------------------------------------------------------------------- argmax rule
def _rule_scores(c: int) -> torch.Tensor:
    """[1, c, 40] float32: per pixel four values at classes 0 < a < b < c - 1, -inf elsewhere
    (classes past the eight in flight for c = 19): exact ties, zeros of both signs, NaN first /
    middle / last / several, infinities, a pixel of all -inf."""
    nan, inf = math.nan, math.inf
    rows = [[1, 3, 3, 2], [-0.0, 0.0, -1, -2], [0.0, -0.0, 0.0, -0.0], [nan, 5, 1, 2], [1, nan, 9, 2], [1, 2, 9, nan],
            [1, nan, inf, nan], [inf, 1, inf, 2], [-inf, -inf, -inf, -inf], [-inf, 2, inf, inf], [-inf, -inf, 3, 3],
            [2, 2, 2, 2], [-inf, nan, nan, 1]]
    rows = (rows * 4)[:40]
    at = [0, 1, 2, 3] if c == 4 else [0, c // 3, c // 2 + 1, c - 1]
    x = torch.full((1, c, 40), -inf)
    x[0, at] = torch.tensor(rows, dtype=torch.float32).t()
    return x


@pytest.mark.parametrize("dtype", SCORE_DTYPES)
@pytest.mark.parametrize("c", [4, 19])
def test_argmax_rule(c, dtype, native_calls):
    x = _rule_scores(c).to(dtype)
    pred = torch.from_numpy(O.argmax_first(x.double().numpy()))
    at = [0, 1, 2, 3] if c == 4 else [0, c // 3, c // 2 + 1, c - 1]
    assert pred[0, :13].tolist() == [at[i] for i in (1, 0, 0, 0, 1, 3, 1, 0, 0, 2, 2, 0, 1)]
    t = pred.clone()
    t[0, ::3] = c - 2
    views = {"plane": x.to(DEV), "element": x.to(DEV).transpose(1, 2).contiguous().transpose(1, 2),
             "off 16 bytes": _offset_copy(x, 1), "cut groups": _offset_copy(x[..., :37].contiguous(), 1)}
    assert K.arm(views["plane"]) == "plane" and K.arm(views["element"]) == "element"
    for name, view in views.items():
        p = view.shape[2]
        check(view, t[:, :p].to(DEV), pred[:, :p], t[:, :p], c, None, combos=(COMBOS[2],))
    assert len(native_calls) == 8


# ----------------------------------------------------------------------------- ignore, bad labels
def test_every_pixel_ignored_is_nan(native_calls):
    x, pred, t = scores(3, 19, (9,), 10, torch.float32)
    td = torch.full_like(t, 255).to(torch.uint8).to(DEV)
    for dice, average in COMBOS:
        out = (dice_score if dice else mean_iou)(x.to(DEV), td, num_classes=19, ignore_index=255, average=average)
        assert out.dtype == torch.float32 and out.shape == ((19,) if average == "none" else ()) and out.isnan().all()
    m = MeanIoU(num_classes=19, ignore_index=255, device=DEV).update(x.to(DEV), td)
    assert m.compute().isnan() and all(float(getattr(m, s).sum()) == 0.0 for s in STATES)
    assert MeanIoU(num_classes=19, device=DEV).compute().isnan()
    assert len(native_calls) == 7


@pytest.mark.parametrize("label_map", [False, True])
def test_labels_out_of_range(label_map, native_calls):
    c = 19
    x, pred, t = scores(3, c, (K.SPAN + 8,), 11, torch.float16)
    cases = []
    for value in (c, -1, 255):
        bt = with_ignored(t, -100)
        bt[1, 18] = value
        cases.append((pred if label_map else x, pred, bt, 1, "`target` holds"))
    if label_map:
        bp = pred.clone()
        bp[2, K.SPAN + 1] = c
        bp[0, 3] = -7  # on an ignored pixel: not examined
        cases.append((bp, bp, with_ignored(t, -100), 2, "label-map `input` holds"))
    for inp, p, bt, bits, msg in cases:
        assert bt.reshape(-1)[3] == -100
        xd, td = inp.to(DEV), bt.to(DEV)
        want = O.counts(p.numpy(), bt.numpy(), c, -100, drop_bad=True)
        assert want[2].sum() == O.counts(pred.numpy(), with_ignored(t, -100).numpy(), c, -100)[2].sum() - 1
        check_value(mean_iou(xd, td, num_classes=c, ignore_index=-100), O.value(*want, False, "macro"))  # no raise
        m = MeanIoU(num_classes=c, ignore_index=-100, device=DEV)
        m.update(xd[:1], with_ignored(t, -100)[:1].to(DEV))
        m.update(xd, td)  # no raise at the update
        assert int(m._err.item()) == bits
        first = O.counts(p[:1].numpy(), with_ignored(t, -100)[:1].numpy(), c, -100, drop_bad=True)
        check_states(m, [a + b for a, b in zip(first, want)])
        with pytest.raises(ValueError, match=msg):
            m.compute()
        assert int(m._err.item()) == 0
        assert not m.compute().isnan()  # and no second raise
        with flags(validate=True):
            with pytest.raises(ValueError, match=msg):
                dice_score(xd, td, num_classes=c, ignore_index=-100)
            assert not dice_score(xd[:1], with_ignored(t, -100)[:1].to(DEV), num_classes=c, ignore_index=-100).isnan()
    assert len(native_calls) == 5 * len(cases)


def test_label_maps_of_every_integer_dtype(native_calls):
    x, pred, t = scores(3, 150, (K.SPAN + 1,), 12, torch.float32)
    ti = with_ignored(t, 255)
    for i, (pdt, tdt) in enumerate(zip(TARGET_DTYPES, reversed(TARGET_DTYPES))):
        pd = pred.to(pdt).to(DEV)
        assert K.arm(pd) == "label"
        check(pd, ti.to(tdt).to(DEV), pred, ti, 150, 255, combos=(COMBOS[i], COMBOS[5 - i]))
    pd = pred.to(DEV).transpose(0, 1).contiguous().transpose(0, 1)  # copied on the host side of the op
    check(pd, ti.to(DEV), pred, ti, 150, 255, combos=(COMBOS[0],))
    assert len(native_calls) == 14


@pytest.mark.parametrize("n,p", [(3, K.SPAN + 1), (101, 5)])
@pytest.mark.parametrize("c", [1, 341, 342, 1024])
def test_finish_chunks_and_runs_of_label_maps(c, n, p, native_calls):
    """The finish launch's fold over runs of blocks (tea_partials.h run_fold) on label maps, the
    counts exact against ``bincount``.  The 3 c pairs are taken 1024 at a time: one class is 3 pairs
    and 341 runs, 341 classes one chunk of one run, 342 a second chunk of 2 pairs with 512 runs, 1024
    three full chunks; each over 6 blocks (most runs empty) and over 101.  A second update
    accumulates into the same states."""
    assert c <= K.max_classes() and n * -(-p // K.SPAN) == (6 if n == 3 else 101)  # one block per span
    g = torch.Generator().manual_seed(7000 + c + n)
    pred = torch.randint(0, c, (n, p), generator=g)
    t = torch.where(torch.rand(n, p, generator=g) < 0.5, pred, torch.randint(0, c, (n, p), generator=g))
    want = [torch.bincount(v.reshape(-1), minlength=c).double() for v in (pred[pred == t], pred, t)]
    pd, td = pred.to(DEV), t.to(DEV)
    assert K.arm(pd) == "label"
    m = MeanIoU(num_classes=c, device=DEV).update(pd, td)
    for name, w in zip(STATES, want):
        assert torch.equal(getattr(m, name).cpu(), w), name
    m.update(pd, td)
    for name, w in zip(STATES, want):
        assert torch.equal(getattr(m, name).cpu(), 2 * w), name
    assert len(native_calls) == 2


# ----------------------------------------------------------------------------- label structure
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_one_label_images_and_sixty_four_labels_in_a_wave(dtype, native_calls):
    c, p = 67, K.SPAN + 16  # 67 is prime: any 64 pixels at one stride hold 64 labels
    # every image one label, predicted right: one fold round per wave
    x = torch.zeros(3, c, p)
    t = torch.tensor([5, 66, 0])[:, None].expand(3, p).contiguous()
    x.scatter_(1, t[:, None], 4.0)
    check(x.to(dtype).to(DEV), t.to(DEV), t, t, c, None, combos=(COMBOS[0],))
    # labels that change at every pixel: 64 distinct (target, prediction) values in a wave's step
    t = (torch.arange(3 * p).reshape(3, p) * 3) % c
    pred = (torch.arange(3 * p).reshape(3, p) * 11 + 3) % c
    x = torch.zeros(3, c, p).scatter_(1, pred[:, None], 4.0)
    check(x.to(dtype).to(DEV), t.to(DEV), pred, t, c, None, combos=(COMBOS[1],))
    # and two values per wave: the second fold round
    t = (torch.arange(3 * p).reshape(3, p) // 37) % 2 * 60
    check(x.to(dtype).to(DEV), t.to(DEV), pred, t, c, None, combos=(COMBOS[2],))
    check(pred.to(DEV), t.to(DEV), pred, t, c, None, combos=(COMBOS[3],))
    assert len(native_calls) == 8


# ----------------------------------------------------------------------------- class, repeatability
def test_two_runs_are_bit_identical(native_calls):
    x, pred, t = scores(3, 33, (K.SPAN + 1,), 2033, torch.float32)
    xd, td = x.to(DEV), with_ignored(t, 255).to(DEV)
    a = MeanIoU(num_classes=33, ignore_index=255, device=DEV).update(xd, td)
    b = MeanIoU(num_classes=33, ignore_index=255, device=DEV).update(xd, td)
    for name in STATES:
        assert torch.equal(getattr(a, name), getattr(b, name))
    for dice, average in COMBOS:
        fn = dice_score if dice else mean_iou
        v1 = fn(xd, td, num_classes=33, ignore_index=255, average=average)
        v2 = fn(xd, td, num_classes=33, ignore_index=255, average=average)
        assert torch.equal(v1, v2) or (average == "none" and torch.equal(v1.isnan(), v2.isnan())
                                       and torch.equal(v1.nan_to_num(), v2.nan_to_num()))
    assert len(native_calls) == 14


def test_class_updates_accumulate_and_merge_matches_one_pass(native_calls):
    """What an update dispatches: views of its operands, the K17 op (its two launches) and nothing
    else.  States after three updates, and after a merge of halves, equal those of one update, bit
    for bit."""
    from torch.utils._python_dispatch import TorchDispatchMode

    seen = []

    class Recorder(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    x, pred, t = scores(5, 19, (40, 56), 13, torch.bfloat16)
    ti = with_ignored(t, 255)
    xd, td = x.to(DEV), ti.to(DEV)
    want = O.counts(pred.numpy(), ti.numpy(), 19, 255)
    for cls, dice in ((MeanIoU, False), (DiceScore, True)):
        del seen[:]
        m = cls(num_classes=19, ignore_index=255, device=DEV)
        parts = [(xd[lo:hi], td[lo:hi]) for lo, hi in ((0, 1), (1, 4), (4, 5))]
        with Recorder():
            for px, pt in parts:
                m.update(px, pt)
        views = {"aten.as_strided.default", "aten.reshape.default", "aten.view.default"}  # the [N, C, P] forms
        assert [s for s in seen if s not in views] == ["torcheval_amd_segmentation.segmentation_update.default"] * 3, seen
        whole = cls(num_classes=19, ignore_index=255, device=DEV).update(xd, td)
        a = cls(num_classes=19, ignore_index=255, device=DEV).update(xd[:2], td[:2])
        b = cls(num_classes=19, ignore_index=255, device=DEV).update(xd[2:], td[2:])
        a.merge_state([b])
        for other in (m, a):
            check_states(other, want)
            for name in STATES:
                assert torch.equal(getattr(other, name), getattr(whole, name))
            assert torch.equal(other.compute(), whole.compute())
        check_value(m.compute(), O.value(*want, dice, "macro"))
        moved = m.to("cpu")
        assert moved.intersection.device.type == "cpu"
        assert abs(float(moved.compute()) - float(whole.compute())) <= TOL
        whole.reset()
        assert float(whole.pred_count.sum()) == 0.0 and whole.compute().isnan()
    assert len(native_calls) == 12
