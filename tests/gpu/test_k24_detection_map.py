"""K24 (csrc/kernels/detection_map.hip) on MI355X: detection mean average precision against the numpy
oracle of tests/_detection_oracle.py under the exactness of tests/metrics/detection/test_mean_ap.py:
the integers of the matching equal, the float64 tables within 2^-40, the float32 results within
2^-23.  The image sizes sit at the edges of the kernel's paths: the 64-lane chunks of ground truths,
the powers of two the LDS sort pads to, ``max_detections``, the cap of ``ops.detection.max_boxes()``
(one box more must agree through the ATen form) and more images than the grid has workgroups; the
curve's segments sit around its 256-position chunks."""

import numpy as np
import pytest
import torch

from tests import _detection_oracle as oracle
from tests.metrics.detection.test_mean_ap import (
    KEYS,
    case,
    check_match,
    check_tables,
    check_values,
    run_case,
    table,
    want_match,
)
from torcheval_amd.config import flags
from torcheval_amd.metrics import MeanAveragePrecision
from torcheval_amd.metrics.functional import mean_average_precision
from torcheval_amd.metrics.functional.detection.mean_ap import _map_match, _map_tables
from torcheval_amd.ops import detection as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CAP = K.MAX_BOXES


@pytest.fixture
def native_calls(monkeypatch):
    """Counts the launches through the K24 wrapper: the native path really ran."""
    calls = {"match": 0, "curve": 0}
    real_match, real_curve = K.map_match, K.map_curve

    def match(*a, **k):
        calls["match"] += 1
        return real_match(*a, **k)

    def curve(*a, **k):
        calls["curve"] += 1
        return real_curve(*a, **k)

    monkeypatch.setattr(K, "map_match", match)
    monkeypatch.setattr(K, "map_curve", curve)
    return calls


def gpu_case(key, num_classes, native_calls, **kwargs):
    """``run_case`` on the device, the native path seen by the spy, and the ATen form on the CPU
    copies giving the same integers."""
    before = dict(native_calls)
    got, out = run_case(key, num_classes, device=DEV, **kwargs)
    assert native_calls["match"] == before["match"] + 2 and native_calls["curve"] == before["curve"] + 2
    assert all(t.is_cuda for t in got) and all(v.is_cuda for v in out.values())
    pb, ps, pl, pc, tb, tl, tc = case(*key)
    thr = torch.tensor(table(kwargs.get("thresholds")), dtype=torch.float64)
    cpu = _map_match(pb, ps, pl, list(pc), tb, tl, list(tc), num_classes, thr, kwargs.get("max_detections", 100),
                     None, True)
    for g, c in zip(got, cpu):
        assert torch.equal(g.cpu().view(torch.int32) if g.dtype == torch.float32 else g.cpu(),
                           c.view(torch.int32) if c.dtype == torch.float32 else c)
    return got, out


# ----------------------------------------------------------------------------- matching shapes
@pytest.mark.parametrize("num_classes", [1, 3])
def test_detections_and_ground_truths_per_image_at_the_chunk_edges(num_classes, native_calls):
    gpu_case((20, (0, 1, 2, 63, 64, 65, 101, 257), (3, 0, 1, 63, 64, 65, 130, 5), num_classes), num_classes,
             native_calls)
    gpu_case((21, (65, 130, 1), (0, 1, 64), num_classes), num_classes, native_calls, max_detections=64)


def test_images_at_the_cap(native_calls):
    # every detection kept: max_detections above the cap
    gpu_case((22, (CAP - 1, CAP), (65, 64), 1), 1, native_calls, max_detections=5000)
    gpu_case((23, (101, 3), (CAP, CAP - 1), 1), 1, native_calls, thresholds=(0.5,))
    gpu_case((24, (CAP, CAP - 1), (130, 1), 3), 3, native_calls, thresholds=(0.5, 0.75))


@pytest.mark.parametrize("num_classes", [1, 3, 80, 2**22 - 1])
def test_class_counts_up_to_the_key_width(num_classes, native_calls):
    thresholds = (0.5,) if num_classes > 80 else None
    gpu_case((25, (20, 0, 33, 7, 64), (10, 5, 0, 7, 40), num_classes), num_classes, native_calls,
             thresholds=thresholds)


@pytest.mark.parametrize("images", [1, K.GRID + 37])
def test_one_image_and_more_images_than_workgroups(images, native_calls):
    pred = tuple((3 * i + 1) % 5 for i in range(images))
    target = tuple((2 * i + 1) % 4 for i in range(images))
    gpu_case((26, pred, target, 3), 3, native_calls)


@pytest.mark.parametrize("thresholds", [(0.5,), tuple((np.arange(16) + 1.0) / 16)])
def test_one_and_sixteen_thresholds(thresholds, native_calls):
    gpu_case((27, (40, 70, 9), (30, 66, 9), 3), 3, native_calls, thresholds=thresholds)


def test_all_scores_equal_and_all_boxes_identical(native_calls):
    gpu_case((28, (70, 5), (66, 70), 2, True, False), 2, native_calls)
    got, _ = gpu_case((29, (70, 5), (66, 70), 2, False, True), 2, native_calls)
    gpu_case((30, (70, 5), (66, 70), 1, True, True), 1, native_calls)
    # identical boxes: every IoU is 1, so every detection takes the last free ground truth of its class
    assert int(got[2].max()) == 2**10 - 1


def test_fractional_coordinates_decide_as_the_oracle(native_calls):
    # products that do not fit a double: a fused multiply-add anywhere in the IoU would show
    g = torch.Generator().manual_seed(31)
    counts = (60, 33)
    xy = torch.rand(93, 2, generator=g) * 50
    tb = torch.cat([xy, xy + torch.rand(93, 2, generator=g) * 30 + 0.1], dim=1)
    pb = tb + torch.randn(93, 4, generator=g) * 0.7
    pb[:, 2:] = torch.maximum(pb[:, 2:], pb[:, :2])
    ps = torch.rand(93, generator=g)
    lab = torch.randint(0, 2, (93,), generator=g)
    thr = oracle.default_thresholds()
    want = oracle.match(pb.numpy(), ps.numpy(), lab.numpy(), counts, tb.numpy(), lab.numpy(), counts, 2, thr, 100)
    got = _map_match(pb.to(DEV), ps.to(DEV), lab.to(DEV), list(counts), tb.to(DEV), lab.to(DEV), list(counts), 2,
                     torch.tensor(thr), 100, None, True)
    assert native_calls["match"] == 1
    check_match(got, want)


def test_an_image_over_the_cap_takes_the_aten_form(native_calls):
    key = (32, (CAP + 1, 4), (3, 2), 1)
    got, out = run_case(key, 1, device=DEV, thresholds=(0.5, 0.75))
    assert native_calls["match"] == 0 and native_calls["curve"] == 2  # the curves are K24's at any size
    assert all(t.is_cuda for t in got)
    key = (33, (5, 4), (CAP + 1, 2), 1)
    run_case(key, 1, device=DEV, thresholds=(0.5,), max_detections=3)
    assert native_calls["match"] == 0


# ----------------------------------------------------------------------------- curve shapes
@pytest.mark.parametrize("kind", ["random", "all hits", "no hits", "leading misses"])
def test_curve_segments_around_the_chunk(kind, native_calls):
    ch = K.CURVE_CHUNK
    sizes = (0, 1, ch - 1, ch, ch + 1, 3 * ch + 5, 0)
    g = torch.Generator().manual_seed(34)
    n, t = sum(sizes), 3
    labels = torch.cat([torch.full((s,), c, dtype=torch.int32) for c, s in enumerate(sizes)])
    if kind == "random":
        hits = torch.randint(0, 2**t, (n,), generator=g, dtype=torch.int32)
    elif kind == "all hits":
        hits = torch.full((n,), 2**t - 1, dtype=torch.int32)
    elif kind == "no hits":
        hits = torch.zeros(n, dtype=torch.int32)
    else:  # the first hit of every class behind misses, one of them a whole chunk deep
        hits = torch.zeros(n, dtype=torch.int32)
        start = 0
        for s in sizes:
            lead = min(s // 2, ch + 2)
            hits[start + lead:start + s] = torch.randint(0, 2**t, (s - lead,), generator=g, dtype=torch.int32)
            start += s
    scores = torch.tensor([0.9, 0.5, 0.5, 0.25])[torch.randint(0, 4, (n,), generator=g)]
    perm = torch.randperm(n, generator=g)  # stored order is not the global order
    scores, labels, hits = scores[perm], labels[perm], hits[perm]
    gt_count = torch.tensor([2.0, 1.0, 300.0, 256.0, 1000.0, 800.0, 0.0], dtype=torch.float64)
    ap, rec = oracle.tables(scores.numpy(), labels.numpy(), hits.numpy(), gt_count.numpy(), t)
    got = _map_tables(scores.to(DEV), labels.to(DEV), hits.to(DEV), gt_count.to(DEV), t)
    assert native_calls["curve"] == 1
    check_tables(*got, ap, rec)
    cpu = _map_tables(scores, labels, hits, gt_count, t)
    check_tables(*cpu, ap, rec)


# ----------------------------------------------------------------------------- dtypes
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_boxes_and_scores(dtype, native_calls):
    pb, ps, pl, pc, tb, tl, tc = case(35, (40, 9, 70), (30, 9, 66), 3)
    pb, ps, tb = pb.to(dtype), ps.to(dtype), tb.to(dtype)  # the coordinates are small integers: exact
    thr = oracle.default_thresholds()
    want = oracle.match(pb.float().numpy(), ps.float().numpy(), pl.numpy(), pc, tb.float().numpy(), tl.numpy(), tc,
                        3, thr, 100)
    got = _map_match(pb.to(DEV), ps.to(DEV), pl.to(DEV), list(pc), tb.to(DEV), tl.to(DEV), list(tc), 3,
                     torch.tensor(thr), 100, None, True)
    assert native_calls["match"] == 1
    check_match(got, want)
    out = mean_average_precision(pb.to(DEV), ps.to(DEV), pl.to(DEV), pc, tb.to(DEV), tl.to(DEV), tc, num_classes=3)
    check_values(out, *oracle.tables(*want[:4], 10), table(None))


def test_int32_labels(native_calls):
    gpu_case((36, (40, 9, 70), (30, 9, 66), 3), 3, native_calls, move=lambda pb, ps, pl, tb, tl: (pb, ps, pl.int(), tb, tl.int()))


def test_float64_boxes_take_the_aten_form(native_calls):
    run_case((37, (12, 6), (8, 7), 3), 3, device=DEV, move=lambda pb, ps, pl, tb, tl: (pb.double(), ps, pl, tb.double(), tl))
    assert native_calls["match"] == 0


# ----------------------------------------------------------------------------- bad input
def _bad_case():
    pb, ps, pl, pc, tb, tl, tc = case(38, (20, 9, 30), (12, 9, 25), 3)
    return [pb.clone(), ps.clone(), pl.clone(), list(pc), tb.clone(), tl.clone(), list(tc)]


@pytest.mark.parametrize("slot,row,col,value,bit", [
    (1, 3, None, float("nan"), K.BAD_SCORE),
    (0, 25, 1, float("inf"), K.BAD_COORDINATE),
    (4, 14, 2, float("nan"), K.BAD_COORDINATE),
    (0, 58, 2, -5.0, K.BAD_BOX),
    (4, 0, 3, -1.0, K.BAD_BOX),
    (2, 22, None, 3, K.BAD_LABEL),
    (5, 45, None, -1, K.BAD_LABEL),
])
def test_bad_rows_set_their_bit_are_counted_nowhere_and_raise_at_compute(slot, row, col, value, bit, native_calls):
    # the rows are valid memory; only their values are bad
    args = _bad_case()
    if col is None:
        args[slot][row] = value
    else:
        args[slot][row, col] = value
    # the same call without the bad row
    clean = _bad_case()
    counts_slot = 3 if slot < 3 else 6
    image = int(np.searchsorted(np.cumsum(clean[counts_slot]), row, side="right"))
    keep = torch.arange(sum(clean[counts_slot])) != row
    for s in ((0, 1, 2) if slot < 3 else (4, 5)):
        clean[s] = clean[s][keep]
    clean[counts_slot][image] -= 1
    want = mean_average_precision(*clean, num_classes=3)

    on_device = [a.to(DEV) if isinstance(a, torch.Tensor) else a for a in args]
    m = MeanAveragePrecision(3, device=DEV).update_packed(*on_device)
    assert native_calls["match"] == 1 and int(m._err) == bit
    with pytest.raises(ValueError, match="counted nowhere"):
        m.compute()
    assert int(m._err) == 0
    got = m.compute()  # the flag is cleared: the second compute answers
    for name in KEYS:
        torch.testing.assert_close(got[name].cpu(), want[name], rtol=0, atol=2.0**-23, equal_nan=True)
    assert int(m.gt_count.sum()) == sum(clean[6]) and sum(int((l >= 0).sum()) for l in m.det_labels) == sum(clean[3])
    # the functional raises only under config.validate
    out = mean_average_precision(*on_device, num_classes=3)
    for name in KEYS:
        torch.testing.assert_close(out[name].cpu(), want[name], rtol=0, atol=2.0**-23, equal_nan=True)
    with flags(validate=True):
        with pytest.raises(ValueError, match="counted nowhere"):
            mean_average_precision(*on_device, num_classes=3)


# ----------------------------------------------------------------------------- determinism, the class
def test_two_runs_are_bit_identical(native_calls):
    pb, ps, pl, pc, tb, tl, tc = (a.to(DEV) if isinstance(a, torch.Tensor) else a
                                  for a in case(39, tuple([100] * 64), tuple([7] * 64), 80))
    thr = torch.tensor(oracle.default_thresholds())
    runs = [_map_match(pb, ps, pl, list(pc), tb, tl, list(tc), 80, thr, 100, None, True) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b)
    outs = [mean_average_precision(pb, ps, pl, pc, tb, tl, tc, num_classes=80) for _ in range(2)]
    tabs = [_map_tables(*runs[i][:4], 10) for i in range(2)]
    for name in KEYS:
        assert torch.equal(outs[0][name].view(torch.int32), outs[1][name].view(torch.int32))
    assert torch.equal(tabs[0][0].view(torch.int64), tabs[1][0].view(torch.int64))
    assert torch.equal(tabs[0][1].view(torch.int64), tabs[1][1].view(torch.int64))


def test_class_updates_are_one_native_launch_each(native_calls):
    key = (40, (30, 0, 64, 12), (20, 3, 66, 0), 5)
    pb, ps, pl, pc, tb, tl, tc = (a.to(DEV) if isinstance(a, torch.Tensor) else a for a in case(*key))
    m = MeanAveragePrecision(5, device=DEV)
    m.update_packed(pb[:30], ps[:30], pl[:30], [30, 0], tb[:23], tl[:23], [20, 3])
    m.update_packed(pb[30:], ps[30:], pl[30:], [64, 12], tb[23:], tl[23:], [66, 0])
    assert native_calls == {"match": 2, "curve": 0}
    got = m.compute()
    assert native_calls == {"match": 2, "curve": 1}
    want = want_match(key, 5, table(None), 100)
    check_values(got, *oracle.tables(*want[:4], 10), table(None))
    assert m.gt_count.is_cuda and m.gt_count.cpu().tolist() == want[3].astype(np.float64).tolist()
