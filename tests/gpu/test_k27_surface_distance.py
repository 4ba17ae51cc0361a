"""K27 (csrc/kernels/surface_distance.hip) on MI355X: Hausdorff and average surface distance against the
float64 brute-force oracle of tests/_surface_distance_oracle.py, under its derived tolerance (two float32
ulps, NaN and +inf in place).  The cases are the smallest at which the row scan, the column search or
the select can go wrong; tests/_surface_distance_oracle.py draws them.  A test item is a case: its label
dtypes and modes run inside it."""

import pytest
import torch

import torcheval_amd.metrics.functional as MF
from tests._surface_distance_oracle import CASES, MODES, call, case, check
from torcheval_amd.metrics import AverageSurfaceDistance, HausdorffDistance
from torcheval_amd.ops import surface_distance as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NATIVE = [name for name in CASES if name != "too_wide"]


def _run(name, mode, dtype=torch.int64):
    p, t, num_classes, background, want = case(name, mode)
    fn, kw = call(MF, mode)
    got = fn(p.to(DEV, dtype), t.to(DEV, dtype), num_classes=num_classes, include_background=background, **kw)
    check(got, want)
    return got


@pytest.mark.parametrize("name", NATIVE)
def test_against_oracle(name, monkeypatch):
    """Every label dtype and mode of the case; the combination is printed before it is checked."""
    launched = []
    op = K.surface_distance
    monkeypatch.setattr(K, "surface_distance", lambda *a, **k: launched.append(1) or op(*a, **k))
    for dtype in (torch.uint8, torch.int64):
        for mode in MODES:
            print(name, dtype, mode)
            got = _run(name, mode, dtype)
            assert got.is_cuda and len(launched) % 2 == 1
            # bitwise, NaN included
            assert torch.equal(got.view(torch.int32), _run(name, mode, dtype).view(torch.int32))
    assert len(launched) == 4 * len(MODES)


def test_above_the_native_limit_takes_the_aten_form(monkeypatch):
    monkeypatch.setattr(K, "surface_distance", lambda *a, **k: pytest.fail("K27 launched"))
    for mode in ("p95", "assd"):
        assert _run("too_wide", mode).is_cuda


def test_chunks_of_whole_images_and_mixed_dtypes(monkeypatch):
    monkeypatch.setattr(K, "WORKSPACE_CAP", 1)  # one image per call of the op
    assert K.images_per_call(2, 9, 129) == 1
    for mode in ("p50", "asd"):
        p, t, num_classes, background, want = case("w129", mode)
        fn, kw = call(MF, mode)
        check(fn(p.to(DEV, torch.int16), t.to(DEV, torch.int32), num_classes=num_classes, **kw), want)


@pytest.mark.parametrize("mode", ["p95", "assd"])
def test_class_updates_states_in_the_state_buffer(mode):
    from torcheval_amd.parallel.state_buffer import buffer_of

    p, t, num_classes, background, want = case("hand", mode)
    cls, kw = (AverageSurfaceDistance, {}) if mode == "assd" else (HausdorffDistance, {"percentile": 95})
    m = cls(num_classes=num_classes, include_background=background, average=None, device=DEV, **kw)
    sb = buffer_of(m)
    ptrs = [getattr(m, s).data_ptr() for s in ("distance_sum", "num_finite", "num_inf")]
    m.update(p[:1].to(DEV), t[:1].to(DEV)).update(p[1:].to(DEV), t[1:].to(DEV))
    lo, hi = sb.buf.data_ptr(), sb.buf.data_ptr() + sb.buf.numel() * sb.buf.element_size()
    assert [getattr(m, s).data_ptr() for s in ("distance_sum", "num_finite", "num_inf")] == ptrs
    assert all(lo <= q < hi for q in ptrs)
    values = torch.from_numpy(want).float().double()
    finite = values.isfinite()
    assert torch.equal(m.num_finite.cpu(), finite.sum(0).double())
    assert torch.equal(m.num_inf.cpu(), values.isinf().sum(0).double())
    check(m.compute().unsqueeze(0), (torch.where(finite, values, 0.0).sum(0) / finite.sum(0)).unsqueeze(0).numpy())
