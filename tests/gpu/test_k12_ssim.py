"""K12 (csrc/kernels/ssim.hip) on MI355X: structural similarity against the FP64 CPU oracle of
tests/metrics/image/test_ssim.py, under that file's tolerance rule (4 x the error of the float32
form on the same inputs + 1e-6).  The shapes are the smallest at which the tiling can go wrong;
those at tile edges are derived from the tile constants the extension exports."""

import functools
import math

import pytest
import torch

import torcheval_amd.ops as ops
from tests.metrics.image.test_ssim import _form, check, images, oracle
from torcheval_amd.metrics import StructuralSimilarity
from torcheval_amd.metrics.functional import structural_similarity
from torcheval_amd.ops import ssim as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _tile():
    return K.tile_shape()


@functools.lru_cache(maxsize=None)
def _case(shape, seed, kind="rand"):
    """CPU images of a case, shared by the tests that use it (never modified)."""
    return images(shape, seed, kind)


def _run(x, y, *args, **kw):
    return structural_similarity(x.to(DEV), y.to(DEV), *args, **kw)


@pytest.fixture
def native_calls(monkeypatch):
    """Counts the launches through the K12 wrapper: the native path really ran."""
    calls = []
    real = K.ssim

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(K, "ssim", spy)
    return calls


# ----------------------------------------------------------------------------- tile geometry
def test_one_output_pixel(native_calls):
    x, y = _case((1, 1, 11, 11), 20)
    check(_run(x, y, reduction="none"), x, y)
    check(_run(x, y), x, y, "mean")
    assert len(native_calls) == 2


def test_one_column_and_one_row_past_a_tile_edge():
    th, tw = _tile()
    for shape in ((1, 1, 12, tw + 11), (1, 1, th + 11, 12), (2, 1, th + 11, tw + 11)):
        x, y = _case(shape, 21)
        check(_run(x, y, reduction="none"), x, y)


def test_exact_tile_and_one_short():
    th, tw = _tile()
    for shape in ((1, 2, th + 10, tw + 10), (1, 1, th + 9, tw + 9)):
        x, y = _case(shape, 22)
        check(_run(x, y, reduction="none"), x, y)


def test_plane_indexing_with_distinct_images():
    x, y = _case((3, 3, 37, 131), 23)
    y = y.clone()
    y[1] = 1 - y[1]
    y[2] = y[2] * 0.5
    want, _ = oracle(x, y)
    assert float((want[0] - want[1]).abs()) > 0.1 and float((want[1] - want[2]).abs()) > 0.1
    check(_run(x, y, reduction="none"), x, y)


def test_several_tiles_in_both_directions():
    x, y = _case((2, 3, 300, 260), 24)
    check(_run(x, y, reduction="none"), x, y)
    check(_run(x, y), x, y, "mean")


def test_more_planes_than_65535():
    x, y = _case((66000, 1, 11, 11), 25)
    got = _run(x, y, reduction="none")
    check(got, x, y)
    check(_run(x, y), x, y, "mean")


# ----------------------------------------------------------------------------- dtypes, layouts
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16, torch.uint8])
def test_dtypes(dtype, native_calls):
    if dtype == torch.uint8:
        x, y = _case((2, 3, 37, 131), 26, "uint8")
        kw = {"data_range": 255.0}
    else:
        x, y = _case((2, 3, 37, 131), 26)
        kw = {}
    xq, yq = x.to(dtype), y.to(dtype)  # the oracle sees the values after the dtype's rounding
    got = _run(xq, yq, kw.get("data_range", 1.0), reduction="none")
    check(got, xq.double(), yq.double(), **kw)
    assert len(native_calls) == 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.uint8])
def test_odd_width_view_off_16_byte_alignment(dtype):
    shape = (2, 2, 13, 77)
    x, y = _case(shape, 27, "uint8" if dtype == torch.uint8 else "rand")
    xq, yq = x.to(dtype), y.to(dtype)
    n = xq.numel()
    bx, by = torch.zeros(n + 1, dtype=dtype, device=DEV), torch.zeros(n + 3, dtype=dtype, device=DEV)
    vx, vy = bx[1:].view(shape), by[3:].view(shape)  # contiguous, bases 1 and 3 elements in
    vx.copy_(xq)
    vy.copy_(yq)
    assert vx.is_contiguous() and vx.data_ptr() % 16 != 0
    rng = 255.0 if dtype == torch.uint8 else 1.0
    check(structural_similarity(vx, vy, rng, reduction="none"), xq.double(), yq.double(), data_range=rng)


def test_channels_last_equals_its_contiguous_copy():
    x, y = _case((2, 3, 20, 70), 28)
    xc, yc = x.to(DEV), y.to(DEV)
    xl, yl = xc.contiguous(memory_format=torch.channels_last), yc.contiguous(memory_format=torch.channels_last)
    assert not xl.is_contiguous()
    a = structural_similarity(xl, yl, reduction="none")
    b = structural_similarity(xc, yc, reduction="none")
    assert torch.equal(a, b)
    check(a, x, y)
    sliced = torch.rand(2, 3, 20, 140, device=DEV)[..., ::2]
    check(structural_similarity(sliced, sliced.flip(0), reduction="none"), sliced.cpu(), sliced.flip(0).cpu())


# ----------------------------------------------------------------------------- window sizes
@pytest.mark.parametrize("ks", [3, 7, 15])
def test_runtime_window_sizes(ks, native_calls):
    th, tw = _tile()
    x, y = _case((2, 2, th + ks + 2, tw + ks + 2), 29)
    check(_run(x, y, kernel_size=ks, reduction="none"), x, y, ks=ks)
    check(_run(x, y, kernel_size=ks, sigma=0.5 + ks / 6, reduction="none"), x, y, ks=ks, sigma=0.5 + ks / 6)
    assert len(native_calls) == 2


def test_large_window_and_float64_take_the_aten_path(native_calls):
    x, y = _case((2, 2, 40, 45), 30)
    check(_run(x, y, kernel_size=17, reduction="none"), x, y, ks=17)
    got = _run(x.double(), y.double(), reduction="none")
    assert got.dtype == torch.float32 and got.is_cuda
    check(got, x, y)
    check(_run(x.half(), y, reduction="none"), x.half().double(), y)  # mixed dtypes
    assert native_calls == []


# ----------------------------------------------------------------------------- special values
def test_near_flat_images():
    x, y = _case((2, 3, 37, 131), 31, "flat")
    check(_run(x, y, reduction="none"), x, y)


def test_constant_images_are_exact_to_float32_rounding():
    """The kernel shifts both inputs by the tile's first pixel, so constant images have exactly
    zero shifted moments: mx = a, my = b, every variance 0, and what is left is two FMAs and a
    product per factor, the quotient and the final rounding to float32 - below 4 eps."""
    a, b = 0.3, 0.7
    x, y = torch.full((2, 1, 45, 80), a), torch.full((2, 1, 45, 80), b)
    af, bf = float(torch.tensor(a)), float(torch.tensor(b))  # the float32 values the kernel sees
    c1 = 0.01**2
    want = (2 * af * bf + c1) / (af * af + bf * bf + c1)
    got = _run(x, y, reduction="none")
    assert float((got.double().cpu() - want).abs().max()) <= 4 * torch.finfo(torch.float32).eps * want


def test_nan_stays_in_its_image():
    x, y = _case((3, 2, 40, 70), 32)
    x = x.clone()
    x[1, 1, 35, 68] = math.nan
    got = _run(x, y, reduction="none")
    assert got.isnan().tolist() == [False, True, False]
    check(got[[0, 2]], x[[0, 2]], y[[0, 2]])
    assert _run(x, y).isnan()


def test_identical_images_give_one():
    x, _ = _case((2, 3, 37, 131), 33)
    got = _run(x, x.clone(), reduction="none")
    assert float((got - 1).abs().max()) <= 1e-6


def test_two_runs_are_bit_identical():
    x, y = _case((2, 3, 300, 260), 24)
    xd, yd = x.to(DEV), y.to(DEV)
    a = structural_similarity(xd, yd, reduction="none")
    b = structural_similarity(xd, yd, reduction="none")
    assert torch.equal(a, b)
    assert torch.equal(structural_similarity(xd, yd), structural_similarity(xd, yd))


def test_aten_cross_check(monkeypatch):
    x, y = _case((2, 3, 37, 131), 34)
    native = _run(x, y, reduction="none")
    monkeypatch.setattr(ops, "DISABLE_HIP", True)

    def no_kernel(*a, **k):
        raise AssertionError("K12 launched with TORCHEVAL_AMD_DISABLE_HIP set")

    monkeypatch.setattr(K, "ssim", no_kernel)
    aten = _run(x, y, reduction="none")
    assert aten.is_cuda
    check(aten, x, y)
    check(native, x, y)
    m = StructuralSimilarity(device=DEV).update(x.to(DEV), y.to(DEV))
    check(m.compute(), x, y, "mean")


# ----------------------------------------------------------------------------- class API
def test_class_updates_states_in_the_state_buffer(native_calls):
    from torcheval_amd.parallel.state_buffer import buffer_of

    x, y = _case((6, 3, 37, 131), 35)
    m = StructuralSimilarity(device=DEV)
    sb = buffer_of(m)
    assert sb is not None
    ptrs = (m.mssim_sum.data_ptr(), m.num_images.data_ptr())
    for lo, hi in ((0, 1), (1, 4), (4, 6)):
        m.update(x[lo:hi].to(DEV), y[lo:hi].to(DEV))
    assert len(native_calls) == 3
    assert buffer_of(m, build=False) is sb and (m.mssim_sum.data_ptr(), m.num_images.data_ptr()) == ptrs
    lo, hi = sb.buf.data_ptr(), sb.buf.data_ptr() + sb.buf.numel()
    assert all(lo <= p < hi for p in ptrs)
    assert m.mssim_sum.dtype == torch.float64 and m.num_images.dtype == torch.float64
    assert float(m.num_images) == 6.0
    got = m.compute()
    assert got.dtype == torch.float32 and got.is_cuda
    check(got, x, y, "mean")
    torch.testing.assert_close(m.mssim_sum.cpu(), _form(x, y).sum(), rtol=0, atol=6 * oracle(x, y)[1])
    moved = m.to("cpu")
    assert moved.mssim_sum.device.type == "cpu"
    check(moved.compute(), x, y, "mean")
    m.reset()
    assert float(m.num_images) == 0.0 and m.compute().isnan()


def test_class_merge_state():
    x, y = _case((6, 3, 37, 131), 35)
    a = StructuralSimilarity(device=DEV).update(x[:2].to(DEV), y[:2].to(DEV))
    b = StructuralSimilarity(device=DEV).update(x[2:].to(DEV), y[2:].to(DEV))
    a.merge_state([b])
    assert float(a.num_images) == 6.0 and float(b.num_images) == 4.0
    check(a.compute(), x, y, "mean")


def test_class_sync_and_compute_one_rank():
    import socket

    import torch.distributed as dist

    from torcheval_amd.metrics.toolkit import sync_and_compute
    from torcheval_amd.parallel.collectives import collectives_at_world_size_1

    x, y = _case((6, 3, 37, 131), 35)
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=DEV)
    try:
        m = StructuralSimilarity(device=DEV).update(x.to(DEV), y.to(DEV))
        local = m.compute().clone()
        with collectives_at_world_size_1():
            torch.testing.assert_close(sync_and_compute(m), local, rtol=0, atol=0)
        torch.testing.assert_close(m.compute(), local, rtol=0, atol=0)
        check(local, x, y, "mean")
    finally:
        dist.destroy_process_group()
