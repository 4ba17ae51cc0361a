"""K26 (csrc/kernels/msssim.hip) on MI355X: multi-scale SSIM against the float64 CPU oracle of
tests/_msssim_oracle.py, under its tolerance rule (4 x the error of the oracle's own float32 form on the
same inputs + 1e-6).  The shapes are the smallest at which the tiling, the pooling ownership or the level
offsets can go wrong; those at tile and halo edges are derived from the extension's tile constants."""

import functools
import math

import pytest
import torch

from tests._msssim_oracle import check, images, oracle
from torcheval_amd.metrics import MultiScaleStructuralSimilarity
from torcheval_amd.metrics.functional import multiscale_structural_similarity, structural_similarity
from torcheval_amd.ops import msssim as K
from torcheval_amd.ops import native_loaded
from torcheval_amd.ops import ssim as K12

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TH, TW = K12.tile_shape() if native_loaded() else (64, 64)  # (only ever run with the extension)
B2, B3, B4 = (0.5, 0.5), (0.3, 0.3, 0.4), (0.2, 0.2, 0.3, 0.3)


@functools.lru_cache(maxsize=None)
def _case(shape, seed, kind="rand"):
    """CPU images of a case, shared by the tests that use it (never modified): the noise grows with
    the image and the channel, so every plane has a value of its own."""
    x, y = images(shape, seed, kind)
    scale = 1 + torch.arange(shape[0] * shape[1]).view(shape[0], shape[1], 1, 1) / 2.0
    y = x + (y - x) * scale
    return x, y.clamp(0, 255).round() if kind == "uint8" else y.clamp(0, 1)


def _run(x, y, data_range=1.0, **kw):
    """Both reductions on the device, checked against the oracle; returns the per-image values."""
    xd, yd = x.to(DEV), y.to(DEV)
    api = {("kernel_size" if k == "ks" else k): v for k, v in kw.items()}
    assert K.supported(xd, yd, kw.get("ks", 11), len(kw.get("betas", (0,) * 5)))
    got = multiscale_structural_similarity(xd, yd, data_range, reduction="none", **api)
    check(got, x.double(), y.double(), data_range=data_range, **kw)
    check(multiscale_structural_similarity(xd, yd, data_range, **api), x.double(), y.double(), "mean",
          data_range=data_range, **kw)
    return got


CASES = {
    # every level in the tail launch; one output pixel at the last level
    "tail5": ((2, 3, 56, 48), {"ks": 3}),
    "tail4": ((2, 3, 48, 40), {"ks": 3, "betas": B4}),
    "tail_one_pixel": ((1, 1, 22, 22), {"betas": B2}),
    # level 1 fits the halo exactly, or is one past it (then a level launch of its own)
    "fits": ((1, 2, 2 * (TH + 10), 112), {"betas": B4}),
    "fits_w": ((1, 2, 112, 2 * (TW + 10)), {"betas": B4}),
    "one_past": ((1, 2, 2 * (TH + 10) + 2, 2 * (TW + 10)), {"betas": B4}),
    "one_past_w": ((1, 2, 112, 2 * (TW + 10) + 2), {"betas": B4}),
    # pooling across tile edges: two tiles, an odd side whose last row / column is dropped
    "edge_rows": ((2, 2, 2 * TH + 11, TW + 11), {"betas": B2}),
    "edge_cols": ((2, 2, TH + 11, 2 * TW + 11), {"betas": B2}),
    "edge_both": ((2, 2, 2 * TH + 11, 2 * TW + 11), {"betas": B2}),
    # the runtime-window arm: the smallest three-level shape of each size, and one with level launches
    "ks3": ((2, 2, 12, 12), {"ks": 3, "betas": B3}),
    "ks7": ((2, 2, 28, 28), {"ks": 7, "betas": B3}),
    "ks15": ((2, 2, 60, 60), {"ks": 15, "betas": B3}),
    "ks7_levels": ((1, 2, TH + 8, 2 * TW + 9), {"ks": 7, "betas": B3}),
}


@pytest.mark.parametrize("name", CASES)
def test_against_oracle(name):
    shape, kw = CASES[name]
    x, y = _case(shape, 40)
    got = _run(x, y, **kw)
    assert float((got[0] - got[-1]).abs()) > 1e-3 or shape[0] == 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16, torch.uint8])
def test_dtypes(dtype):
    kind, rng = ("uint8", 255.0) if dtype == torch.uint8 else ("rand", 1.0)
    x, y = _case((2, 2, 60, TW + 11), 41, kind)  # two tiles at level 0, then the tail
    _run(x.to(dtype), y.to(dtype), rng, betas=B3)  # the oracle sees the values after the dtype's rounding


@pytest.mark.parametrize("shape", [(2, 2, 60, TW + 11), (2, 3, 30, 41)])
def test_one_level_with_unit_exponent_is_k12(shape):
    x, y = _case(shape, 42)
    got = _run(x, y, betas=(1.0,))
    ssim = structural_similarity(x.to(DEV), y.to(DEV), reduction="none")
    assert float((got - ssim).abs().max()) <= oracle(x, y, betas=(1.0,))[1]


def test_special_values_and_determinism():
    x, y = _case((3, 2, 2 * TH + 11, TW + 11), 43)
    xd, yd = x.to(DEV), y.to(DEV)
    one = multiscale_structural_similarity(xd, xd.clone(), betas=B3, reduction="none")
    assert float((one - 1).abs().max()) <= 1e-6
    a = multiscale_structural_similarity(xd, yd, betas=B3, reduction="none")
    assert torch.equal(a, multiscale_structural_similarity(xd, yd, betas=B3, reduction="none"))
    assert torch.equal(multiscale_structural_similarity(xd, yd, betas=B3),
                       multiscale_structural_similarity(xd, yd, betas=B3))
    xn = xd.clone()
    xn[1, 1, 2 * TH + 9, TW + 9] = math.nan  # the last pooled pixel of the last tile
    got = multiscale_structural_similarity(xn, yd, betas=B3, reduction="none")
    assert got.isnan().tolist() == [False, True, False] and torch.equal(got[[0, 2]], a[[0, 2]])
    assert multiscale_structural_similarity(xn, yd, betas=B3).isnan()


def test_float64_and_large_window_take_the_aten_path(monkeypatch):
    x, y = _case((2, 2, 70, 75), 44)
    monkeypatch.setattr(K, "msssim", lambda *a, **k: pytest.fail("K26 launched"))
    for xi, kw in ((x.double(), {}), (x, {"ks": 17})):
        xd, yd = xi.to(DEV), y.to(xi.dtype).to(DEV)
        assert not K.supported(xd, yd, kw.get("ks", 11), 2)
        got = multiscale_structural_similarity(xd, yd, kernel_size=kw.get("ks", 11), betas=B2, reduction="none")
        assert got.is_cuda
        check(got, x, y, betas=B2, **kw)
        if xi.dtype == torch.float64:  # computed in float64: the oracle rounded once
            assert float((got.double().cpu() - oracle(x, y, betas=B2)[0]).abs().max()) <= 1e-7


def test_class_updates_states_in_the_state_buffer():
    from torcheval_amd.parallel.state_buffer import buffer_of

    x, y = _case((5, 2, 60, TW + 11), 45)
    m = MultiScaleStructuralSimilarity(betas=B3, device=DEV)
    sb = buffer_of(m)
    ptrs = (m.msssim_sum.data_ptr(), m.num_images.data_ptr())
    m.update(x[:2].to(DEV), y[:2].to(DEV)).update(x[2:3].to(DEV), y[2:3].to(DEV))
    other = MultiScaleStructuralSimilarity(betas=B3, device=DEV).update(x[3:].to(DEV), y[3:].to(DEV))
    m.merge_state([other])
    lo, hi = sb.buf.data_ptr(), sb.buf.data_ptr() + sb.buf.numel() * sb.buf.element_size()
    assert (m.msssim_sum.data_ptr(), m.num_images.data_ptr()) == ptrs and all(lo <= p < hi for p in ptrs)
    assert m.msssim_sum.dtype == torch.float64 and m.num_images.dtype == torch.float64
    assert float(m.num_images) == 5.0
    check(m.compute(), x, y, "mean", betas=B3)
