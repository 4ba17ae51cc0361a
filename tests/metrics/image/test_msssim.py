"""Multi-scale SSIM on CPU tensors: the ATen form and the class against the float64 oracle of
tests/_msssim_oracle.py, under its tolerance rule."""

import pytest
import torch

import torcheval_amd.metrics as M
import torcheval_amd.metrics.functional as MF
import torcheval_amd.metrics.functional.image as MFI
import torcheval_amd.metrics.image as MI
import torcheval_amd.ops as ops
from tests._msssim_oracle import check, images, terms, values
from torcheval_amd.metrics import MultiScaleStructuralSimilarity
from torcheval_amd.metrics.functional import multiscale_structural_similarity, structural_similarity

# (shape, kind, oracle keywords); odd sizes drop a row or a column at every pooling
CASES = [
    ((2, 3, 176, 180), "rand", {}),
    ((2, 2, 53, 49), "rand", {"ks": 3}),
    ((1, 2, 45, 51), "uint8", {"ks": 7, "betas": (0.3, 0.3, 0.4), "data_range": 255.0}),
    ((2, 1, 31, 30), "rand", {"ks": 15, "sigma": 2.5, "betas": (0.5, 0.5)}),
]


def _api(kw):
    out = dict(kw)
    if "ks" in out:
        out["kernel_size"] = out.pop("ks")
    return out


@pytest.mark.parametrize("reduction", ["none", "mean"])
@pytest.mark.parametrize("shape,kind,kw", CASES)
def test_functional_against_oracle(shape, kind, kw, reduction):
    x, y = images(shape, 1, kind)
    assert float(terms(x, y, **kw).min()) > 0.2  # x^beta is well-conditioned on these inputs
    check(multiscale_structural_similarity(x, y, reduction=reduction, **_api(kw)), x, y, reduction, **kw)


@pytest.mark.parametrize("shape,kind,kw", CASES)
def test_float64_inputs_are_the_oracle_rounded_once(shape, kind, kw):
    """Pins the ATen form absolutely: computed in float64, its only error is the rounding to float32."""
    x, y = images(shape, 2, kind)
    got = multiscale_structural_similarity(x.double(), y.double(), reduction="none", **_api(kw))
    assert got.dtype == torch.float32
    torch.testing.assert_close(got.double(), values(x, y, **kw), rtol=0, atol=1e-7)


def test_one_level_with_unit_exponent_is_ssim():
    x, y = images((2, 3, 24, 31), 2)
    got = multiscale_structural_similarity(x, y, betas=(1.0,), reduction="none")
    torch.testing.assert_close(got, structural_similarity(x, y, reduction="none"), rtol=0, atol=1e-6)


def test_product_is_taken_per_channel():
    x, y = images((1, 2, 44, 44), 3)
    y[:, 1] = (x[:, 1] + 0.3 * torch.randn(44, 44, generator=torch.Generator().manual_seed(4))).clamp(0, 1)
    kw = {"betas": (1.0, 1.0)}
    t = terms(x, y, **kw)  # [M, 1, 2]
    per_channel, per_image = t.prod(0).mean(1), t.mean(2).prod(0)
    assert float((per_channel - per_image).abs()) > 1e-3
    got = multiscale_structural_similarity(x.double(), y.double(), reduction="none", **kw)
    torch.testing.assert_close(got.double(), per_channel, rtol=0, atol=1e-7)  # float64, rounded once


def test_odd_last_row_and_column_are_dropped():
    """With a zero exponent at level 0 only level 1 counts, and it never sees row 44 or column 46."""
    x, y = images((1, 1, 45, 47), 5)
    kw = {"betas": (0.0, 1.0), "reduction": "none"}
    want = multiscale_structural_similarity(x, y, **kw)
    x2, y2 = x.clone(), y.clone()
    x2[..., 44, :], y2[..., :, 46] = 1.0, 0.0
    assert torch.equal(multiscale_structural_similarity(x2, y2, **kw), want)
    assert torch.equal(multiscale_structural_similarity(x[..., :44, :46], y[..., :44, :46], **kw), want)


def test_invalid_arguments():
    x = torch.rand(2, 3, 176, 176)
    with pytest.raises(ValueError, match="at least 176 for 5 levels"):
        multiscale_structural_similarity(x[..., :175], x[..., :175])
    with pytest.raises(ValueError, match="at least 12 for 3 levels"):
        MultiScaleStructuralSimilarity(kernel_size=3, betas=(0.3, 0.3, 0.4)).update(x[:, :, :11], x[:, :, :11])
    for betas in ((), [0.5, 0.5], (0.5, -0.1), (1,), (float("nan"),)):
        with pytest.raises(ValueError, match="`betas` needs to be a non-empty `tuple`"):
            multiscale_structural_similarity(x, x, betas=betas)
    with pytest.raises(ValueError, match="`betas`"):
        MultiScaleStructuralSimilarity(betas=())
    with pytest.raises(ValueError, match="same shape"):
        multiscale_structural_similarity(x, x[:1])
    with pytest.raises(ValueError, match="`kernel_size` needs to be an odd `int`"):
        multiscale_structural_similarity(x, x, kernel_size=8)
    with pytest.raises(ValueError, match="`reduction`"):
        multiscale_structural_similarity(x, x, reduction="sum")
    empty = multiscale_structural_similarity(x[:0], x[:0], reduction="none")
    assert empty.shape == (0,) and multiscale_structural_similarity(x[:0], x[:0]).isnan()


def test_class_update_merge_compute():
    x, y = images((5, 2, 48, 50), 6)
    kw = {"ks": 7, "betas": (0.2, 0.3, 0.5)}
    a = MultiScaleStructuralSimilarity(**_api(kw)).update(x[:1], y[:1]).update(x[1:3], y[1:3])
    b = MultiScaleStructuralSimilarity(**_api(kw)).update(x[3:], y[3:])
    assert MultiScaleStructuralSimilarity().compute().isnan()
    a.merge_state([b])
    assert a.msssim_sum.dtype == torch.float64 and a.num_images.dtype == torch.float64
    assert float(a.num_images) == 5.0 and float(b.num_images) == 2.0
    check(a.compute(), x, y, "mean", **kw)
    c = MultiScaleStructuralSimilarity(**_api(kw))
    c.load_state_dict(a.state_dict())
    assert torch.equal(c.compute(), a.compute())
    a.reset()
    assert float(a.num_images) == 0.0 and a.compute().isnan()


def test_exports():
    assert M.MultiScaleStructuralSimilarity is MI.MultiScaleStructuralSimilarity is MultiScaleStructuralSimilarity
    assert MF.multiscale_structural_similarity is MFI.multiscale_structural_similarity
    assert "MultiScaleStructuralSimilarity" in MI.__all__ and "multiscale_structural_similarity" in MFI.__all__
    # the top-level lists mirror the reference's public names, which have no MS-SSIM
    assert "MultiScaleStructuralSimilarity" not in M.__all__ and "multiscale_structural_similarity" not in MF.__all__


@pytest.mark.skipif(not ops.native_loaded(), reason="extension not built")
def test_op_schema_and_meta_kernel():
    from torcheval_amd.ops import msssim as K

    op = torch.ops.torcheval_amd_msssim.msssim.default
    schema = str(op._schema)
    for part in ("Tensor(a!) workspace", "Tensor(b!) partials", "Tensor(c!)? out", "Tensor(d!)? value_sum",
                 "Tensor(e!)? num_images", "float[] betas"):
        assert part in schema
    for key in ("CUDA", "Meta"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key("torcheval_amd_msssim::msssim", key)
    x = torch.empty(2, 3, 256, 256, device="meta")
    s = torch.empty((), dtype=torch.float64, device="meta")
    assert K.msssim(x, x, (0.25, 0.5, 0.25), (0.5, 0.5), 1e-4, 9e-4, None, False, s, s) is None
    # 256 and 128 are level launches of 16 and 4 tiles, the 64-pixel level and below are the tail
    p = K.plan(256, 256, 11, 5)
    assert (p["tail"], p["per"], p["partials"]) == (2, [16, 4, 1, 1, 1], 23)
    assert (p["ws_off"], p["ws_pairs"]) == ([0, 0, 128 * 128, 0, 0], 128 * 128 + 64 * 64)
    assert p["ws_pairs"] * 2 <= 256 * 256 * 2 // 3
