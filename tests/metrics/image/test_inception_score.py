"""Inception Score (not in the reference tree; definition in docs/parity.md).

Oracle: tests/_inception_oracle.py, numpy FP64 of the definition.  CPU tensors run the ATen form;
tests/gpu/test_k21_inception_score.py runs the same oracle against K21.

``split_log`` of the float32 ATen form must lie within 1e-6 of the oracle (measured on the CPU: 4e-9
to 2e-8 at the shapes below and at 50000 x 1000), float64 logits within 1e-12.
"""

import math
import os
import pickle
import re
import warnings

import numpy as np
import pytest
import torch

import torcheval_amd.metrics as M
import torcheval_amd.metrics.functional as MF
import torcheval_amd.metrics.functional.image as MFI
import torcheval_amd.metrics.image as MI
import torcheval_amd.ops as ops
from tests import _inception_oracle as O
from torcheval_amd.metrics import InceptionScore
from torcheval_amd.metrics.functional import inception_score
from torcheval_amd.metrics.functional.image.inception_score import _inception_score_stats, _inception_score_values
from torcheval_amd.utils.test_utils import MetricClassTester
from torcheval_amd.utils.test_utils.dist_pool import run_distributed

NAN, INF = math.nan, math.inf


def logits(n: int, c: int, seed: int, dtype=torch.float32) -> torch.Tensor:
    """Seeded logits within [-8, 8]."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, c, generator=g, dtype=torch.float64) * 3).clamp(-8, 8).to(dtype)


def check_states(got, want, rtol=1e-12):
    for g, w in zip(got, want):
        assert g.dtype == torch.float64 and tuple(g.shape) == w.shape
        np.testing.assert_allclose(g.numpy(), w, rtol=rtol, atol=0, equal_nan=True)


def metric(c: int, splits: int, **kw) -> InceptionScore:
    return InceptionScore(model=torch.nn.Identity(), num_classes=c, splits=splits, **kw)


# ----------------------------------------------------------------------------- values
@pytest.mark.parametrize("n,c,splits", [(777, 65, 10), (4096, 1000, 10), (37, 70, 4)])
def test_values_against_the_oracle(n, c, splits):
    x = logits(n, c, n + c)
    want_log, want_mean, want_std = O.values(*O.stats(x.double().numpy(), splits))
    states = _inception_score_stats(x, splits)
    assert [tuple(s.shape) for s in states] == [(splits, c), (splits,), (splits,)]
    assert torch.equal(states[2], torch.from_numpy(O.stats(x.double().numpy(), splits)[2]))
    split_log, mean, std = _inception_score_values(*states)
    assert split_log.dtype == torch.float64 and split_log.shape == (splits,)
    err = float(np.abs(split_log.numpy() - want_log).max())
    print(f"inception {n}x{c} S={splits}: float32 ATen split_log error {err:.2e}")
    assert err <= 1e-6
    got = inception_score(x, splits=splits)
    assert all(v.dtype == torch.float32 and v.shape == () for v in got)
    assert torch.equal(got[0], mean) and torch.equal(got[1], std)
    assert float(mean) == pytest.approx(want_mean, rel=2e-6) and float(std) == pytest.approx(want_std, rel=1e-4, abs=1e-6)
    # float64 logits
    xd = x.double()
    states = _inception_score_stats(xd, splits)
    check_states(states, O.stats(xd.numpy(), splits))
    split_log, mean, std = _inception_score_values(*states, dtype=torch.float64)
    np.testing.assert_allclose(split_log.numpy(), want_log, rtol=0, atol=1e-12)
    got = inception_score(xd, splits=splits)
    assert all(v.dtype == torch.float64 and v.shape == () for v in got)
    assert float(got[0]) == pytest.approx(want_mean, rel=1e-12) and float(got[1]) == pytest.approx(want_std, rel=1e-9)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_logits_take_the_definition_on_their_values(dtype):
    x = logits(37, 70, 5, dtype)
    want = O.score(x.double().numpy(), 4)
    got = inception_score(x, splits=4)
    assert got[0].dtype == torch.float32
    assert float(got[0]) == pytest.approx(want[0], rel=2e-6) and float(got[1]) == pytest.approx(want[1], rel=1e-4)


def test_dyadic_rows_are_exact_in_the_aten_form_too():
    x, prob_sum, neg, rows = O.dyadic(41, 65, 4, 3, seed=1)
    got = _inception_score_stats(torch.from_numpy(x), 4, first_split=3)
    assert torch.equal(got[2], torch.from_numpy(rows))
    np.testing.assert_allclose(got[0].numpy(), prob_sum, rtol=1e-6, atol=0)
    np.testing.assert_allclose(got[1].numpy(), neg, rtol=1e-6, atol=1e-6)


def test_first_split_continues_the_partition_across_updates():
    x = logits(37, 70, 107)
    m = metric(70, 4).update_logits(x[:13]).update_logits(x[13:])
    whole = _inception_score_stats(x, 4)
    assert torch.equal(m.num_rows, whole[2]) and m.num_rows.tolist() == [10.0, 9.0, 9.0, 9.0]
    torch.testing.assert_close(m.prob_sum, whole[0], rtol=1e-12, atol=0)
    torch.testing.assert_close(m.neg_entropy_sum, whole[1], rtol=1e-12, atol=0)
    got, want = m.compute(), inception_score(x, splits=4)
    assert float(got[0]) == pytest.approx(float(want[0]), rel=1e-6)
    # the second update alone starts at split 13 mod 4
    second = _inception_score_stats(x[13:].double(), 4, first_split=13)
    check_states(second, O.stats(x[13:].double().numpy(), 4, first=1))


# ----------------------------------------------------------------------------- special values
def test_minus_inf_columns_are_masked_classes():
    x = logits(23, 17, 3)
    x[:, 4] = -INF
    x[5, :16] = -INF  # one class left: p = 1, h = 0
    want = O.stats(x.double().numpy(), 3)
    assert np.isfinite(want[1]).all() and (want[0][:, 4] == 0).all()
    got = _inception_score_stats(x, 3)
    np.testing.assert_allclose(got[0].numpy(), want[0], rtol=1e-6, atol=0)
    np.testing.assert_allclose(got[1].numpy(), want[1], rtol=1e-6, atol=0)
    check_states(_inception_score_stats(x.double(), 3), want)
    assert float(inception_score(x, splits=3)[0]) == pytest.approx(O.score(x.double().numpy(), 3)[0], rel=2e-6)


@pytest.mark.parametrize("bad", ["all -inf", "nan", "+inf"])
def test_a_bad_row_makes_its_split_nan_and_leaves_the_others(bad):
    clean = logits(22, 9, 4)
    x = clean.clone()
    if bad == "all -inf":
        x[6] = -INF
    else:
        x[6, 3] = NAN if bad == "nan" else INF
    want = O.stats(x.double().numpy(), 4)
    assert np.isnan(want[0][2]).all() and np.isnan(want[1][2]) and not np.isnan(want[0][[0, 1, 3]]).any()
    got, ref = _inception_score_stats(x, 4), _inception_score_stats(clean, 4)
    assert bool(got[0][2].isnan().all()) and bool(got[1][2].isnan())
    for s in (0, 1, 3):
        assert torch.equal(got[0][s], ref[0][s]) and torch.equal(got[1][s], ref[1][s])
    assert torch.equal(got[2], ref[2])
    split_log, mean, std = _inception_score_values(*got)
    assert split_log.isnan().tolist() == [False, False, True, False]
    assert bool(mean.isnan()) and bool(std.isnan())
    assert all(bool(v.isnan()) for v in inception_score(x, splits=4))
    assert all(bool(v.isnan()) for v in inception_score(x.double(), splits=4))


def test_fewer_rows_than_splits_one_split_and_no_rows():
    x = logits(3, 9, 5)
    split_log, mean, std = _inception_score_values(*_inception_score_stats(x, 5))
    assert split_log.isnan().tolist() == [False, False, False, True, True]
    want = O.score(x.double().numpy(), 5)
    assert float(mean) == pytest.approx(want[0], rel=1e-6) and not math.isnan(want[0])
    # a split of one row scores exp(0) = 1
    assert float(mean) == pytest.approx(1.0, abs=1e-6) and float(std) == pytest.approx(0.0, abs=1e-6)
    x = logits(40, 9, 6)
    mean, std = inception_score(x, splits=1)
    assert float(mean) == pytest.approx(O.score(x.double().numpy(), 1)[0], rel=1e-6) and float(std) == 0.0
    for dtype in (torch.float32, torch.float64, torch.bfloat16):
        got = inception_score(torch.empty(0, 9, dtype=dtype), splits=3)
        want_dtype = torch.float64 if dtype == torch.float64 else torch.float32
        assert all(v.dtype == want_dtype and v.shape == () and bool(v.isnan()) for v in got)
    assert all(bool(v.isnan()) for v in inception_score(torch.empty(0, 0)))


def test_value_errors():
    x = logits(6, 5, 7)
    for splits in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="splits"):
            inception_score(x, splits=splits)
        with pytest.raises(ValueError, match="splits"):
            metric(5, splits)
    with pytest.raises(ValueError, match="two-dimensional"):
        inception_score(x[0])
    with pytest.raises(ValueError, match="two-dimensional"):
        inception_score(x[None])
    for bad in (torch.ones(4, 5, dtype=torch.int64), torch.ones(4, 5, dtype=torch.bool)):
        with pytest.raises(ValueError, match="floating-point"):
            inception_score(bad)
    with pytest.raises(ValueError, match="at least one column"):
        inception_score(torch.empty(3, 0))
    m = metric(5, 2)
    with pytest.raises(ValueError, match=r"\[B, 5\]"):
        m.update_logits(logits(6, 4, 8))
    with pytest.raises(ValueError, match="two-dimensional"):
        m.update_logits(x[0])
    with pytest.raises(ValueError, match="floating-point"):
        m.update_logits(torch.ones(4, 5, dtype=torch.int64))
    with pytest.raises(ValueError, match="num_classes"):
        InceptionScore(num_classes=10)
    assert float(m.num_rows.sum()) == 0.0


# ----------------------------------------------------------------------------- the class
def test_class_compute_before_update_reset_and_no_rows():
    m = metric(9, 3)
    assert all(v.dtype == torch.float32 and v.shape == () and bool(v.isnan()) for v in m.compute())
    x = logits(11, 9, 9)
    m.update_logits(x[:0])  # a no-op
    assert float(m.num_rows.sum()) == 0.0 and m._rows_seen == 0
    m.update_logits(x[:4])
    assert m.num_rows.tolist() == [2.0, 1.0, 1.0] and m._rows_seen == 1
    m.reset()
    assert float(m.num_rows.sum()) == 0.0 and float(m.prob_sum.abs().sum()) == 0.0 and m._rows_seen == 0
    m.update_logits(x)  # the partition starts at split 0 again
    check_states((m.prob_sum, m.neg_entropy_sum, m.num_rows), O.stats(x.double().numpy(), 3), rtol=1e-6)
    assert m.num_rows.tolist() == [4.0, 4.0, 3.0]
    got = m.compute()
    want = O.score(x.double().numpy(), 3)
    assert float(got[0]) == pytest.approx(want[0], rel=2e-6) and float(got[1]) == pytest.approx(want[1], rel=1e-4)
    assert m._state_merge_kinds() == {"prob_sum": "sum", "neg_entropy_sum": "sum", "num_rows": "sum"}


def test_class_merge_state_dict_pickle_and_to():
    x = logits(30, 9, 10)
    a = metric(9, 4).update_logits(x[:11])
    b = metric(9, 4).update_logits(x[11:])
    before = a._rows_seen
    a.merge_state([b])
    assert a._rows_seen == before == 3 and b.num_rows.tolist() == [5.0, 5.0, 5.0, 4.0]
    # each metric partitions its own rows from split 0: the states are the sums of the two
    w0, w1 = O.stats(x[:11].double().numpy(), 4), O.stats(x[11:].double().numpy(), 4)
    check_states((a.prob_sum, a.neg_entropy_sum, a.num_rows), [p + q for p, q in zip(w0, w1)], rtol=1e-6)
    want = O.values(*[p + q for p, q in zip(w0, w1)])
    assert float(a.compute()[0]) == pytest.approx(want[1], rel=2e-6)
    state = a.state_dict()
    assert set(state) == {"prob_sum", "neg_entropy_sum", "num_rows"}
    c = metric(9, 4).update_logits(x[:2])
    c.load_state_dict(state)
    assert c._rows_seen == 2  # not a state: left as it was
    assert all(torch.equal(p, q) for p, q in zip(c.compute(), a.compute()))
    p = pickle.loads(pickle.dumps(a))
    assert p._rows_seen == a._rows_seen and all(torch.equal(u, v) for u, v in zip(p.compute(), a.compute()))
    assert p.to("cpu") is p and p.device == torch.device("cpu") and p.prob_sum.device.type == "cpu"


class Head(torch.nn.Module):
    """A stand-in classifier: [B, 3, 2, 2] images to [B, 12] logits."""

    def __init__(self):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.tensor(6.0), requires_grad=False)

    def forward(self, images):
        return (images.flatten(1) - 0.5) * self.scale


def test_class_update_runs_the_model_checks_images_and_moves_the_model():
    images = torch.rand(14, 3, 2, 2, generator=torch.Generator().manual_seed(11))
    m = InceptionScore(model=Head(), num_classes=12, splits=3)
    m.update(images[:5]).update(images[5:])
    want = O.score(Head()(images).double().numpy(), 3)
    got = m.compute()
    assert float(got[0]) == pytest.approx(want[0], rel=2e-6) and float(got[1]) == pytest.approx(want[1], rel=1e-4)
    with pytest.raises(ValueError, match="4D"):
        m.update(images[0])
    with pytest.raises(ValueError, match="3 channels"):
        m.update(images[:, :2])
    m.to("meta")
    assert m.model.scale.device.type == "meta" and m.prob_sum.device.type == "meta"


class TestInceptionScore(MetricClassTester):
    def test_class_suite(self) -> None:
        """Eight updates of five images into four splits.  One metric continues its partition
        over the updates; four metrics of two updates each start theirs at split 0, so the merged
        and the synced result is the value of the summed states, computed here from the oracle."""
        images = torch.rand(8, 5, 3, 2, 2, generator=torch.Generator().manual_seed(12))
        x = Head()(images.flatten(0, 1)).double().numpy()
        one = O.score(x, 4)
        parts = [O.stats(x[10 * r:10 * r + 10], 4) for r in range(4)]
        merged = O.values(*[sum(p[k] for p in parts) for k in range(3)])[1:]
        assert abs(one[0] - merged[0]) > 1e-4  # the two partitions differ
        self.run_class_implementation_tests(
            metric=InceptionScore(model=Head(), num_classes=12, splits=4),
            state_names={"prob_sum", "neg_entropy_sum", "num_rows"},
            update_kwargs={"images": images},
            compute_result=tuple(torch.tensor(v, dtype=torch.float32) for v in one),
            merge_and_compute_result=tuple(torch.tensor(v, dtype=torch.float32) for v in merged),
            test_merge_with_one_update=True,
            atol=1e-5,
            rtol=1e-5,
        )


def _sync_job(rank: int, ws: int):
    from torcheval_amd.metrics.toolkit import sync_and_compute

    x = logits(30, 9, 13)
    m = metric(9, 4)
    if rank == 0:
        m.update_logits(x)  # rank 1 never updates
    return sync_and_compute(m)


def test_two_rank_sync_and_compute_with_an_idle_rank():
    want = O.score(logits(30, 9, 13).double().numpy(), 4)
    results = run_distributed(_sync_job, 2)
    assert results[0] is not None  # rank 0 is the recipient
    for got in results:
        if got is not None:
            assert float(got[0]) == pytest.approx(want[0], rel=2e-6) and float(got[1]) == pytest.approx(want[1], rel=1e-4)


# ----------------------------------------------------------------------------- the model
def test_inception_v3_logits_model():
    from torcheval_amd.models.inception import FIDInceptionV3, InceptionV3Logits

    torch.manual_seed(0)
    with pytest.warns(RuntimeWarning, match="InceptionV3Logits is randomly initialised"):
        model = InceptionV3Logits().eval()
    assert isinstance(model.model.fc, torch.nn.Linear) and model.model.fc.out_features == 1000
    with torch.inference_mode():
        out = model(torch.rand(2, 3, 32, 32))
    assert out.shape == (2, 1000) and out.dtype == torch.float32
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        InceptionV3Logits(weights=None)
    with pytest.warns(RuntimeWarning, match="FIDInceptionV3 is randomly initialised"):
        fid = FIDInceptionV3()
    assert isinstance(fid.model.fc, torch.nn.Identity)  # untouched


def test_default_model_checks_images_as_fid_does():
    with pytest.warns(RuntimeWarning):
        m = InceptionScore(splits=2)
    assert m.prob_sum.shape == (2, 1000)
    with pytest.raises(ValueError, match="float32"):
        m.update(torch.zeros(2, 3, 8, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        m.update(torch.full((2, 3, 8, 8), 2.0))


# ----------------------------------------------------------------------------- exports, routing
def test_exports():
    for mod in (M, MI):
        assert mod.InceptionScore is InceptionScore
        assert "InceptionScore" not in mod.__all__
    for mod in (MF, MFI):
        assert mod.inception_score is inception_score
        assert "inception_score" not in mod.__all__
    assert MI.__doc_extras__ == ["InceptionScore"] and MFI.__doc_extras__ == ["inception_score"]


def test_wrapper_constants_match_the_header():
    from torcheval_amd.ops import inception_score as K

    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    with open(os.path.join(root, "csrc", "include", "tea_kernels.h")) as fh:
        header = fh.read()

    def const(name: str) -> int:
        return int(re.search(rf"constexpr int {name} = (\d+);", header).group(1))

    assert K.max_columns() == K.MAX_COLUMNS == const("kInceptionMaxColumns") == 2048
    assert K.max_splits() == K.MAX_SPLITS == const("kInceptionMaxSplits") == 64
    assert K.MAX_BLOCKS == const("kInceptionMaxBlocks")
    assert K.WAVES_PER_BLOCK == const("kInceptionWavesPerBlock")
    assert K.NARROW_COLUMNS == const("kInceptionNarrowColumns")
    assert K.ROWS_PER_WAVE_NARROW == const("kInceptionRowsPerWaveNarrow")
    assert K.ROWS_PER_WAVE_WIDE == const("kInceptionRowsPerWaveWide")
    # the grid rule: blocks per split
    assert K.blocks_per_split(1, 10, 1000) == 1 and K.blocks_per_split(50000, 10, 1000) == 102
    assert K.blocks_per_split(8192, 10, 1000) == 26 and K.blocks_per_split(8192, 10, 256) == 7
    assert K.blocks_per_split(10**6, 64, 8) == 16 and K.blocks_per_split(10**6, 1, 8) == 1024
    # CPU tensors are not the kernel's
    s = _inception_score_stats(logits(4, 5, 1), 2)
    assert not K.supported(logits(4, 5, 1), *s) and not K.value_supported(*s)


@pytest.mark.skipif(not ops.native_loaded(), reason="extension not built")
def test_native_op_surface_and_meta_route():
    """K21's two ops: their schemas, which dispatch keys hold a kernel, Meta kernels that return
    None, and the wrapper on meta tensors."""
    from torcheval_amd.ops import inception_score as K

    ns = "torcheval_amd_inception::"
    names = sorted(n for n in torch._C._dispatch_get_all_op_names() if n.startswith(ns))
    assert names == [ns + "inception_update", ns + "inception_value"]
    lib = torch.ops.torcheval_amd_inception
    assert str(lib.inception_update.default._schema) == (
        ns + "inception_update(Tensor logits, int first_split, Tensor(a!) prob_sum, Tensor(b!) neg_entropy_sum, "
        "Tensor(c!) num_rows) -> ()")
    assert str(lib.inception_value.default._schema) == (
        ns + "inception_value(Tensor prob_sum, Tensor neg_entropy_sum, Tensor num_rows, Tensor(a!) split_log, "
        "Tensor(b!) out) -> ()")
    for name in names:
        has = [k for k in ("CPU", "CUDA", "Meta") if torch._C._dispatch_has_kernel_for_dispatch_key(name, k)]
        assert has == ["CUDA", "Meta"]
    meta = torch.device("meta")
    x = torch.empty(7, 9, device=meta)
    states = [torch.empty(s, dtype=torch.float64, device=meta) for s in ((3, 9), (3,), (3,))]
    assert K.inception_update(x, 2, *states) is None
    split_log, out = K.inception_value(*states)
    assert split_log.shape == (3,) and split_log.dtype == torch.float64 and split_log.device.type == "meta"
    assert out.shape == (2,) and out.dtype == torch.float32
