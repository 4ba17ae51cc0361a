"""Improved precision / recall and density / coverage (not in the reference tree; definition in
docs/parity.md).

The oracle is an independent numpy evaluation written here: the full FP64 distance matrix, a
diagonal set to ``inf``, ``np.sort``.  CPU tensors run the ATen form; tests/gpu/test_k22_prdc.py
runs the same oracle against K22.
"""

import os
import pickle
import re

import numpy as np
import pytest
import torch

import torcheval_amd.ops as ops
from torcheval_amd.metrics import DensityCoverage, ImprovedPrecisionRecall
from torcheval_amd.metrics.functional import density_coverage, improved_precision_recall
from torcheval_amd.metrics.functional.image import prdc as P
from torcheval_amd.metrics.functional.image.prdc import _prdc


def oracle(real, fake, k):
    x, y = real.double().numpy(), fake.double().numpy()
    nx, ny = (x * x).sum(1), (y * y).sum(1)

    def d2(a, na, b, nb):
        return np.maximum(0.0, (na[:, None] + nb[None, :]) - 2.0 * (a @ b.T))

    def radii(a, na):
        d = d2(a, na, a, na)
        np.fill_diagonal(d, np.inf)
        return np.sort(d, axis=1)[:, k - 1]

    rr, rf = radii(x, nx), radii(y, ny)
    dfx, dxf = d2(y, ny, x, nx), d2(x, nx, y, ny)
    out = {
        "radii_real": rr, "radii_fake": rf,
        "hits_fake": (dfx <= rr[None, :]).sum(1), "hits_real": (dxf <= rf[None, :]).sum(1),
        "nearest_fake": dfx.min(1), "nearest_real": dxf.min(1),
    }
    out["tallies"] = np.array([(out["hits_fake"] > 0).sum(), (out["hits_real"] > 0).sum(), out["hits_fake"].sum(),
                               (out["nearest_real"] <= rr).sum()], dtype=np.int64)
    n, m = x.shape[0], y.shape[0]
    out["values"] = (out["tallies"] / np.array([m, n, k * m, n], dtype=np.float64)).astype(np.float32)
    return out


def check(got, want, exact):
    for name in ("radii_real", "radii_fake", "nearest_real", "nearest_fake"):
        assert got[name].dtype == torch.float64
        if exact:
            assert np.array_equal(got[name].numpy(), want[name]), name
        else:
            np.testing.assert_allclose(got[name].numpy(), want[name], rtol=1e-12, atol=0.0, err_msg=name)
    for name in ("hits_real", "hits_fake"):
        assert got[name].dtype == torch.int32
        assert np.array_equal(got[name].numpy(), want[name]), name
    assert got["tallies"].dtype == torch.int64 and np.array_equal(got["tallies"].numpy(), want["tallies"])
    assert got["values"].dtype == torch.float32 and np.array_equal(got["values"].numpy(), want["values"])


def integer_features(n_r, n_f, d, seed):
    """Integers in [0, 4).  Row i of the real side is non-zero only in its first 1 + i d // n_r
    columns and row j of the generated side in its first 1 + d // 4 + 3 j d // (4 n_f), so norms
    grow with the row number, the rows are not exchangeable and the two sets overlap in part."""
    g = torch.Generator().manual_seed(seed)
    cols = torch.arange(d)[None, :]
    real = torch.randint(0, 4, (n_r, d), generator=g).float()
    real = real * (cols <= (torch.arange(n_r)[:, None] * d) // n_r)
    fake = torch.randint(0, 4, (n_f, d), generator=g).float()
    fake = fake * (cols <= d // 4 + (3 * torch.arange(n_f)[:, None] * d) // (4 * n_f))
    return real, fake


def features(n_r, n_f, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n_r, d, generator=g), 0.9 * torch.rand(n_f, d, generator=g) + 0.05


# ----------------------------------------------------------------------------- the ATen form
@pytest.mark.parametrize("k", [1, 3, 5, 9])
@pytest.mark.parametrize("n,m,d", [(40, 31, 16), (33, 50, 4), (130, 129, 64)])
def test_aten_form_on_integer_data_is_exact(n, m, d, k):
    real, fake = integer_features(n, m, d, n + d + k)
    check(_prdc(real, fake, k), oracle(real, fake, k), exact=True)


def test_integer_data_is_not_degenerate():
    """The shape the GPU tests lean on: all four values strictly between the trivial ends."""
    for seed in (5, 6):
        real, fake = integer_features(130, 129, 64, seed)
        for k in (3, 5):
            values = oracle(real, fake, k)["values"]
            assert np.all(values > 0.6) and np.all(values < 1.2), values


@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("n,m,d", [(60, 45, 24), (45, 60, 7)])
def test_aten_form_on_random_float32_data(n, m, d, k):
    real, fake = features(n, m, d, n + k)
    check(_prdc(real, fake, k), oracle(real, fake, k), exact=False)
    check(_prdc(real.double(), fake.half().double(), k), oracle(real, fake.half().float(), k), exact=False)


@pytest.mark.parametrize("nbytes", [8, 8 * 45 * 7, 8 * 60 * 16 + 8, 1 << 28])
def test_chunk_edges_inside_the_data(monkeypatch, nbytes):
    """A bound of 8 bytes is one query row per chunk; the next two put a handful of rows in one, so
    chunk edges fall inside either set; the last is one chunk."""
    real, fake = integer_features(60, 45, 12, 3)
    want = oracle(real, fake, 3)
    monkeypatch.setattr(P, "_ATEN_CHUNK_BYTES", nbytes)
    check(_prdc(real, fake, 3), want, exact=True)
    real, fake = features(60, 45, 12, 4)
    one = _prdc(real, fake, 3)
    monkeypatch.setattr(P, "_ATEN_CHUNK_BYTES", 1 << 28)
    whole = _prdc(real, fake, 3)
    for name in ("hits_real", "hits_fake", "tallies", "values"):
        assert torch.equal(one[name], whole[name])
    check(one, oracle(real, fake, 3), exact=False)


# ----------------------------------------------------------------------------- hand-made cases
def test_identical_sets_score_one():
    real, _ = features(30, 30, 8, 1)
    for k in (1, 3):
        p, r = improved_precision_recall(real, real.clone(), k=k)
        d, c = density_coverage(real, real.clone(), k=k)
        assert float(p) == 1.0 and float(r) == 1.0 and float(c) == 1.0
        assert p.dtype == torch.float32 and p.shape == () and d.dtype == torch.float32
        # y_j lies in its own ball and in those of the rows that count it among their k nearest
        want = oracle(real, real, k)
        assert float(d) == want["values"][2] and float(d) >= 1.0 / k


def test_far_shifted_fake_scores_zero():
    real, fake = features(30, 25, 8, 2)
    fake = fake + 100.0
    assert [float(v) for v in improved_precision_recall(real, fake)] == [0.0, 0.0]
    assert [float(v) for v in density_coverage(real, fake)] == [0.0, 0.0]
    assert _prdc(real, fake, 3)["tallies"].tolist() == [0, 0, 0, 0]


def test_duplicate_row_has_radius_zero_and_still_holds_its_duplicate():
    real = torch.tensor([[0.0, 0.0], [0.0, 0.0], [5.0, 0.0], [9.0, 0.0]])
    fake = torch.tensor([[0.0, 0.0], [7.0, 0.0], [20.0, 0.0]])
    out = _prdc(real, fake, 1)
    assert out["radii_real"].tolist() == [0.0, 0.0, 16.0, 16.0]  # positional: the duplicate counts
    assert out["radii_fake"].tolist() == [49.0, 49.0, 169.0]
    # fake row 0 sits on the duplicates: inside both balls of radius 0 (<=); fake row 1 is at
    # distance 4 from rows 2 and 3
    assert out["hits_fake"].tolist() == [2, 2, 0]
    assert out["nearest_fake"].tolist() == [0.0, 4.0, 121.0]
    assert out["hits_real"].tolist() == [2, 2, 2, 2]
    assert out["tallies"].tolist() == [2, 4, 4, 4]
    check(out, oracle(real, fake, 1), exact=True)


def test_k_equal_to_rows_minus_one():
    real, fake = integer_features(9, 7, 6, 8)
    check(_prdc(real, fake, 6), oracle(real, fake, 6), exact=True)
    out = _prdc(real, fake, 6)
    d = torch.cdist(fake.double(), fake.double()) ** 2
    assert torch.allclose(out["radii_fake"], d.max(dim=1).values)  # the farthest other row
    with pytest.raises(ValueError, match="k \\+ 1 rows"):
        _ = improved_precision_recall(real, fake, k=7)


def test_value_errors():
    real, fake = features(10, 12, 4, 9)
    for fn in (improved_precision_recall, density_coverage):
        for bad in (0, -1, 2.0, True, None):
            with pytest.raises(ValueError, match="`k`"):
                fn(real, fake, k=bad)
        with pytest.raises(ValueError, match="k \\+ 1 rows"):
            fn(real, fake, k=10)
        with pytest.raises(ValueError, match="k \\+ 1 rows"):
            fn(real[:3], fake, k=3)
        with pytest.raises(ValueError, match="two-dimensional"):
            fn(real[0], fake)
        with pytest.raises(ValueError, match="two-dimensional"):
            fn(real, fake[None])
        with pytest.raises(ValueError, match="two-dimensional"):
            fn(real, fake[:, :3])
        with pytest.raises(ValueError, match="two-dimensional"):
            fn(real[:, :0], fake[:, :0])
    for cls in (ImprovedPrecisionRecall, DensityCoverage):
        with pytest.raises(ValueError, match="`k`"):
            cls(model=torch.nn.Identity(), feature_dim=4, k=0)


# ----------------------------------------------------------------------------- the classes
CASES = [(ImprovedPrecisionRecall, improved_precision_recall, 3), (DensityCoverage, density_coverage, 5)]


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("cls,fn,k", CASES)
def test_class_in_pieces_equals_the_functional(cls, fn, k):
    real, fake = features(40, 30, 16, 12)
    m = cls(model=torch.nn.Identity(), feature_dim=16)
    assert m.k == k
    with pytest.raises(ValueError, match="k \\+ 1 rows"):
        m.compute()
    for lo, hi in ((0, 1), (1, 17), (17, 40)):
        m.update_activations(real[lo:hi], True)
    m.update_activations(fake[:2], False)
    with pytest.raises(ValueError, match="k \\+ 1 rows"):
        m.compute()
    m.update_activations(fake[2:], False)
    got = m.compute()
    assert same(got, fn(real, fake)) and same(m.compute(), got)
    assert same(cls(model=torch.nn.Identity(), feature_dim=16, k=2).update_activations(real, True)
                .update_activations(fake, False).compute(), fn(real, fake, k=2))
    with pytest.raises(ValueError, match="bool"):
        m.update_activations(real, 1)
    with pytest.raises(ValueError, match="activations"):
        m.update_activations(real[:, :8], True)
    m.reset()
    assert m.real_features == [] and m.fake_features == []


def test_class_update_runs_the_model_and_checks_images():
    class Pool(torch.nn.Module):
        def forward(self, images):
            return images.flatten(2).mean(-1).repeat(1, 2)  # [B, 6]

    images = torch.rand(14, 3, 5, 5, generator=torch.Generator().manual_seed(14))
    m = DensityCoverage(model=Pool(), feature_dim=6, k=2)
    m.update(images[:8], True).update(images[8:], False)
    assert same(m.compute(), density_coverage(Pool()(images[:8]), Pool()(images[8:]), k=2))
    with pytest.raises(ValueError, match="4D"):
        m.update(images[0], True)
    with pytest.raises(ValueError, match="bool"):
        m.update(images, 1)


@pytest.mark.parametrize("cls,fn,k", CASES)
def test_class_merge_state_equals_one_metric_fed_everything(cls, fn, k):
    real, fake = features(40, 30, 16, 15)

    def new():
        return cls(model=torch.nn.Identity(), feature_dim=16)

    a = new().update_activations(real[:10], True).update_activations(fake[:5], False)
    b = new().update_activations(real[10:25], True).update_activations(real[25:], True)
    c = new().update_activations(fake[5:], False)
    a.merge_state([b, c])
    assert same(a.compute(), fn(real, fake))
    assert a._state_merge_kinds() == {"real_features": "cat", "fake_features": "cat"}
    b._prepare_for_merge_state()
    assert len(b.real_features) == 1 and b.real_features[0].shape == (30, 16) and b.fake_features == []


@pytest.mark.parametrize("cls,fn,k", CASES)
def test_class_state_dict_and_pickle_round_trips(cls, fn, k):
    real, fake = features(40, 30, 16, 16)
    m = cls(model=torch.nn.Identity(), feature_dim=16)
    m.update_activations(real[:20], True).update_activations(real[20:], True).update_activations(fake, False)
    want = m.compute()
    state = m.state_dict()
    assert sorted(state) == ["fake_features", "real_features"] and len(state["real_features"]) == 2
    n = cls(model=torch.nn.Identity(), feature_dim=16)
    n.load_state_dict(state)
    assert same(n.compute(), want)
    p = pickle.loads(pickle.dumps(m))
    assert same(p.compute(), want)
    assert p.to("cpu") is p and p.device == torch.device("cpu")


def test_classes_share_one_base():
    base = ImprovedPrecisionRecall.__mro__[1]
    assert base is DensityCoverage.__mro__[1] and base.__name__ == "_NeighbourMetric"
    assert "update_activations" not in vars(ImprovedPrecisionRecall) and "compute" not in vars(DensityCoverage)


def test_exports():
    import torcheval_amd.metrics as M
    import torcheval_amd.metrics.functional as MF
    import torcheval_amd.metrics.functional.image as MFI
    import torcheval_amd.metrics.image as MI

    assert MI.ImprovedPrecisionRecall is ImprovedPrecisionRecall is M.ImprovedPrecisionRecall
    assert MI.DensityCoverage is DensityCoverage is M.DensityCoverage
    assert MFI.improved_precision_recall is improved_precision_recall is MF.improved_precision_recall
    assert MFI.density_coverage is density_coverage is MF.density_coverage
    assert "ImprovedPrecisionRecall" in MI.__all__ and "DensityCoverage" in MI.__all__
    assert "improved_precision_recall" in MFI.__all__ and "density_coverage" in MFI.__all__
    # not reference names: importable from the package roots, outside their __all__
    for name in ("ImprovedPrecisionRecall", "DensityCoverage"):
        assert name not in M.__all__
    for name in ("improved_precision_recall", "density_coverage"):
        assert name not in MF.__all__


# ----------------------------------------------------------------------------- the native surface
def test_constants_match_the_header():
    from torcheval_amd.ops import prdc as K

    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    with open(os.path.join(root, "csrc", "include", "tea_kernels.h")) as fh:
        header = fh.read()
    for name, value in (("kPrdcTile", K.TILE), ("kPrdcMaxK", K.MAX_K), ("kPrdcCUs", K.CUS),
                        ("kPrdcMaxGroups", K.MAX_GROUPS), ("kPrdcBlockStages", K.BLOCK_STAGES),
                        ("kPrdcHitsRows", K.HITS_ROWS)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, header).group(1)) == value
    t = K.TILE
    # the rule (prdc_groups): small sets take a block per tile; 79 panels fill the CUs' two slots
    # once at narrow rows (474 blocks) and five times at wide ones, where a block's fixed cost is small
    sizes = (2, t, t + 1, 2 * t + 1, 10000, 50000, 100000)
    assert [K.groups_for(n, n, 64) for n in sizes] == [1, 1, 2, 3, 6, 5, 7]
    assert [K.groups_for(n, n, 2048) for n in sizes] == [1, 1, 2, 3, 16, 11, 16]
    assert K.groups_for(2 * t + 1, 2 * t + 1, 64, 2) == 2 and K.groups_for(2 * t + 1, t, 64, 7) == 1
    assert K.groups_for(2 * t + 1, 10000, 64, 100) == 79
    assert K.hits_blocks(1, 1) == 2 and K.hits_blocks(256, 257) == 3


def test_native_op_surface_and_meta_route():
    """K22's five ops: their schemas, which dispatch keys hold a kernel, Meta kernels that return
    None, and the wrapper on meta tensors."""
    from torcheval_amd.ops import prdc as K

    assert ops.native_loaded()
    names = sorted(n for n in torch._C._dispatch_get_all_op_names() if n.startswith("torcheval_amd_prdc::"))
    assert names == ["torcheval_amd_prdc::prdc_" + s for s in ("cross", "finish", "knn", "norms", "radii")]
    ns = torch.ops.torcheval_amd_prdc
    assert str(ns.prdc_norms.default._schema) == (
        "torcheval_amd_prdc::prdc_norms(Tensor real, Tensor fake, Tensor(a!) norms_real, Tensor(b!) norms_fake) "
        "-> ()")
    assert str(ns.prdc_knn.default._schema) == (
        "torcheval_amd_prdc::prdc_knn(Tensor feats, Tensor norms, int k, int groups, Tensor(a!) partial) -> ()")
    assert str(ns.prdc_radii.default._schema) == (
        "torcheval_amd_prdc::prdc_radii(Tensor partial, Tensor(a!) radii) -> ()")
    assert str(ns.prdc_cross.default._schema) == (
        "torcheval_amd_prdc::prdc_cross(Tensor query, Tensor ref, Tensor norms_q, Tensor norms_ref, "
        "Tensor radii_ref, int groups, Tensor(a!) counts, Tensor(b!) mins) -> ()")
    assert str(ns.prdc_finish.default._schema) == (
        "torcheval_amd_prdc::prdc_finish(Tensor counts_fake, Tensor mins_fake, Tensor counts_real, "
        "Tensor mins_real, Tensor radii_real, int k, Tensor(a!) block_tallies, Tensor(b!) hits_real, "
        "Tensor(c!) hits_fake, Tensor(d!) nearest_real, Tensor(e!) nearest_fake, Tensor(f!) tallies, "
        "Tensor(g!) values) -> ()")
    for name in names:
        has = [k for k in ("CPU", "CUDA", "Meta") if torch._C._dispatch_has_kernel_for_dispatch_key(name, k)]
        assert has == ["CUDA", "Meta"]
    meta = torch.device("meta")
    real = torch.empty(300, 64, device=meta)
    fake = torch.empty(200, 64, dtype=torch.float16, device=meta)
    norms = torch.empty(300, dtype=torch.float64, device=meta)
    assert ns.prdc_norms.default(real, real, norms, norms) is None
    out = K.prdc(real, fake, 3, groups=2)
    assert out["radii_real"].shape == (300,) and out["radii_fake"].dtype == torch.float64
    assert out["hits_fake"].shape == (200,) and out["hits_real"].dtype == torch.int32
    assert out["nearest_real"].shape == (300,) and out["nearest_fake"].shape == (200,)
    assert out["tallies"].shape == (4,) and out["tallies"].dtype == torch.int64
    assert out["values"].shape == (4,) and out["values"].dtype == torch.float32 and out["values"].device.type == "meta"
    # CPU tensors and k > 8 are not the kernel's: the functional takes the ATen form
    assert not K.supported(torch.rand(9, 4), torch.rand(9, 4), 3)


def test_wrapper_traces_into_one_graph():
    """The wrapper's Python (the group rule's loop, the buffer shapes, the widening copy) holds
    nothing that breaks a ``fullgraph=True`` trace; tests/gpu/test_k22_prdc.py runs the graph."""
    from torcheval_amd.ops import prdc as K

    torch._dynamo.reset()
    fn = torch.compile(lambda r, f: K.prdc(r, f, 3), fullgraph=True, backend="eager")
    meta = torch.device("meta")
    out = fn(torch.empty(300, 64, device=meta), torch.empty(200, 64, dtype=torch.bfloat16, device=meta))
    assert out["radii_real"].shape == (300,) and out["hits_fake"].shape == (200,) and out["values"].shape == (4,)
