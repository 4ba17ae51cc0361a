"""Silhouette coefficient (not in the reference tree; definition in docs/parity.md).

CPU tensors run the ATen form, which is held to ``sklearn.metrics.silhouette_samples`` /
``silhouette_score`` on float64 copies of the data; where sklearn raises or rejects the input (one
cluster, NaN features) a plain numpy oracle written here stands in.  tests/gpu/test_k23_silhouette.py
runs the same kind of oracle against K23.
"""

import math
import os
import pickle
import re

import numpy as np
import pytest
import torch
from sklearn.metrics import silhouette_samples as sk_samples
from sklearn.metrics import silhouette_score as sk_score

import torcheval_amd.ops as ops
from torcheval_amd.metrics import SilhouetteScore
from torcheval_amd.metrics.functional import silhouette_samples, silhouette_score
from torcheval_amd.metrics.functional.clustering import silhouette as S
from torcheval_amd.metrics.functional.clustering.silhouette import _silhouette
from torcheval_amd.utils.test_utils import MetricClassTester
from torcheval_amd.utils.test_utils.dist_pool import run_distributed


def oracle(x, labels, k):
    """a, b, s [N] and the score by the definition: direct differences, a loop over samples and
    clusters, ``math.fsum``; a non-finite row is at distance NaN from every other row and a NaN mean
    is no candidate for b."""
    x = x.double().numpy()
    lab = labels.numpy().astype(np.int64)
    n = len(x)
    members = [np.flatnonzero(lab == c) for c in range(k)]
    counts = np.array([len(m) for m in members])
    poisoned = ~np.isfinite(x).all(axis=1)
    a, b, s = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    for i in range(n):
        with np.errstate(invalid="ignore"):
            d = np.sqrt(((x - x[i]) ** 2).sum(axis=1))
        d[poisoned | poisoned[i]] = np.nan
        d[i] = 0.0
        best = math.nan
        for c in range(k):
            if counts[c] == 0:
                continue
            total = math.fsum(d[members[c]])
            if c == lab[i]:
                a[i] = total / (counts[c] - 1) if counts[c] > 1 else 0.0
            elif not math.isnan(total) and (math.isnan(best) or total / counts[c] < best):
                best = total / counts[c]
        b[i] = best
        top = max(a[i], b[i])
        if math.isnan(a[i]) or math.isnan(b[i]):
            s[i] = math.nan
        else:
            s[i] = 0.0 if counts[lab[i]] == 1 or top == 0.0 else (b[i] - a[i]) / top
    score = math.fsum(s) / n if (counts > 0).sum() >= 2 else math.nan
    return {"a": a, "b": b, "s": s, "score": score}


def data(n, d, k, seed, integer=False):
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, k, (n,), generator=g)
    if integer:
        return torch.randint(-8, 9, (n, d), generator=g).float(), labels
    return torch.rand(k, d, generator=g)[labels] + 0.4 * torch.rand(n, d, generator=g), labels


# ----------------------------------------------------------------------------- the ATen form
@pytest.mark.parametrize("n,d,k,integer", [(300, 5, 6, True), (150, 16, 4, False), (97, 3, 9, False)])
def test_aten_form_against_sklearn(n, d, k, integer):
    x, labels = data(n, d, k, n + d, integer)
    labels[0] = k  # a singleton cluster; ids without members lie below and above it
    want = sk_samples(x.double().numpy(), labels.numpy())
    for dtype in (torch.float32, torch.float64):
        got = silhouette_samples(x.to(dtype), labels, num_clusters=k + 3)
        assert got.dtype == dtype and got.shape == (n,)
        np.testing.assert_allclose(got.double().numpy(), want, rtol=0, atol=1e-12 if dtype == torch.float64 else 1e-6)
        score = silhouette_score(x.to(dtype), labels, num_clusters=k + 3)
        assert score.dtype == dtype and score.shape == ()
    assert abs(float(silhouette_score(x.double(), labels)) - sk_score(x.double().numpy(), labels.numpy())) <= 1e-12
    out = _silhouette(x, labels, k + 3)
    want = oracle(x, labels, k + 3)
    for name in ("a", "b", "s"):
        assert out[name].dtype == torch.float64
        np.testing.assert_allclose(out[name].numpy(), want[name], rtol=0, atol=1e-12, err_msg=name)
    assert abs(float(out["score64"]) - want["score"]) <= 1e-12 and out["score"].dtype == torch.float32


def test_numpy_oracle_agrees_with_sklearn():
    x, labels = data(300, 5, 6, 1, integer=True)
    labels[0] = 6
    assert np.abs(oracle(x, labels, 7)["s"] - sk_samples(x.double().numpy(), labels.numpy())).max() <= 1e-14


@pytest.mark.parametrize("nbytes", [8, 8 * 97 * 5, 1 << 28])
def test_chunk_edges_inside_the_data(monkeypatch, nbytes):
    x, labels = data(97, 3, 5, 2)
    want = sk_samples(x.double().numpy(), labels.numpy())
    monkeypatch.setattr(S, "_ATEN_CHUNK_BYTES", nbytes)
    np.testing.assert_allclose(silhouette_samples(x.double(), labels).numpy(), want, rtol=0, atol=1e-12)


# ----------------------------------------------------------------------------- edge semantics
def test_one_cluster_and_one_sample_are_nan():
    x, _ = data(20, 4, 2, 3)
    labels = torch.full((20,), 2)
    assert math.isnan(float(silhouette_score(x, labels))) and math.isnan(float(silhouette_score(x, labels, num_clusters=5)))
    assert torch.isnan(silhouette_samples(x, labels)).all()
    assert math.isnan(float(silhouette_score(x[:1], labels[:1])))
    assert math.isnan(float(silhouette_score(x[:0], labels[:0]))) and silhouette_samples(x[:0], labels[:0]).shape == (0,)


def test_all_singletons_score_zero():
    x, _ = data(12, 4, 2, 4)
    assert float(silhouette_score(x, torch.arange(12))) == 0.0
    assert silhouette_samples(x, torch.arange(12), num_clusters=20).tolist() == [0.0] * 12


def test_identical_points_give_zero_not_nan():
    x = torch.ones(10, 3)
    labels = torch.tensor([0] * 6 + [1] * 4)
    assert silhouette_samples(x, labels).tolist() == [0.0] * 10  # a = b = 0
    x[6:] += 3.0
    assert silhouette_samples(x, labels).tolist() == [1.0] * 10 and float(silhouette_score(x, labels)) == 1.0


def test_empty_ids_num_clusters_none_and_int32_labels():
    x, labels = data(60, 6, 4, 5)
    labels = labels * 3 + 1  # ids 1, 4, 7, 10 of 12
    want = silhouette_samples(x, labels, num_clusters=12)
    np.testing.assert_allclose(want.double().numpy(), sk_samples(x.double().numpy(), labels.numpy()), rtol=0, atol=1e-6)
    assert torch.equal(silhouette_samples(x, labels), want)  # labels.max() + 1 = 11
    assert torch.equal(silhouette_samples(x, labels.int(), num_clusters=40), want)
    assert torch.equal(silhouette_score(x, labels.int()), silhouette_score(x, labels, num_clusters=12))


def test_bad_labels_raise_on_cpu():
    x, labels = data(30, 4, 3, 6)
    with pytest.raises(ValueError, match="outside \\[0, num_clusters\\)"):
        silhouette_score(x, labels, num_clusters=2)
    labels[4] = -1
    with pytest.raises(ValueError, match="outside \\[0, num_clusters\\)"):
        silhouette_samples(x, labels)


def test_nan_and_inf_features():
    x, labels = data(40, 4, 2, 7)
    labels[-1] = 2  # the poisoned row alone in a third cluster
    for value in (math.nan, math.inf, -math.inf):
        y = x.clone()
        y[-1, 1] = value
        samples = silhouette_samples(y, labels)
        assert torch.isnan(samples).nonzero().flatten().tolist() == [39] and math.isnan(float(silhouette_score(y, labels)))
        want = oracle(y, labels, 3)
        np.testing.assert_allclose(samples.double().numpy(), want["s"], rtol=0, atol=1e-6, equal_nan=True)
        # inside a cluster: NaN for its members, finite for the others
        y = x.clone()
        y[0, 0] = value
        samples = silhouette_samples(y, labels)
        assert torch.equal(torch.isnan(samples), labels == labels[0])
        np.testing.assert_allclose(samples.double().numpy(), oracle(y, labels, 3)["s"], rtol=0, atol=1e-6, equal_nan=True)


def test_value_errors():
    x, labels = data(10, 4, 2, 8)
    for fn in (silhouette_score, silhouette_samples):
        for bad in (0, -1, 2.0, True):
            with pytest.raises(ValueError, match="`num_clusters`"):
                fn(x, labels, num_clusters=bad)
        with pytest.raises(ValueError, match="floating \\[N, D\\]"):
            fn(x[0], labels)
        with pytest.raises(ValueError, match="floating \\[N, D\\]"):
            fn(x.long(), labels)
        with pytest.raises(ValueError, match="floating \\[N, D\\]"):
            fn(x[:, :0], labels)
        with pytest.raises(ValueError, match="int64 or int32"):
            fn(x, labels.float())
        with pytest.raises(ValueError, match="labels should be \\[N\\]"):
            fn(x, labels[:9])
    with pytest.raises(ValueError, match="`num_clusters`"):
        SilhouetteScore(num_clusters=0)


# ----------------------------------------------------------------------------- the class
class TestSilhouetteScore(MetricClassTester):
    def test_class_suite(self) -> None:
        x, labels = data(8 * 12, 5, 3, 9)
        want = torch.tensor(sk_score(x.double().numpy(), labels.numpy()), dtype=torch.float32)
        self.run_class_implementation_tests(
            metric=SilhouetteScore(num_clusters=3),
            state_names={"features", "labels"},
            update_kwargs={"input": x.reshape(8, 12, 5), "labels": labels.reshape(8, 12)},
            compute_result=want,
            min_updates_before_compute=1,
            atol=1e-6,
            rtol=1e-5,
        )


def test_class_in_pieces_merge_state_dict_and_pickle():
    x, labels = data(50, 6, 3, 10)
    want = silhouette_score(x, labels)
    m = SilhouetteScore()
    assert math.isnan(float(m.compute()))
    m.update(x[:1], labels[:1]).update(x[1:20], labels[1:20].int()).update(x[20:], labels[20:])
    assert torch.equal(m.compute(), want) and torch.equal(m.compute(), want)
    assert m._state_merge_kinds() == {"features": "cat", "labels": "cat"}
    a = SilhouetteScore(num_clusters=3).update(x[:10], labels[:10])
    b = SilhouetteScore(num_clusters=3).update(x[10:30], labels[10:30]).update(x[30:], labels[30:])
    assert torch.equal(a.merge_state([b, SilhouetteScore(num_clusters=3)]).compute(), want)
    b._prepare_for_merge_state()
    assert len(b.features) == 1 and b.features[0].shape == (40, 6) and b.labels[0].shape == (40,)
    state = m.state_dict()
    assert sorted(state) == ["features", "labels"] and len(state["features"]) == 3
    n = SilhouetteScore()
    n.load_state_dict(state)
    assert torch.equal(n.compute(), want)
    p = pickle.loads(pickle.dumps(m))
    assert torch.equal(p.compute(), want) and p.to("cpu") is p and p.device == torch.device("cpu")
    with pytest.raises(ValueError, match="Expected \\[B, 6\\]"):
        m.update(x[:, :3], labels)
    m.reset()
    assert m.features == [] and m.labels == []
    assert SilhouetteScore().update(x.double(), labels).compute().dtype == torch.float64


def _sync_job(rank: int, ws: int):
    from torcheval_amd.metrics.toolkit import sync_and_compute

    x, labels = data(40, 4, 3, 11)
    m = SilhouetteScore(num_clusters=3)
    m.update(x[rank::2], labels[rank::2])
    return sync_and_compute(m)


def test_two_rank_gloo_sync_and_compute():
    x, labels = data(40, 4, 3, 11)
    order = torch.cat([torch.arange(0, 40, 2), torch.arange(1, 40, 2)])
    want = silhouette_score(x[order], labels[order], num_clusters=3)
    results = run_distributed(_sync_job, 2)
    assert results[0] is not None  # rank 0 is the recipient
    for got in results:
        if got is not None:
            assert float(got) == pytest.approx(float(want), rel=1e-6)


def test_exports():
    import torcheval_amd.metrics as M
    import torcheval_amd.metrics.clustering as MC
    import torcheval_amd.metrics.functional as MF
    import torcheval_amd.metrics.functional.clustering as MFC

    assert MC.SilhouetteScore is SilhouetteScore is M.SilhouetteScore
    assert MFC.silhouette_score is silhouette_score is MF.silhouette_score
    assert MFC.silhouette_samples is silhouette_samples is MF.silhouette_samples
    assert MC.__all__ == ["SilhouetteScore"] and MFC.__all__ == ["silhouette_samples", "silhouette_score"]
    # not reference names: importable from the package roots, outside their __all__
    assert "SilhouetteScore" not in M.__all__
    assert "silhouette_score" not in MF.__all__ and "silhouette_samples" not in MF.__all__


# ----------------------------------------------------------------------------- the native surface
def test_constants_match_the_header_and_the_plan():
    from torcheval_amd.ops import silhouette as K

    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    with open(os.path.join(root, "csrc", "include", "tea_kernels.h")) as fh:
        header = fh.read()
    for name, value in (("kSilTile", K.TILE), ("kSilCUs", K.CUS), ("kSilMaxGroups", K.MAX_GROUPS),
                        ("kSilBlockStages", K.BLOCK_STAGES), ("kSilEpilogueStages", K.EPILOGUE_STAGES),
                        ("kSilStitchRows", K.STITCH_ROWS)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, header).group(1)) == value
    assert K.max_panels_for(642, 8) == 14 and K.stitch_blocks(257) == 2
    assert K.groups_for(642, 14, 5, 3) == 3 and K.groups_for(642, 14, 5, 99) == 14
    # the rule at the benchmark shapes (a model): (N, K, D)
    picked = [K.groups_for(n, K.max_panels_for(n, k), d) for n, k, d in
              ((10000, 10, 64), (50000, 100, 128), (10000, 10, 2048), (50000, 1000, 16))]
    assert picked == [6, 13, 6, 13], picked
    # the plan: every sample once, in its cluster's panels; bad labels nowhere
    labels = torch.tensor([2] * 130 + [0] * 3 + [5] * 128 + [9, -1])
    labels = labels[torch.randperm(len(labels), generator=torch.Generator().manual_seed(0))]
    p = K.plan(labels, 7)
    assert p["counts"].tolist() == [3, 0, 130, 0, 0, 128, 0] and p["num_panels"].tolist() == [4]
    assert p["panel_cluster"].tolist() == [0, 2, 2, 5] + [-1] * (K.max_panels_for(263, 7) - 4)
    assert all(v.dtype == torch.int32 for v in p.values())
    assert torch.equal(p["labels"], torch.where((labels >= 0) & (labels < 7), labels, -1).int())
    rows = p["ref_index"].view(-1, K.TILE)
    assert (rows[4:] == -1).all() and (rows[0][3:] == -1).all() and (rows[2][2:] == -1).all()
    for t, c in enumerate((0, 2, 2, 5)):
        assert (labels[rows[t][rows[t] >= 0].long()] == c).all()
    kept = rows[rows >= 0]
    assert sorted(kept.tolist()) == sorted(torch.nonzero((labels >= 0) & (labels < 7)).flatten().tolist())


def test_native_op_surface_and_meta_route():
    """K23's three ops: their schemas, which dispatch keys hold a kernel, Meta kernels that return
    None, and the wrapper on meta tensors."""
    from torcheval_amd.ops import silhouette as K

    assert ops.native_loaded()
    names = sorted(n for n in torch._C._dispatch_get_all_op_names() if n.startswith("torcheval_amd_silhouette::"))
    assert names == ["torcheval_amd_silhouette::silhouette_" + s for s in ("finish", "norms", "tile")]
    ns = torch.ops.torcheval_amd_silhouette
    assert str(ns.silhouette_norms.default._schema) == (
        "torcheval_amd_silhouette::silhouette_norms(Tensor input, Tensor(a!) norms) -> ()")
    assert str(ns.silhouette_tile.default._schema) == (
        "torcheval_amd_silhouette::silhouette_tile(Tensor input, Tensor norms, Tensor labels, Tensor ref_index, "
        "Tensor panel_cluster, Tensor counts, Tensor num_panels, int groups, Tensor(a!) edges) -> ()")
    assert str(ns.silhouette_finish.default._schema) == (
        "torcheval_amd_silhouette::silhouette_finish(Tensor edges, Tensor labels, Tensor panel_cluster, "
        "Tensor counts, Tensor num_panels, Tensor(a!) block_sums, Tensor(b!) a, Tensor(c!) b, Tensor(d!) s, "
        "Tensor(e!) samples, Tensor(f!) score64, Tensor(g!) score) -> ()")
    for name in names:
        has = [k for k in ("CPU", "CUDA", "Meta") if torch._C._dispatch_has_kernel_for_dispatch_key(name, k)]
        assert has == ["CUDA", "Meta"]
    meta = torch.device("meta")
    x = torch.empty(300, 64, dtype=torch.float16, device=meta)
    labels = torch.empty(300, dtype=torch.int64, device=meta)
    assert ns.silhouette_norms.default(x.float(), torch.empty(300, dtype=torch.float64, device=meta)) is None
    out = K.silhouette(x, labels, 5, groups=2)
    for name in ("a", "b", "s"):
        assert out[name].shape == (300,) and out[name].dtype == torch.float64
    assert out["samples"].shape == (300,) and out["samples"].dtype == torch.float32
    assert out["score64"].shape == (1,) and out["score"].dtype == torch.float32 and out["score"].device.type == "meta"
    # CPU tensors, float64 and a strided feature axis are not the kernel's
    assert not K.supported(torch.rand(9, 4), torch.zeros(9, dtype=torch.int64), 2)


def test_wrapper_traces_into_one_graph():
    """The wrapper's Python (the plan, the group rule's loop, the buffer shapes, the widening copy)
    holds nothing that breaks a ``fullgraph=True`` trace; tests/gpu/test_k23_silhouette.py runs the
    graph."""
    from torcheval_amd.ops import silhouette as K

    torch._dynamo.reset()
    fn = torch.compile(lambda f, l: K.silhouette(f, l, 5), fullgraph=True, backend="eager")
    meta = torch.device("meta")
    out = fn(torch.empty(300, 64, dtype=torch.bfloat16, device=meta), torch.empty(300, dtype=torch.int32, device=meta))
    assert out["a"].shape == (300,) and out["samples"].shape == (300,) and out["score"].shape == (1,)
