"""The indices of a contingency table (K25's public interface) on CPU tensors: the ATen form against
sklearn 1.7.2, against the oracles of tests/_contingency_oracle.py (whose docstring derives the
bounds), the classes' state handling, argument errors, the export surface and the native op surface.
"""

import math
import os
import pickle
import re

import numpy as np
import pytest
import torch

import torcheval_amd.ops as ops
from tests import _contingency_oracle as O
from torcheval_amd.metrics import clustering as MC
from torcheval_amd.metrics.functional import clustering as MFC
from torcheval_amd.metrics.functional.clustering import contingency as FC



class _Sklearn:
    """sklearn.metrics, imported by the first test that compares with it: only those tests skip where
    it is not installed."""

    def __getattr__(self, name):
        return getattr(pytest.importorskip("sklearn.metrics"), name)


sk = _Sklearn()

FUNCTIONALS = ("rand_score", "adjusted_rand_score", "mutual_info_score", "normalized_mutual_info_score",
               "adjusted_mutual_info_score", "homogeneity_score", "completeness_score", "v_measure_score",
               "fowlkes_mallows_score")
CLASSES = ("RandScore", "AdjustedRandScore", "MutualInfoScore", "NormalizedMutualInfoScore",
           "AdjustedMutualInfoScore", "HomogeneityScore", "CompletenessScore", "VMeasureScore", "FowlkesMallowsScore")
# the oracle's name of a functional's value (V-measure is derived from two of them)
ORACLE_NAME = {"rand_score": "rand", "adjusted_rand_score": "adjusted_rand", "mutual_info_score": "mutual_info",
               "normalized_mutual_info_score": "normalized_mutual_info",
               "adjusted_mutual_info_score": "adjusted_mutual_info", "homogeneity_score": "homogeneity",
               "completeness_score": "completeness", "fowlkes_mallows_score": "fowlkes_mallows"}


def _random(n, r, c, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, r, (n,), generator=g), torch.randint(0, c, (n,), generator=g), r, c


def _cases():
    out = {}
    for i, (n, r, c) in enumerate(((50, 3, 5), (1000, 7, 3), (5000, 70, 3))):
        out[f"random-{n}-{r}-{c}"] = _random(n, r, c, i)
    t, _, r, _ = _random(300, 6, 6, 7)
    out["identical"] = (t, t.clone(), r, r)
    out["permuted"] = (t, torch.tensor([3, 5, 0, 1, 4, 2])[t], r, r)
    out["one-vs-singletons"] = (torch.zeros(40, dtype=torch.int64), torch.arange(40), 1, 40)
    out["singletons-vs-one"] = (torch.arange(40), torch.zeros(40, dtype=torch.int64), 40, 1)
    out["one-vs-one"] = (torch.zeros(9, dtype=torch.int64), torch.zeros(9, dtype=torch.int64), 1, 1)
    t, p, _, _ = _random(400, 4, 5, 11)
    out["empty-class-id"] = (torch.where(t >= 2, t + 1, t), p, 5, 5)  # id 2 has no member
    out["int32"] = tuple(x.int() if torch.is_tensor(x) else x for x in _random(200, 4, 4, 13))
    return out


CASES = _cases()
_ORACLES = {}


def _oracle(key):
    """Table, values and bounds of a case, once."""
    if key not in _ORACLES:
        t, p, r, c = CASES[key]
        table = O.table_of(t.numpy(), p.numpy(), r, c)
        a, b = [int(v) for v in table.sum(1)], [int(v) for v in table.sum(0)]
        emi, mag = O.emi_oracle(a, b)
        _ORACLES[key] = (table, *O.values_oracle(table, (emi, O.emi_bound(len(t), mag))), emi, mag)
    return _ORACLES[key]


def _sk(name, t, p, **kw):
    return float(getattr(sk, name)(t.numpy(), p.numpy(), **kw))


# ----------------------------------------------------------------------------- against sklearn and the oracle
@pytest.mark.parametrize("key", sorted(CASES))
def test_functionals_and_classes_against_sklearn(key):
    t, p, r, c = CASES[key]
    table, want, bound, _, _ = _oracle(key)
    got_table = MFC.contingency_matrix(t, p, num_classes=r, num_clusters=c)
    assert got_table.dtype == torch.int64 and got_table.shape == (r, c)
    # sklearn relabels to the ids present, in order: pad it back to [R, C]
    ref = np.zeros((r, c), dtype=np.int64)
    small = sk.cluster.contingency_matrix(t.numpy(), p.numpy())
    ref[np.ix_(np.unique(t.numpy()), np.unique(p.numpy()))] = small
    assert np.array_equal(got_table.numpy(), ref) and np.array_equal(ref, table)
    cells = r * c
    for name in FUNCTIONALS:
        got = getattr(MFC, name)(t, p, num_classes=r, num_clusters=c)
        assert got.dtype == torch.float64 and got.dim() == 0
        ref_value = _sk(name, t, p)
        if name == "v_measure_score":
            tol = 4 * (bound["homogeneity"] + bound["completeness"]) + 8 * O.U
        else:
            e = bound[ORACLE_NAME[name]]
            e = e[2] if isinstance(e, list) else e
            # both sides FP64; sklearn also drops MI terms below eps, one per cell at most
            tol = 2 * e + (cells * O.EPS if "info" in name or name in ("homogeneity_score", "completeness_score") else 0)
            w = want[ORACLE_NAME[name]]
            w = w[2] if isinstance(w, list) else w
            assert abs(float(got) - w) <= tol, (name, float(got), w)
        assert abs(float(got) - ref_value) <= tol * 4 + 1e-300, (name, float(got), ref_value)
        # ranges read from the labels (one host read each) agree
        assert float(getattr(MFC, name)(t, p)) == pytest.approx(float(got), abs=4 * tol + 1e-300)
        cls = getattr(MC, CLASSES[FUNCTIONALS.index(name)])
        assert float(cls(r, c).update(t, p).compute()) == float(got), name


@pytest.mark.parametrize("key", ["random-50-3-5", "random-1000-7-3", "identical", "empty-class-id"])
@pytest.mark.parametrize("method", O.METHODS)
def test_average_methods_against_sklearn(key, method):
    t, p, r, c = CASES[key]
    _, want, bound, _, _ = _oracle(key)
    k = O.METHODS.index(method)
    for name, oname, cls in (("normalized_mutual_info_score", "normalized_mutual_info", MC.NormalizedMutualInfoScore),
                             ("adjusted_mutual_info_score", "adjusted_mutual_info", MC.AdjustedMutualInfoScore)):
        got = float(getattr(MFC, name)(t, p, num_classes=r, num_clusters=c, average_method=method))
        tol = 2 * bound[oname][k] + r * c * O.EPS
        assert abs(got - want[oname][k]) <= tol, (name, got, want[oname][k])
        assert abs(got - _sk(name, t, p, average_method=method)) <= 4 * tol
        assert float(cls(r, c, average_method=method).update(t, p).compute()) == got


@pytest.mark.parametrize("beta", [0.5, 2.0])
def test_v_measure_beta(beta):
    for key in ("random-1000-7-3", "permuted", "one-vs-singletons", "one-vs-one"):
        t, p, r, c = CASES[key]
        _, _, bound, _, _ = _oracle(key)
        got = float(MFC.v_measure_score(t, p, num_classes=r, num_clusters=c, beta=beta))
        tol = 8 * (bound["homogeneity"] + bound["completeness"]) * max(1.0, beta) + 16 * O.U
        assert abs(got - _sk("v_measure_score", t, p, beta=beta)) <= tol
        assert float(MC.VMeasureScore(r, c, beta=beta).update(t, p).compute()) == got


def test_degenerate_conventions_are_sklearns():
    one, singles = torch.zeros(12, dtype=torch.int64), torch.arange(12)
    kw = dict(num_classes=12, num_clusters=12)
    # both labelings one cluster: ARI, NMI, AMI 1
    for name in ("adjusted_rand_score", "normalized_mutual_info_score", "adjusted_mutual_info_score", "rand_score"):
        assert float(getattr(MFC, name)(one, one, **kw)) == _sk(name, one, one) == 1.0
    # MI 0 (one side a single cluster): NMI and AMI 0, FMI 0 (no pair together in both)
    for name in ("normalized_mutual_info_score", "adjusted_mutual_info_score", "fowlkes_mallows_score",
                 "mutual_info_score"):
        assert float(getattr(MFC, name)(one, singles, **kw)) == _sk(name, one, singles) == 0.0
        assert float(getattr(MFC, name)(singles, one, **kw)) == _sk(name, singles, one) == 0.0
    assert float(MFC.homogeneity_score(one, singles, **kw)) == _sk("homogeneity_score", one, singles) == 1.0
    assert float(MFC.completeness_score(singles, one, **kw)) == _sk("completeness_score", singles, one) == 1.0
    # independent labelings: MI is an exact 0 after the clip, NMI 0
    t, p = torch.tensor([0, 0, 1, 1]), torch.tensor([0, 1, 0, 1])
    assert float(MFC.mutual_info_score(t, p)) == 0.0 and float(MFC.normalized_mutual_info_score(t, p)) == 0.0
    assert _sk("normalized_mutual_info_score", t, p) == 0.0
    # AMI keeps numerator and denominator eps away from 0, signs kept
    t, p = torch.tensor([0, 0, 1, 2]), torch.tensor([0, 0, 1, 1])
    assert float(MFC.adjusted_mutual_info_score(t, p)) == pytest.approx(_sk("adjusted_mutual_info_score", t, p), abs=1e-14)
    # N = 0: NaN where sklearn raises
    e = torch.zeros(0, dtype=torch.int64)
    for name in FUNCTIONALS:
        assert math.isnan(float(getattr(MFC, name)(e, e, num_classes=2, num_clusters=3)))
        assert math.isnan(float(getattr(MFC, name)(e, e)))
    assert MFC.contingency_matrix(e, e).tolist() == [[0]]


@pytest.mark.parametrize("key", sorted(CASES))
def test_expected_mutual_information_against_the_exact_oracle(key):
    t, p, r, c = CASES[key]
    table, _, _, emi, mag = _oracle(key)
    values = FC._values_aten(torch.from_numpy(table), emi=True)
    got = float(values[6])
    assert abs(got - emi) <= O.emi_bound(len(t), mag), (got, emi)
    expected_mutual_information = sk.cluster.expected_mutual_information

    present = table[table.sum(1) > 0][:, table.sum(0) > 0]  # sklearn's table has no empty ids
    assert abs(float(expected_mutual_information(present, len(t))) - emi) <= O.emi_bound(len(t), mag) + 1e-13


def test_expected_mutual_information_small_exact_cases():
    for a, b in (([2, 2], [2, 2]), ([1], [1]), ([3, 1], [3, 1]), ([0, 5, 2], [4, 0, 3])):
        table = torch.zeros(len(a), len(b), dtype=torch.int64)
        # any table with these marginals: fill greedily
        ra, cb = list(a), list(b)
        for i in range(len(a)):
            for j in range(len(b)):
                v = min(ra[i], cb[j])
                table[i, j] = v
                ra[i] -= v
                cb[j] -= v
        emi, mag = O.emi_oracle(a, b)
        got = float(FC._values_aten(table, emi=True)[6])
        assert abs(got - emi) <= O.emi_bound(sum(a), mag), (a, b, got, emi)


# ----------------------------------------------------------------------------- class behaviour
def test_class_state_updates_merge_reset_and_state_dict():
    t, p, r, c = CASES["random-1000-7-3"]
    table = _oracle("random-1000-7-3")[0]
    for name in CLASSES:
        cls = getattr(MC, name)
        whole = cls(r, c).update(t, p)
        assert whole._state_merge_kinds() == {"contingency": "sum"}
        assert whole.contingency.dtype == torch.int64 and whole.contingency.shape == (r, c)
        assert np.array_equal(whole.contingency.numpy(), table)
        want = whole.compute()
        assert want.dtype == torch.float64 and want.dim() == 0 and torch.isfinite(want)
        two = cls(r, c).update(t[:333], p[:333]).update(t[333:].int(), p[333:].int())
        assert torch.equal(two.contingency, whole.contingency) and two.compute() == want
        a, b = cls(r, c).update(t[:500], p[:500]), cls(r, c).update(t[500:], p[500:])
        assert a.merge_state([b, cls(r, c)]).compute() == want
        n = cls(r, c)
        n.load_state_dict(whole.state_dict())
        assert sorted(whole.state_dict()) == ["contingency"] and n.compute() == want
        assert pickle.loads(pickle.dumps(whole)).compute() == want
        whole.reset()
        assert whole.contingency.sum() == 0 and math.isnan(float(whole.compute()))
        assert math.isnan(float(cls(r, c).compute()))  # before any update
        e = torch.zeros(0, dtype=torch.int64)
        assert math.isnan(float(cls(r, c).update(e, e).compute()))  # N = 0


def test_totals_of_2_to_32_and_more_do_not_wrap():
    """Hand-made tables written into the state.  From a total of 2^32 on N (N - 1) / 2 leaves int64, and a
    cell above 3.03e9 does so alone: the ATen form takes FP64 pair sums there, compared with the
    Python-integer oracle under pair_bounds_f64.  One below 2^32 is still the exact route."""
    tables = ([[2**32, 5], [3, 2**31]],              # ARI about 1
              [[2**31, 2**31], [2**31, 2**31]],      # independent: ARI about 0
              [[4 * 10**9, 7], [11, 10**9], [3 * 10**9, 2 * 10**9]],
              [[2**32]],
              [[2**31, 2**30], [2**29, 2**29 - 1]])  # total 2^32 - 1
    for table in tables:
        np_table = np.array(table, dtype=np.int64)
        want, bound = O.values_oracle(np_table)
        big = int(np_table.sum()) >= 2**32
        if big:
            bound.update(O.pair_bounds_f64(np_table))
        r, c = np_table.shape
        for cls, key in ((MC.RandScore, "rand"), (MC.AdjustedRandScore, "adjusted_rand"),
                         (MC.FowlkesMallowsScore, "fowlkes_mallows"), (MC.MutualInfoScore, "mutual_info"),
                         (MC.HomogeneityScore, "homogeneity")):
            m = cls(r, c)
            m.contingency.copy_(torch.from_numpy(np_table))
            got = float(m.compute())
            assert abs(got - want[key]) <= 2 * bound[key], (table, key, got, want[key], bound[key])
        if big:
            assert max(O.pair_bounds_f64(np_table).values()) < 1e-9  # the bound itself says something
    v = FC._values_aten(torch.tensor(tables[0]), emi=False)
    assert abs(float(v[1]) - 1.0) < 1e-8 and abs(float(v[0]) - 1.0) < 1e-8


def test_bad_label_raises_at_compute_and_is_counted_nowhere():
    t = torch.tensor([0, 1, -1, 2, 1])
    p = torch.tensor([0, 1, 0, 3, 1])
    m = MC.RandScore(3, 3).update(t, p)  # -1 in labels_true, 3 in labels_pred
    assert m.contingency.tolist() == [[1, 0, 0], [0, 2, 0], [0, 0, 0]]
    with pytest.raises(ValueError, match="outside"):
        m.compute()
    assert float(m.compute()) == 1.0  # raised once; the three good pairs agree
    with pytest.raises(ValueError, match="outside"):
        MFC.rand_score(t, p, num_classes=3, num_clusters=3)
    from torcheval_amd.config import config

    old = config.validate
    config.validate = True
    try:
        with pytest.raises(ValueError, match="outside"):
            MC.RandScore(3, 3).update(t, p)
    finally:
        config.validate = old


def test_argument_errors():
    t, p = torch.tensor([0, 1, 1]), torch.tensor([1, 0, 1])
    for f in [getattr(MFC, n) for n in FUNCTIONALS] + [MFC.contingency_matrix]:
        with pytest.raises(ValueError, match="one length"):
            f(t, p[:2])
        with pytest.raises(ValueError, match="int64 or int32"):
            f(t.float(), p)
        with pytest.raises(ValueError, match="vector"):
            f(t[None], p[None])
        with pytest.raises(ValueError, match="num_classes"):
            f(t, p, num_classes=0)
        with pytest.raises(ValueError, match="num_clusters"):
            f(t, p, num_clusters=True)
    for f in (MFC.normalized_mutual_info_score, MFC.adjusted_mutual_info_score):
        with pytest.raises(ValueError, match="average_method"):
            f(t, p, average_method="harmonic")
    with pytest.raises(ValueError, match="beta"):
        MFC.v_measure_score(t, p, beta=-1.0)
    for name in CLASSES:
        with pytest.raises(ValueError, match="num_classes"):
            getattr(MC, name)(0, 3)
        with pytest.raises(ValueError, match="num_clusters"):
            getattr(MC, name)(3, None)
        with pytest.raises(ValueError, match="one length"):
            getattr(MC, name)(3, 3).update(t, p[:2])
        with pytest.raises(ValueError, match="int64 or int32"):
            getattr(MC, name)(3, 3).update(t.double(), p)
    with pytest.raises(ValueError, match="average_method"):
        MC.AdjustedMutualInfoScore(3, 3, average_method="mean")
    with pytest.raises(ValueError, match="beta"):
        MC.VMeasureScore(3, 3, beta=math.inf)


def test_exports():
    import torcheval_amd.metrics as M
    import torcheval_amd.metrics.clustering.contingency as C
    import torcheval_amd.metrics.functional as MF

    for name in CLASSES:
        assert getattr(MC, name) is getattr(C, name) is getattr(M, name)
        assert name not in M.__all__ and name not in MC.__all__
    for name in FUNCTIONALS + ("contingency_matrix",):
        assert getattr(MFC, name) is getattr(FC, name) is getattr(MF, name)
        assert name not in MF.__all__ and name not in MFC.__all__
    assert MC.__doc_extras__ == list(CLASSES)
    assert MFC.__doc_extras__ == ["contingency_matrix"] + list(FUNCTIONALS)
    assert sorted(C.__all__) == sorted(CLASSES) and sorted(FC.__all__) == sorted(FUNCTIONALS + ("contingency_matrix",))


# ----------------------------------------------------------------------------- the native surface
def test_constants_match_the_header_and_the_plan():
    from torcheval_amd.ops import contingency as K

    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    with open(os.path.join(root, "csrc", "include", "tea_kernels.h")) as fh:
        header = fh.read()
    for name, value in (("kCtgSliceSmall", K.SLICE_SMALL), ("kCtgSliceLarge", K.SLICE_LARGE),
                        ("kCtgBlockSmall", K.BLOCK_SMALL), ("kCtgBlockLarge", K.BLOCK_LARGE), ("kCtgUnit", K.UNIT),
                        ("kCtgMaxBlocks", K.MAX_BLOCKS), ("kCtgStatsBlocks", K.STATS_BLOCKS),
                        ("kCtgMarginBlocks", K.MARGIN_BLOCKS), ("kCtgEmiBlocks", K.EMI_BLOCKS),
                        ("kCtgEmiMaxParts", K.EMI_MAX_PARTS), ("kCtgInts", K.INTS), ("kCtgValues", K.VALUES)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, header).group(1)) == value
    assert re.search(r"constexpr int kCtgMaxCells = 1 << (\d+);", header).group(1) == "22" and K.MAX_CELLS == 1 << 22
    with open(os.path.join(root, "csrc", "kernels", "contingency.hip")) as fh:
        kernel = fh.read()
    for name, value in (("kRows", K._ROWS), ("kStatBlock", K._STAT_BLOCK), ("kEmiTargetItems", K._EMI_TARGET_ITEMS)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, kernel).group(1)) == value
    assert K.VALUES == max(K.INDEX.values()) + 1 and K.INDEX["adjusted_mutual_info"] + 4 == K.INDEX["homogeneity"]
    # the plan: a table the small slice holds takes it below LARGE_FROM_PAIRS pairs; the grid stays bounded
    assert K.plan(10**7, 100) == (K.SLICE_LARGE, 611) and K.plan(1, 100) == (K.SLICE_SMALL, 1)
    assert K.plan(10**6 - 1, K.SLICE_SMALL) == (K.SLICE_SMALL, 245) and K.plan(10**6, 100) == (K.SLICE_LARGE, 62)
    assert K.plan(10**7, 100, K.SLICE_SMALL) == (K.SLICE_SMALL, 1024)
    assert K.plan(10**7, K.SLICE_SMALL + 1) == (K.SLICE_LARGE, 611)
    assert K.plan(10**7, 10**6) == (K.SLICE_LARGE, 1024 // 31) and K.plan(10**7, 4 * 10**6) == (K.SLICE_LARGE, 8)
    assert K.plan(10**7, K.SLICE_SMALL + 1, K.SLICE_SMALL) == (K.SLICE_SMALL, 512)
    assert K.stats_blocks(1, 1) == 1 and K.stats_blocks(2000, 2000) == 1000 and K.stats_blocks(4096, 1024) == 1024 and K.margin_blocks(7, 1) == 1
    assert K.emi_parts(2, 2) == 64 and K.emi_parts(1000, 1000) == 1 and K.emi_blocks(2, 2) == 64
    assert K.emi_blocks(3, 70) == 1050 and K.emi_blocks(1000, 1000) == K.EMI_BLOCKS


@pytest.mark.skipif(not ops.native_loaded(), reason="the native extension is not built")
def test_native_op_surface_and_meta_route():
    """K25's four ops: their schemas, which dispatch keys hold a kernel, Meta kernels that return
    None, and the wrapper on meta tensors."""
    from torcheval_amd.ops import contingency as K

    names = sorted(n for n in torch._C._dispatch_get_all_op_names() if n.startswith("torcheval_amd_contingency::"))
    assert names == ["torcheval_amd_contingency::contingency_" + s for s in ("emi", "stats", "update", "values")]
    ns = torch.ops.torcheval_amd_contingency
    assert str(ns.contingency_update.default._schema) == (
        "torcheval_amd_contingency::contingency_update(Tensor labels_true, Tensor labels_pred, int slice, int groups, "
        "Tensor(a!) table, Tensor(b!)? err) -> ()")
    assert str(ns.contingency_stats.default._schema) == (
        "torcheval_amd_contingency::contingency_stats(Tensor table, Tensor(a!) marginals, Tensor(b!) cell_partials, "
        "Tensor(c!) margin_partials, Tensor(d!) margin_logs) -> ()")
    assert str(ns.contingency_emi.default._schema) == (
        "torcheval_amd_contingency::contingency_emi(Tensor marginals, Tensor margin_logs, int num_classes, "
        "int num_clusters, Tensor(a!) emi_partials) -> ()")
    assert str(ns.contingency_values.default._schema) == (
        "torcheval_amd_contingency::contingency_values(Tensor marginals, Tensor cell_partials, "
        "Tensor margin_partials, Tensor? emi_partials, Tensor(a!) values) -> ()")
    for name in names:
        has = [k for k in ("CPU", "CUDA", "Meta") if torch._C._dispatch_has_kernel_for_dispatch_key(name, k)]
        assert has == ["CUDA", "Meta"]
    meta = torch.device("meta")
    labels = torch.empty(300, dtype=torch.int64, device=meta)
    table = torch.empty(7, 5, dtype=torch.int64, device=meta)
    assert ns.contingency_update.default(labels, labels, K.SLICE_SMALL, 1, table, None) is None
    values, total = K.contingency_values(table)
    assert values.shape == (K.VALUES,) and values.dtype == torch.float64 and values.device.type == "meta"
    assert total.shape == () and total.dtype == torch.int64
    # CPU tensors, strided labels and tables past the cap are not the kernels'
    cpu = torch.zeros(9, dtype=torch.int64)
    assert not K.supported(cpu, cpu, torch.zeros(2, 2, dtype=torch.int64)) and not K.supported_table(torch.zeros(2, 2))
