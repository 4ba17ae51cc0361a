"""K23 (csrc/kernels/silhouette.hip) on the device: the silhouette coefficient against an
independent numpy oracle written here (direct differences, a loop over samples and clusters,
``math.fsum``).

The sharp tests use integer features with ``|x| <= 8`` and ``D <= 260`` as float32: every product and
partial sum of an inner product stays below 2^24, so every squared distance is exact in the kernel
and only the FP64 square root and the order of the sums separate kernel and oracle.  ``a`` and ``b``
are asserted relative to the oracle at ``2 (n_c + 2) 2^-53`` with ``n_c`` the size of the cluster
summed (one rounding per square root, ``n_c - 1`` per sum, one per division, and the same again for
the oracle; for ``b``, a minimum of such means, the largest other cluster), ``s`` at the error that
propagates from these.  Random float32 data is compared under bounds computed from the data
(docstring of ``float_bounds``).
"""

import functools
import math

import numpy as np
import pytest
import torch

from torcheval_amd.metrics import SilhouetteScore
from torcheval_amd.metrics.functional import silhouette_samples, silhouette_score
from torcheval_amd.metrics.functional.clustering.silhouette import _silhouette
from torcheval_amd.ops import silhouette as K

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
T = K.TILE
U = 2.0**-53
NAMES = ("a", "b", "s", "samples", "score64", "score")


# ----------------------------------------------------------------------------- oracle
def oracle(x, labels, k):
    """a, b, s [N] and the score by the definition; a row with a non-finite feature is at distance
    NaN from every other row, a NaN mean is no candidate for b, a bad label is in no cluster."""
    x = x.cpu().double().numpy()
    lab = labels.cpu().numpy().astype(np.int64)
    n = len(x)
    ok = (lab >= 0) & (lab < k)
    members = [np.flatnonzero(lab == c) for c in range(k)]
    counts = np.array([len(m) for m in members])
    poisoned = ~np.isfinite(x).all(axis=1)
    a, b, s = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    nb = np.zeros(n, dtype=np.int64)  # the largest other cluster: the n_c of b's bound
    for i in np.flatnonzero(ok):
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
            else:
                nb[i] = max(nb[i], counts[c])
                mean = total / counts[c]
                if not math.isnan(mean) and (math.isnan(best) or mean < best):
                    best = mean
        b[i] = best
        top = max(a[i], b[i])
        if math.isnan(a[i]) or math.isnan(b[i]):
            s[i] = math.nan
        elif counts[lab[i]] == 1 or top == 0.0:
            s[i] = 0.0
        else:
            s[i] = (b[i] - a[i]) / top
    score = math.fsum(s[ok]) / ok.sum() if (counts > 0).sum() >= 2 else math.nan
    return {"a": a, "b": b, "s": s, "score": score, "n_a": counts[np.where(ok, lab, 0)], "n_b": nb}


def s_bound(want, e_a, e_b):
    """|s - oracle| from absolute errors of a and b: both quotients a / max and b / max move by at
    most (E_a + E_b) / (max - E_a - E_b); a few roundings of the last operations on top."""
    top = np.maximum(want["a"], want["b"])
    with np.errstate(invalid="ignore", divide="ignore"):
        e = 2.0 * (e_a + e_b) / (top - e_a - e_b) + 4 * U
    return np.where((top == 0) | ~np.isfinite(top), 0.0, e)


def check_integer(x, labels, k, groups=0):
    """The call against the oracle under the bounds of the module docstring; returns the call's
    dictionary."""
    want = cached_oracle(x, labels, k)
    got = _silhouette(x, labels, k, groups)
    out = {name: got[name].cpu().numpy() for name in NAMES}
    assert got["a"].dtype == torch.float64 and got["samples"].dtype == torch.float32 and got["a"].device == DEV
    e_a = 2 * (want["n_a"] + 2) * U * np.abs(want["a"])
    e_b = 2 * (want["n_b"] + 2) * U * np.abs(want["b"])
    for name, bound in (("a", e_a), ("b", e_b), ("s", s_bound(want, e_a, e_b))):
        assert np.array_equal(np.isnan(out[name]), np.isnan(want[name])), name
        err = np.nan_to_num(np.abs(out[name] - want[name]))
        worst = int(np.argmax(err - np.nan_to_num(bound)))
        assert (err <= np.nan_to_num(bound)).all(), (name, worst, out[name][worst], want[name][worst])
    assert np.array_equal(out["samples"], out["s"].astype(np.float32), equal_nan=True)
    if math.isnan(want["score"]):
        assert math.isnan(out["score64"][0]) and math.isnan(out["score"][0])
    else:
        e_s = float(np.nanmean(s_bound(want, e_a, e_b))) + 2 * (len(x) + 2) * U
        assert abs(out["score64"][0] - want["score"]) <= e_s
        assert out["score"][0] == np.float32(out["score64"][0])
    return got


_ORACLES = {}


def cached_oracle(x, labels, k):
    key = (x.cpu().numpy().tobytes(), labels.cpu().numpy().tobytes(), x.shape, k)
    if key not in _ORACLES:
        _ORACLES[key] = oracle(x, labels, k)
    return _ORACLES[key]


def same(a, b):
    return all(torch.equal(a[name].view(torch.int64 if a[name].dtype == torch.float64 else torch.int32),
                           b[name].view(torch.int64 if b[name].dtype == torch.float64 else torch.int32))
               for name in NAMES)


# ----------------------------------------------------------------------------- data
@functools.lru_cache(maxsize=None)
def integer_data(sizes, d, seed, shuffle=True):
    """Cluster c has sizes[c] members (0: an empty id): an integer centre in [-4, 4] plus integer
    noise in [-4, 4], so |x| <= 8.  Shuffled unless asked otherwise."""
    g = torch.Generator().manual_seed(seed)
    labels = torch.cat([torch.full((m,), c, dtype=torch.int64) for c, m in enumerate(sizes)])
    centres = torch.randint(-4, 5, (len(sizes), d), generator=g)
    x = centres[labels] + torch.randint(-4, 5, (len(labels), d), generator=g)
    if shuffle:
        perm = torch.randperm(len(labels), generator=g)
        x, labels = x[perm], labels[perm]
    return x.float().to(DEV), labels.to(DEV)


# ----------------------------------------------------------------------------- exact data
def test_two_singletons_and_a_pair_with_a_singleton():
    x = torch.tensor([[0.0, 3.0], [4.0, 0.0]], device=DEV)
    got = check_integer(x, torch.tensor([0, 1], device=DEV), 2)
    assert got["b"].tolist() == [5.0, 5.0] and got["s"].tolist() == [0.0, 0.0] and float(got["score"]) == 0.0
    x = torch.tensor([[0.0, 0.0], [0.0, 2.0], [0.0, 8.0]], device=DEV)
    got = check_integer(x, torch.tensor([1, 1, 0], device=DEV), 2)
    assert got["a"].tolist() == [2.0, 2.0, 0.0] and got["b"].tolist() == [8.0, 6.0, 7.0]
    assert got["s"].tolist() == [0.75, 4.0 / 6.0, 0.0]


def test_panel_boundaries_a_one_row_second_panel_a_singleton_and_empty_ids():
    x, labels = integer_data((127, 0, 128, 129, 0, 1, 257, 0), 5, 1)
    assert len(x) == 642
    check_integer(x, labels, 8)


@pytest.mark.parametrize("n", [129, 257])
def test_column_tile_tail(n):
    check_integer(*integer_data((n - 60, 60), 7, n), 2)


@pytest.mark.parametrize("d", [1, 3, 4, 32, 33, 128, 129, 260])
def test_stage_and_chunk_boundaries_in_both_load_arms(d):
    """Inner products stay below 64 * 260 < 2^24."""
    check_integer(*integer_data((70, 131, 40), d, d), 3)


@pytest.mark.parametrize("groups", [1, 2, 3, 5])
def test_forced_groups_with_a_cluster_across_three_ranges(groups):
    """Nine panels: 1 + 1 + 4 (the 400-row cluster) + 1 + 1 + 1.  At G = 5 the ranges are
    [0, 1), [1, 3), [3, 5), [5, 7), [7, 9): the large cluster ends one, fills one and starts one; at
    G = 2 and 3 small clusters lie wholly inside a range next to it."""
    x, labels = integer_data((50, 30, 400, 20, 128, 9), 6, 11)
    assert K.groups_for(len(x), K.max_panels_for(len(x), 6), 6, groups) == groups
    check_integer(x, labels, 6, groups)


@pytest.mark.parametrize("groups", [1, 3])
def test_many_tiny_clusters_nearly_all_padding(groups):
    sizes = tuple(2 + (c % 2) for c in range(64))
    check_integer(*integer_data(sizes, 4, 12), 64, groups)


def test_shuffled_against_sorted_labels():
    sizes = (127, 130, 43)
    x, labels = integer_data(sizes, 9, 13)
    got = check_integer(x, labels, 3)
    order = torch.argsort(labels, stable=True)
    sorted_ = check_integer(x[order].contiguous(), labels[order].contiguous(), 3)
    # the same samples in another order: another association of the same sums
    want = cached_oracle(x, labels, 3)
    tol = torch.tensor(2 * (want["n_b"].max() + 2) * U * 2, device=DEV)
    assert (got["a"][order] - sorted_["a"]).abs().max() <= tol * got["a"].abs().max()
    assert (got["b"][order] - sorted_["b"]).abs().max() <= tol * got["b"].abs().max()


def test_clusters_of_identical_points_score_zero_exactly():
    x = torch.zeros(140, 3, device=DEV)
    x[:, 1] = 5.0
    labels = torch.cat([torch.zeros(131, dtype=torch.int64), torch.ones(9, dtype=torch.int64)]).to(DEV)
    got = check_integer(x, labels, 2)  # a = b = 0 everywhere
    assert float(got["a"].abs().max()) == 0.0 and float(got["b"].abs().max()) == 0.0
    assert float(got["s"].abs().max()) == 0.0 and float(got["score"]) == 0.0
    x[131:, 0] = 4.0  # two clusters of identical points, 4 apart: a = 0, b = 4, s = 1
    got = check_integer(x, labels, 2)
    assert float(got["a"].abs().max()) == 0.0 and got["b"].unique().tolist() == [4.0]
    assert got["s"].unique().tolist() == [1.0] and float(got["score"]) == 1.0


def test_misaligned_and_row_padded_features_take_the_element_arm_bit_for_bit():
    for d in (64, 30):
        x, labels = integer_data((100, 131, 29), d, 14 + d)
        want = check_integer(x, labels, 3)
        parent = torch.full((len(x), d + 7), 3.0, device=DEV)
        parent[:, 1 : 1 + d] = x
        view = parent[:, 1 : 1 + d]  # one column into a wider parent: rows 4 bytes off, padded
        assert view.data_ptr() % 16 == 4 and view.stride() == (d + 7, 1) and K.supported(view, labels, 3)
        assert same(_silhouette(view, labels, 3), want)
    # a 16-byte aligned view with a padded row stride stays in the vector arm
    x, labels = integer_data((100, 131, 29), 64, 14 + 64)
    parent = torch.zeros(len(x), 64 + 8, device=DEV)
    parent[:, 4:68] = x
    assert same(_silhouette(parent[:, 4:68], labels, 3), check_integer(x, labels, 3))


def test_the_same_call_twice_is_bit_identical_and_labels_may_be_int32():
    x, labels = integer_data((127, 0, 128, 129, 0, 1, 257, 0), 5, 1)
    first = _silhouette(x, labels, 8)
    assert same(_silhouette(x, labels, 8), first)
    assert same(_silhouette(x, labels.int(), 8), first)
    assert torch.equal(silhouette_samples(x, labels), first["samples"])  # num_clusters from labels.max()
    assert torch.equal(silhouette_score(x, labels, num_clusters=8), first["score"][0])


def test_nan_feature():
    """The poisoned row alone in a third cluster: NaN for itself only.  The same row inside the
    first cluster: NaN for that cluster's members only.  The score is NaN both times."""
    x, labels = integer_data((90, 140, 1), 6, 15, shuffle=False)
    x = x.clone()
    x[230, 2] = float("nan")
    got = check_integer(x, labels, 3)
    samples = silhouette_samples(x, labels, num_clusters=3)
    assert torch.isnan(samples).nonzero().flatten().tolist() == [230]
    assert torch.isfinite(samples[:230]).all() and torch.isnan(silhouette_score(x, labels, num_clusters=3))
    assert torch.isnan(got["score64"]).all()
    x, labels = integer_data((90, 140, 20), 6, 16, shuffle=False)
    x = x.clone()
    x[7, 0] = float("inf")
    check_integer(x, labels, 3)
    samples = silhouette_samples(x, labels, num_clusters=3)
    assert torch.isnan(samples[:90]).all() and torch.isfinite(samples[90:]).all()
    assert torch.isnan(silhouette_score(x, labels, num_clusters=3))


def test_bad_labels_belong_to_no_cluster_and_raise_under_validate():
    from torcheval_amd.config import config

    x, labels = integer_data((60, 70, 9), 5, 17)
    bad = labels.clone()
    bad[3], bad[100] = 3, -1
    keep = torch.ones(len(x), dtype=torch.bool, device=DEV)
    keep[3] = keep[100] = False
    got = check_integer(x, bad, 3)
    clean = check_integer(x[keep].contiguous(), labels[keep].contiguous(), 3)
    assert torch.isnan(got["s"][~keep]).all() and torch.allclose(got["s"][keep], clean["s"], rtol=1e-13, atol=0)
    assert torch.allclose(got["score64"], clean["score64"], rtol=1e-13, atol=0)
    assert torch.isfinite(silhouette_score(x, bad, num_clusters=3))
    previous = config.validate
    config.validate = True
    try:
        with pytest.raises(ValueError, match="outside \\[0, num_clusters\\)"):
            silhouette_score(x, bad, num_clusters=3)
        assert torch.isfinite(silhouette_score(x, labels, num_clusters=3))
    finally:
        config.validate = previous


def test_fewer_than_two_clusters_is_nan_and_all_singletons_is_zero():
    x, _ = integer_data((70, 61), 5, 18)
    one = torch.full((len(x),), 2, dtype=torch.int64, device=DEV)
    got = check_integer(x, one, 4)
    assert torch.isnan(got["score"]).all() and torch.isnan(got["samples"]).all()
    assert torch.isnan(silhouette_score(x[:1], one[:1], num_clusters=4))
    every = torch.arange(len(x), device=DEV)
    got = check_integer(x, every, len(x))
    assert float(got["score"]) == 0.0 and float(got["s"].abs().max()) == 0.0


def test_half_features_equal_the_float32_call_on_the_widened_copy():
    x, labels = integer_data((100, 131, 29), 48, 19)
    x = x * 0.25 + 0.5
    for dtype in (torch.float16, torch.bfloat16):
        h = x.to(dtype)
        assert K.supported(h, labels, 3)
        assert same(_silhouette(h, labels, 3), _silhouette(h.float(), labels, 3))
        assert silhouette_score(h, labels, num_clusters=3).dtype == torch.float32


def test_unsupported_calls_take_the_aten_form():
    x, labels = integer_data((40, 45), 16, 20)
    wide = torch.zeros(len(x), 32, device=DEV)
    wide[:, ::2] = x
    assert K.supported(x, labels, 2) and not K.supported(wide[:, ::2], labels, 2)
    assert not K.supported(x.double(), labels, 2) and not K.supported(x.cpu(), labels.cpu(), 2)
    want = cached_oracle(x, labels, 2)
    for got in (_silhouette(wide[:, ::2], labels, 2), _silhouette(x.double(), labels, 2)):
        np.testing.assert_allclose(got["s"].cpu().numpy(), want["s"], rtol=0, atol=1e-12)
    out = silhouette_score(x.double(), labels, num_clusters=2)
    assert out.dtype == torch.float64 and abs(float(out) - want["score"]) < 1e-12


def test_aten_form_on_the_device_with_more_than_2_24_distances_in_a_block():
    """4200^2 distances in one block of the ATen form: the direct-difference ``cdist`` kernel left
    everything past the first 2^24 outputs of a call at 0 on this runtime, which halved the scores
    at the benchmark shapes (``_distance_block``).  Integer data, so the device's ``mm`` form is
    exact; the CPU form (direct differences) is the reference, and K23 agrees with both."""
    from torcheval_amd.metrics.functional.clustering.silhouette import _silhouette_aten

    n = 4200
    assert n * n > 2**24
    x, labels = integer_data((1500, 1300, 1400), 8, 23)
    on_device = _silhouette_aten(x.double(), labels, 3)
    on_host = _silhouette_aten(x.double().cpu(), labels.cpu(), 3)
    native = _silhouette(x, labels, 3)
    assert abs(float(on_host["score64"])) > 0.1
    for name in ("a", "b", "s", "score64"):
        assert torch.allclose(on_device[name].cpu(), on_host[name], rtol=0, atol=1e-12), name
        assert torch.allclose(native[name].cpu(), on_host[name], rtol=0, atol=1e-11), name


# ----------------------------------------------------------------------------- float data
def float_bounds(x, labels, k):
    """K22's error model (``float_bounds`` of tests/gpu/test_k22_prdc.py), unchanged:
    ``e(i, j) = 2 eps sum_k |x_ik| |x_jk|`` with ``eps = min(D 2^-24, 4e-7)`` bounds the error of one
    squared distance.  A distance then moves by at most ``min(sqrt(e), e / d)`` with ``d`` the
    oracle's distance, ``a`` by the mean of that over its cluster and ``b`` by the largest such mean
    over the other clusters.  Returns (E_a, E_b), both [N]."""
    xa = x.cpu().double().numpy()
    lab = labels.cpu().numpy()
    e = 2.0 * min(xa.shape[1] * 2.0**-24, 4e-7) * (np.abs(xa) @ np.abs(xa).T)
    d = np.stack([np.sqrt(((xa - row) ** 2).sum(axis=1)) for row in xa])
    with np.errstate(divide="ignore", invalid="ignore"):
        move = np.minimum(np.sqrt(e), np.where(d > 0, e / d, np.inf))
    np.fill_diagonal(move, 0.0)
    n = len(xa)
    e_a, e_b = np.zeros(n), np.zeros(n)
    for c in range(k):
        m = lab == c
        if not m.any():
            continue
        total = move[:, m].sum(axis=1)
        e_a[m] = total[m] / max(1, m.sum() - 1)
        e_b[~m] = np.maximum(e_b[~m], total[~m] / m.sum())
    return e_a, e_b


@pytest.mark.parametrize("n,d,k", [(300, 64, 4), (200, 33, 7), (385, 768, 3), (385, 2048, 5)])
def test_random_clustered_features_inside_the_computed_bounds(n, d, k):
    """Centres plus noise, so the score is well away from 0.  ``a`` and ``b`` are asserted at twice the
    bounds of ``float_bounds`` (K22's margin), ``s`` at ``2 (E_a + E_b) / (max(a, b) - E_a - E_b)``
    and the score at the mean of that.

    Measured on an MI355X (largest error of a, b, s with the bound at that sample and the largest
    error / bound over all samples; then the score's error against its bound):
      300 x 64, K = 4     a 1.5e-6 (5.0e-5, 0.031), b 4.4e-7 (1.6e-5, 0.027), s 4.5e-7 (3.6e-5, 0.012); 2.8e-9 / 3.8e-5
      200 x 33, K = 7     a 1.4e-6 (4.3e-5, 0.033), b 3.4e-7 (1.6e-5, 0.023), s 6.8e-7 (5.3e-5, 0.013); 5.7e-8 / 5.4e-5
      385 x 768, K = 3    a 2.4e-6 (1.7e-4, 0.014), b 5.9e-7 (4.9e-5, 0.012), s 2.0e-7 (3.7e-5, 0.005); 1.2e-9 / 3.6e-5
      385 x 2048, K = 5   a 4.1e-6 (2.8e-4, 0.015), b 1.1e-6 (7.8e-5, 0.014), s 2.2e-7 (3.7e-5, 0.006); 1.6e-9 / 3.7e-5
    with scores of 0.60 to 0.67.  A mean over a cluster averages the distances' errors, so the
    figures sit far lower in their bounds than K22's single distances do (0.19 to 0.30).  The main
    loop is K22's chunked one; a single-chain main loop was not tried."""
    g = torch.Generator().manual_seed(n + d)
    labels = torch.randint(0, k, (n,), generator=g)
    x = (torch.rand(k, d, generator=g)[labels] + 0.35 * torch.rand(n, d, generator=g)).to(DEV)
    labels = labels.to(DEV)
    want = oracle(x, labels, k)
    e_a, e_b = float_bounds(x, labels, k)
    e_a, e_b = 2 * e_a, 2 * e_b
    e_s = s_bound(want, e_a, e_b)
    got = _silhouette(x, labels, k)
    out = {name: got[name].cpu().numpy() for name in NAMES}
    errors = {name: np.abs(out[name] - want[name]) for name in ("a", "b", "s")}
    score_err, score_bound = abs(out["score64"][0] - want["score"]), float(e_s.mean())
    # every figure first, then the assertions
    for name, bound in (("a", e_a), ("b", e_b), ("s", e_s)):
        worst = int(np.argmax(errors[name] / bound))
        print(f"N={n} D={d} K={k}: max |{name} - oracle| = {errors[name].max():.3e} (bound there "
              f"{bound[int(np.argmax(errors[name]))]:.3e}); worst ratio {errors[name][worst] / bound[worst]:.3f}")
    print(f"  score {out['score64'][0]:.6f}, |score - oracle| = {score_err:.3e}, bound {score_bound:.3e}")
    assert abs(want["score"]) > 0.2
    for name, bound in (("a", e_a), ("b", e_b), ("s", e_s)):
        assert (errors[name] <= bound).all(), name
    assert score_err <= score_bound
    assert same(_silhouette(x, labels, k), got)  # bit-identical from run to run


# ----------------------------------------------------------------------------- functional, class, compile
def test_class_on_device_equals_the_functional_on_the_concatenation():
    x, labels = integer_data((100, 131, 29), 12, 21)
    want = silhouette_score(x, labels, num_clusters=3)
    assert want.dtype == torch.float32 and want.shape == () and want.device == DEV
    m = SilhouetteScore(num_clusters=3, device=DEV)
    for lo, hi in ((0, 1), (1, 130), (130, 260)):
        m.update(x[lo:hi], labels[lo:hi])
    got = m.compute()
    assert got.device == DEV and torch.equal(got, want) and torch.equal(m.compute(), got)
    other = SilhouetteScore(device=DEV).update(x[:60].cpu(), labels[:60].int().cpu())
    other.merge_state([SilhouetteScore(device=DEV).update(x[60:], labels[60:])])
    assert torch.equal(other.compute(), want)


def test_compiled_call_matches_eager():
    """``fullgraph=True`` through AOT autograd's functionalisation of the mutating ops; the backend
    runs the graph with ATen, since everything in it but K23's three ops is index plumbing."""
    x, labels = integer_data((100, 131, 29), 64, 22)
    torch._dynamo.reset()
    fn = torch.compile(lambda f, l: K.silhouette(f, l, 3), fullgraph=True, backend="aot_eager")
    eager = check_integer(x, labels, 3)
    assert same(fn(x, labels), eager)
    assert same(fn(x.half(), labels), eager)  # the widening copy stays in the graph
