"""K22 (csrc/kernels/prdc.hip) on the device: improved precision / recall and density / coverage
against an independent numpy oracle written here.

The sharp tests use exact data: integer features in [0, 4) as float32.  Every norm, every dot
product (below 2^24) and every squared distance is then an integer that both paths represent
exactly, so radii, hits, nearest values and tallies must equal the oracle's exactly: one padding
column counted, one row compared with itself, one ``<`` in place of ``<=`` or one wrong k-th value
among ties changes the result.  Random float32 data is compared under bounds computed from the data
(docstring of ``float_bounds``).
"""

import numpy as np
import pytest
import torch

from torcheval_amd.metrics import DensityCoverage, ImprovedPrecisionRecall
from torcheval_amd.metrics.functional import density_coverage, improved_precision_recall
from torcheval_amd.metrics.functional.image.prdc import _prdc
from torcheval_amd.ops import prdc as K

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
T = K.TILE
WIDTHS = [1, 3, 4, 31, 32, 33, 64, 100, 256]
NAMES = ("radii_real", "radii_fake", "hits_real", "hits_fake", "nearest_real", "nearest_fake", "tallies", "values")


# ----------------------------------------------------------------------------- oracle
def distances(a, b):
    """[len(a), len(b)] FP64 squared distances by the definition."""
    na, nb = (a * a).sum(1), (b * b).sum(1)
    return np.maximum(0.0, (na[:, None] + nb[None, :]) - 2.0 * (a @ b.T))


def oracle(real, fake, k):
    x, y = real.cpu().double().numpy(), fake.cpu().double().numpy()

    def radii(a):
        d = distances(a, a)
        np.fill_diagonal(d, np.inf)
        return np.sort(d, axis=1)[:, k - 1]

    rr, rf = radii(x), radii(y)
    dfx = distances(y, x)
    dxf = dfx.T
    out = {
        "radii_real": rr, "radii_fake": rf,
        "hits_fake": (dfx <= rr[None, :]).sum(1), "hits_real": (dxf <= rf[None, :]).sum(1),
        "nearest_fake": dfx.min(1), "nearest_real": dxf.min(1),
    }
    out["tallies"] = np.array([(out["hits_fake"] > 0).sum(), (out["hits_real"] > 0).sum(), out["hits_fake"].sum(),
                               (out["nearest_real"] <= rr).sum()], dtype=np.int64)
    return out


def values_of(tallies, n, m, k):
    return (np.asarray(tallies, dtype=np.float64) / np.array([m, n, k * m, n], dtype=np.float64)).astype(np.float32)


def check_exact(real, fake, k, groups=0):
    want = oracle(real, fake, k)
    got = _prdc(real, fake, k, groups)
    for name in ("radii_real", "radii_fake", "nearest_real", "nearest_fake"):
        assert got[name].dtype == torch.float64 and got[name].device == DEV
        assert np.array_equal(got[name].cpu().numpy(), want[name]), name
    for name in ("hits_real", "hits_fake"):
        assert got[name].dtype == torch.int32
        assert np.array_equal(got[name].cpu().numpy(), want[name]), name
    assert got["tallies"].dtype == torch.int64 and np.array_equal(got["tallies"].cpu().numpy(), want["tallies"])
    assert got["values"].dtype == torch.float32
    assert np.array_equal(got["values"].cpu().numpy(), values_of(want["tallies"], len(real), len(fake), k))
    return got


def same(a, b):
    return all(torch.equal(a[name], b[name]) for name in NAMES)


# ----------------------------------------------------------------------------- data
def integer_features(n_r, n_f, d, seed):
    """Integers in [0, 4).  Row i of the real side is non-zero only in its first 1 + i d // n_r
    columns and row j of the generated side in its first 1 + d // 4 + 3 j d // (4 n_f), so norms
    grow with the row number, the rows are not exchangeable and the two sets overlap in part
    (tests/metrics/image/test_prdc.py holds the four values at 130 x 129 x 64 inside 0.6 .. 1.2)."""
    g = torch.Generator().manual_seed(seed)
    cols = torch.arange(d)[None, :]
    real = torch.randint(0, 4, (n_r, d), generator=g).float()
    real = real * (cols <= (torch.arange(n_r)[:, None] * d) // n_r)
    fake = torch.randint(0, 4, (n_f, d), generator=g).float()
    fake = fake * (cols <= d // 4 + (3 * torch.arange(n_f)[:, None] * d) // (4 * n_f))
    return real.to(DEV), fake.to(DEV)


def sizes(k):
    return [k + 1, 31, 33, T - 1, T, T + 1, 2 * T + 1]


def size_pairs(k):
    """Every size on either side, N != M in all pairs but one."""
    s = sizes(k)
    return [(s[i], s[(i + 3) % len(s)]) for i in range(len(s))] + [(T + 1, T + 1)]


# ----------------------------------------------------------------------------- exact data
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("k", [1, 3, 5, 8])
def test_exact_at_every_tile_and_width_edge(k, d):
    """Dot products stay below 9 * 256 < 2^24, squared distances below 2 * 9 * 256."""
    for n, m in size_pairs(k):
        check_exact(*integer_features(n, m, d, 1000 * n + m + d), k)


@pytest.mark.parametrize("d", [129, 132, 160])
def test_exact_where_a_stage_follows_a_chain_boundary(d):
    """The MFMA chains are 128 k long (four stages of 32).  WIDTHS ends inside one chain (100) or on
    a boundary (256); here a second chain holds a partial stage, through the element loads (129) and
    the 16-byte loads (132), or exactly one full stage (160).  Dot products stay below
    9 * 160 = 1440."""
    for n, m in size_pairs(3):
        check_exact(*integer_features(n, m, d, 1000 * n + m + d), 3)


@pytest.mark.parametrize("k", [1, 5, 8])
@pytest.mark.parametrize("d", [4, 64])
def test_every_group_count_gives_the_same_lists(k, d):
    """Three column tiles per pass: one block walks them all (G = 1), two share them unevenly, every
    block takes one (G = 3 = the rule here); the k smallest are a multiset, so nothing may move."""
    n = 2 * T + 1
    real, fake = integer_features(n, n - 40, d, k + d)
    assert K.groups_for(n, n, d) == 3 and K.groups_for(n - 40, n, d) == 3 and K.groups_for(n, n - 40, d) == 2
    first = check_exact(real, fake, k, 0)
    for groups in (1, 2, 3):
        assert same(check_exact(real, fake, k, groups), first)


@pytest.mark.parametrize("k", [1, 2, 8])
def test_tie_stress_at_width_four(k):
    """D = 4: at most 4^4 distinct rows, so duplicates and equal distances are everywhere, radii
    of 0 included."""
    for n, m in ((2 * T + 1, T + 7), (T + 1, 2 * T + 1)):
        real, fake = integer_features(n, m, 4, n + k)
        got = check_exact(real, fake, k)
        if k == 1:
            assert int((got["radii_real"] == 0).sum()) > 0 and int((got["radii_fake"] == 0).sum()) > 0


def test_strided_and_misaligned_features_take_the_element_arm():
    n, m, d, k = T + 6, T + 3, 64, 3
    real, fake = integer_features(n, m, d, 5)
    want = check_exact(real, fake, k)
    # a column slice of a wider parent: row stride 200, still 16-byte aligned rows
    parent = torch.full((n, 200), 3.0, device=DEV)
    parent[:, 8 : 8 + d] = real
    view = parent[:, 8 : 8 + d]
    assert view.stride() == (200, 1) and view.data_ptr() % 16 == 0 and K.supported(view, fake, k)
    assert same(_prdc(view, fake, k), want)
    # the same slice one column on: rows 4 bytes off a 16-byte boundary
    parent[:, 9 : 9 + d] = real
    view = parent[:, 9 : 9 + d]
    assert view.data_ptr() % 16 == 4 and K.supported(view, fake, k)
    assert same(_prdc(view, fake, k), want)
    # a contiguous tensor whose base is 4 bytes off, on the other side
    flat = torch.zeros(m * d + 1, device=DEV)
    off = flat[1:].view(m, d)
    off.copy_(fake)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    assert same(_prdc(real, off, k), want)
    # a row stride that is no multiple of 4 floats
    parent = torch.zeros(n, d + 3, device=DEV)
    parent[:, :d] = real
    assert same(_prdc(parent[:, :d], fake, k), want)


def test_unsupported_calls_take_the_aten_form_and_stay_exact():
    real, fake = integer_features(40, 45, 16, 6)
    want = oracle(real, fake, 3)
    wide = torch.zeros(40, 32, device=DEV)
    wide[:, ::2] = real
    assert K.supported(real, fake, 3) and not K.supported(wide[:, ::2], fake, 3)
    assert not K.supported(real.double(), fake.double(), 3) and not K.supported(real, fake, 9)
    for got in (_prdc(wide[:, ::2], fake, 3), _prdc(real.double(), fake.double(), 3)):
        for name in ("radii_real", "radii_fake", "hits_real", "hits_fake", "nearest_real", "nearest_fake", "tallies"):
            assert np.array_equal(got[name].cpu().numpy(), want[name]), name
        assert same(got, _prdc(real, fake, 3))
    want9 = oracle(real, fake, 9)
    got9 = _prdc(real, fake, 9)
    for name in ("radii_real", "radii_fake", "hits_real", "hits_fake", "nearest_real", "nearest_fake", "tallies"):
        assert np.array_equal(got9[name].cpu().numpy(), want9[name]), name


def test_half_features_equal_the_float32_call_on_the_widened_copy():
    real, fake = integer_features(T + 5, T + 2, 48, 7)
    real, fake = real + 0.5, fake * 0.25
    for dtype in (torch.float16, torch.bfloat16):
        r, f = real.to(dtype), fake.to(dtype)
        assert K.supported(r, f, 3)
        assert same(_prdc(r, f, 3), _prdc(r.float(), f.float(), 3))


# ----------------------------------------------------------------------------- float data
def float_bounds(real, fake):
    """``e(a, b) = 2 eps sum_k |a_k| |b_k|`` with ``eps = min(D 2^-24, 4e-7)`` bounds the error of one
    squared distance: the norms are exact to FP64 rounding, the factor 2 is the one in front of the
    inner product, ``D 2^-24`` is the first-order bound of a k-ordered float32 fmaf chain (which
    the FP32-input MFMA is) and 4e-7 rounds up its measured 3.5e-7 for K <= 4096
    (tests/gpu/test_k20_kid.py).  Returns the three [rows, columns] matrices of ``e``: within the
    real set, within the generated set, and generated against real."""
    x, y = real.cpu().double().abs().numpy(), fake.cpu().double().abs().numpy()
    scale = 2.0 * min(real.shape[1] * 2.0**-24, 4e-7)
    return scale * (x @ x.T), scale * (y @ y.T), scale * (y @ x.T)


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("n,m,d", [(385, 257, 2048), (300, 280, 64), (200, 150, 33), (300, 300, 768)])
def test_random_features_inside_the_computed_bounds(n, m, d, k):
    """A k-th smallest value moves by no more than the largest error of the values it is chosen
    from, so a radius is within ``E_set = max e`` over its set and a nearest value within
    ``max e`` over the cross pairs; both are asserted at twice that.  A decision
    ``d2(a, b) <= rad2`` cannot differ from the oracle's when the oracle's margin exceeds
    ``2 (e(a, b) + E_set)``; rows all of whose decisions are settled must agree with the oracle
    exactly, the others are left out, and at most 5 % of either side may be.

    Measured on an MI355X (largest error of radii_real, radii_fake, nearest_real, nearest_fake
    against twice the bound; k = 3 / k = 5 where they differ):
      200 x 150 x 33    5.7e-6 / 4.1e-6, 5.5e-6 / 3.9e-6, 5.0e-6, 4.3e-6  against 2.5e-5, 2.8e-5, 2.3e-5, 2.3e-5
      300 x 280 x 64    1.6e-5 / 1.1e-5, 1.6e-5 / 1.5e-5, 1.3e-5, 1.2e-5  against 4.5e-5, 5.1e-5, 4.0e-5, 4.0e-5
      300 x 300 x 768   9.1e-5 / 1.0e-4, 1.1e-4 / 1.2e-4, 8.8e-5, 8.7e-5  against 4.4e-4, 4.7e-4, 3.6e-4, 3.6e-4
      385 x 257 x 2048  2.2e-4 / 2.3e-4, 2.8e-4 / 2.8e-4, 2.3e-4, 2.8e-4  against 1.2e-3, 1.2e-3, 9.3e-4, 9.3e-4
    The bounds are why the kernel adds its MFMA chains in chunks of 128 k: one float32 chain over
    all of D measured 4.6e-4 to 5.9e-4 at D = 768 and 1.9e-3 to 2.3e-3 at D = 2048, above them (a
    numpy emulation of one chain gives the same largest radius error, 2.2028414e-03; such a chain is
    off by up to 2.6e-6 of sum |a_k| |b_k| over these pairs, above the 4e-7 that K20's test measured
    on sums averaged over a subset).  In all eight cases every settled row has the oracle's hits and
    coverage decision, and the
    oracle leaves out at most 0.8 % of the rows of a side."""
    g = torch.Generator().manual_seed(n + d)
    real = torch.rand(n, d, generator=g).to(DEV)
    fake = (torch.rand(m, d, generator=g) + 0.02).to(DEV)
    want = oracle(real, fake, k)
    e_rr, e_ff, e_fr = float_bounds(real, fake)
    E_r, E_f, E_x = e_rr.max(), e_ff.max(), e_fr.max()
    got = _prdc(real, fake, k)
    out = {name: got[name].cpu().numpy() for name in NAMES}
    x, y = real.cpu().double().numpy(), fake.cpu().double().numpy()
    dfx = distances(y, x)  # [M, N]
    settled_fake = (np.abs(dfx - want["radii_real"][None, :]) > 2 * (e_fr + E_r)).all(axis=1)
    settled_real = (np.abs(dfx.T - want["radii_fake"][None, :]) > 2 * (e_fr.T + E_f)).all(axis=1)
    covered_settled = np.abs(want["nearest_real"] - want["radii_real"]) > 2 * (e_fr.max(axis=0) + E_r)
    covered = out["nearest_real"] <= out["radii_real"]
    errors = {name: (np.abs(out[name] - want[name]).max(), 2 * bound) for name, bound in
              (("radii_real", E_r), ("radii_fake", E_f), ("nearest_real", E_x), ("nearest_fake", E_x))}
    wrong_fake = int((out["hits_fake"] != want["hits_fake"])[settled_fake].sum())
    wrong_real = int((out["hits_real"] != want["hits_real"])[settled_real].sum())
    wrong_covered = int((covered != (want["nearest_real"] <= want["radii_real"]))[covered_settled].sum())
    # every figure first, then the assertions
    for name, (err, bound) in errors.items():
        print(f"N={n} M={m} D={d} k={k}: max |{name} - oracle| = {err:.3e}, bound {bound:.3e}")
    print(f"  rows left out: fake {1 - settled_fake.mean():.3%}, real {1 - settled_real.mean():.3%}, "
          f"coverage {1 - covered_settled.mean():.3%}; settled rows that differ: hits_fake {wrong_fake}, "
          f"hits_real {wrong_real}, covered {wrong_covered}; values {out['values']}")
    # from the oracle alone (no output of the kernel enters): at most 3 % with these seeds
    assert settled_fake.mean() >= 0.95 and settled_real.mean() >= 0.95 and covered_settled.mean() >= 0.95
    for name, (err, bound) in errors.items():
        assert err <= bound, name
    assert wrong_fake == 0 and wrong_real == 0 and wrong_covered == 0
    assert int(out["tallies"][3]) == int(covered.sum())
    # bit-identical from run to run
    assert same(_prdc(real, fake, k), got)


# ----------------------------------------------------------------------------- functional, class, compile
def test_functional_values_are_the_tallies_divided_in_numpy():
    g = torch.Generator().manual_seed(21)
    real = torch.rand(300, 64, generator=g).to(DEV)
    fake = (0.9 * torch.rand(260, 64, generator=g) + 0.05).to(DEV)
    for k in (3, 5):
        tallies = _prdc(real, fake, k)["tallies"].cpu().numpy()
        want = values_of(tallies, 300, 260, k)
        p, r = improved_precision_recall(real, fake, k=k)
        d, c = density_coverage(real, fake, k=k)
        for v in (p, r, d, c):
            assert v.dtype == torch.float32 and v.shape == () and v.device == DEV
        assert [float(p), float(r), float(d), float(c)] == [float(v) for v in want]
        assert 0 < tallies[0] < 260 and 0 < tallies[1] < 300  # neither end of the scale
    assert float(improved_precision_recall(real, fake)[0]) == float(improved_precision_recall(real, fake, k=3)[0])
    assert float(density_coverage(real, fake)[0]) == float(density_coverage(real, fake, k=5)[0])


@pytest.mark.parametrize("cls,fn", [(ImprovedPrecisionRecall, improved_precision_recall),
                                    (DensityCoverage, density_coverage)])
def test_class_on_device_equals_the_functional_on_the_concatenation(cls, fn):
    g = torch.Generator().manual_seed(22)
    real = torch.rand(200, 32, generator=g).to(DEV)
    fake = (0.9 * torch.rand(170, 32, generator=g) + 0.05).to(DEV)

    def new():
        return cls(model=torch.nn.Identity(), feature_dim=32, device=DEV)

    m = new()
    for lo, hi in ((0, 1), (1, 130), (130, 200)):
        m.update_activations(real[lo:hi], True)
    for lo, hi in ((0, 100), (100, 170)):
        m.update_activations(fake[lo:hi].cpu(), False)  # moved to the metric's device
    got, want = m.compute(), fn(real, fake)
    assert got[0].device == DEV and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    again = m.compute()
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
    other = new().update_activations(real[:60], True).update_activations(fake, False)
    other.merge_state([new().update_activations(real[60:], True)])
    merged = other.compute()
    assert torch.equal(merged[0], got[0]) and torch.equal(merged[1], got[1])


def test_compiled_call_matches_eager():
    real, fake = integer_features(T + 9, T + 3, 64, 23)
    torch._dynamo.reset()
    fn = torch.compile(lambda r, f: K.prdc(r, f, 3), fullgraph=True)
    out = fn(real, fake)
    eager = check_exact(real, fake, 3)
    assert same(out, eager)
    # 16-bit features: the widening copy stays in the graph
    assert same(fn(real.half(), fake.bfloat16()), eager)
