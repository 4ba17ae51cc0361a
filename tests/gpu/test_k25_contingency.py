"""K25 (csrc/kernels/contingency.hip) on the device.

The count is integer work: every table is compared for exact equality with ``np.add.at``, under both
slice instantiations (forced through the wrapper's ``slice_size``).

The statistics and values run on hand-made int64 tables passed straight to the ops and are compared
with the oracle of tests/_contingency_oracle.py, whose docstring derives the bounds by counting
roundings (``U = 2^-53``): ``(k + 20) U S`` for a sum ``S`` of ``k`` terms ``x log x``, ``E(S) / N + 4 U log N`` for an
entropy, ``(E(S_n) + E(S_a) + E(S_b)) / N + 12 U log N`` (absolute) for MI, the propagated quotient bound for
NMI, AMI, homogeneity and completeness, ``4 U`` for Rand, ``8 U`` absolute for ARI (its numerator and
denominator are exact 128-bit integers on the device) and ``10 U`` for FMI; each doubled, because the
oracle is FP64 as well.  The exact pair sums must equal Python integers.

The expected mutual information is compared with the exact-rational oracle.  Its chunk starts carry
the device ``lgamma``'s error at the magnitude of ``lgamma(N + 1)``, a property of the device library,
so the bound is measured: the largest ``|EMI - oracle| / sum |term|`` observed on an MI355X over the
cases of ``EMI_CASES`` (tests/_contingency_oracle.py) was 9.93e-13, at the 2 x 2 case with N = 20000, where
``lgamma(N + 1)`` is 1.8e5; 3 x 70 at N = 6000 gave 2.1e-13 and the four small cases at most 4.2e-16
(profiles/clustering_indices_r39.json, ``emi_accuracy``).  The test asserts 4 times the largest, and per case never more than the model's ceiling
``64 U lgamma(N + 1)`` for nine ``lgamma`` values of a few ulp each.  Only ``test_expected_mutual_information``
holds the measured figure: the EMI and AMI entries of the values tests and of the end-to-end test are
held to the ceiling alone (``emi_bound`` of the oracle module).
"""

import math

import numpy as np
import pytest
import torch

from tests import _contingency_oracle as O
from torcheval_amd.metrics import clustering as MC
from torcheval_amd.metrics.functional.clustering import contingency as FC
from torcheval_amd.ops import contingency as K

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SLICES = (K.SLICE_SMALL, K.SLICE_LARGE)
EMI_MEASURED = 9.93e-13 # largest |EMI - oracle| / sum |term| observed (module docstring)
EMI_BOUND = 4 * EMI_MEASURED


def count(t, p, r, c, slice_size=0, table=None, err=None):
    assert K.supported(t, p, torch.zeros(r, c, dtype=torch.int64, device=DEV))
    return FC._contingency(t, p, r, c, slice_size=slice_size, err=err, table=table)


def check_count(t, p, r, c, slice_size):
    got = count(t, p, r, c, slice_size)
    assert got.dtype == torch.int64 and got.shape == (r, c) and got.device == DEV
    want = O.table_of(t.cpu().numpy(), p.cpu().numpy(), r, c)
    assert np.array_equal(got.cpu().numpy(), want)
    return got


def labels(n, r, c, seed, dtype=torch.int64):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, r, (n,), generator=g).to(dtype).to(DEV),
            torch.randint(0, c, (n,), generator=g).to(dtype).to(DEV))


# ----------------------------------------------------------------------------- count
@pytest.mark.parametrize("slice_size", SLICES)
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 16 * K.BLOCK_LARGE + 3])
def test_count_small_table(n, dtype, slice_size):
    t, p = labels(n, 3, 5, n, dtype)
    check_count(t, p, 3, 5, slice_size)  # 3 x 5: a transposed index shows


@pytest.mark.parametrize("slice_size", SLICES)
def test_count_mixed_dtypes_and_unaligned_heads(slice_size):
    n = 4 * K.BLOCK_LARGE + 7
    t, p = labels(n + 4, 3, 5, 3, torch.int32)
    assert t.data_ptr() % 16 == 0 and p.data_ptr() % 16 == 0
    # heads 4, 8 and 12 bytes past a 16-byte boundary, different for the two vectors
    for ot, op in ((1, 2), (2, 3), (3, 1), (0, 3), (1, 0)):
        a, b = t[ot:ot + n], p[op:op + n]
        assert a.data_ptr() % 16 == 4 * ot and b.data_ptr() % 16 == 4 * op
        check_count(a, b, 3, 5, slice_size)
    t, p = labels(n + 4, 3, 5, 4, torch.int64)
    for ot, op in ((1, 0), (0, 1), (1, 1)):
        check_count(t[ot:ot + n], p[op:op + n], 3, 5, slice_size)
    check_count(t[:n], p[:n].int(), 3, 5, slice_size)
    check_count(t[1:n].int(), p[1:n], 3, 5, slice_size)
    for m in (2, 3, 5, 6, 7):  # shorter than the head and one unit
        check_count(t[1:1 + m].int()[1:], p[1:m], 3, 5, slice_size)


@pytest.mark.parametrize("slice_size", SLICES)
def test_count_one_cell_two_cells_and_bad_labels(slice_size):
    n = 5000
    t, p = torch.full((n,), 2, device=DEV), torch.full((n,), 4, device=DEV)
    assert check_count(t, p, 3, 5, slice_size)[2, 4] == n  # the wave fold
    alt = torch.arange(n, device=DEV) % 2
    got = check_count(alt * 2, 4 - alt * 3, 3, 5, slice_size)  # cells (0, 4) and (2, 1)
    assert got[0, 4] == n // 2 and got[2, 1] == n // 2
    t, p = labels(n, 3, 5, 9)
    t[17], p[4001] = -1, 5  # -1 in labels_true, C in labels_pred
    t[n - 1] = 3            # R, in the scalar tail
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = count(t, p, 3, 5, slice_size, err=err)
    assert err.item() == 1 and got.sum() == n - 3
    assert np.array_equal(got.cpu().numpy(), O.table_of(t.cpu().numpy(), p.cpu().numpy(), 3, 5))
    err.zero_()
    count(*labels(n, 3, 5, 10), 3, 5, slice_size, err=err)
    assert err.item() == 0
    # int32 labels that would wrap a 32-bit cell index are compared in 64-bit
    big = torch.tensor([2**31 - 1, 0, -(2**31)], dtype=torch.int32, device=DEV)
    got = count(big, torch.zeros(3, dtype=torch.int32, device=DEV), 3, 5, slice_size, err=err)
    assert err.item() == 1 and got.sum() == 1 and got[0, 0] == 1


@pytest.mark.parametrize("slice_size", SLICES)
@pytest.mark.parametrize("shape", [(17, 241), (3, 21847)])
def test_count_tables_of_several_slices(shape, slice_size):
    """17 x 241 is one cell more than the small slice; 3 x 21847 spans three large slices.  Samples land
    in the first and the last cell of every slice of either size, some cells several times."""
    r, c = shape
    cells = r * c
    assert cells in (K.SLICE_SMALL + 1, 2 * K.SLICE_LARGE + 5)
    edges = set()
    for s in SLICES:
        for lo in range(0, cells, s):
            edges |= {lo, min(lo + s, cells) - 1}
    g = torch.Generator().manual_seed(cells)
    cell = torch.cat([torch.tensor(sorted(edges)).repeat_interleave(3), torch.randint(0, cells, (20000,), generator=g)])
    cell = cell[torch.randperm(len(cell), generator=g)].to(DEV)
    got = check_count(cell // c, cell % c, r, c, slice_size)
    flat = got.reshape(-1)
    assert all(int(flat[e]) >= 3 for e in edges)
    again = count(cell // c, cell % c, r, c, slice_size, table=got)  # a second update accumulates
    assert again is got and np.array_equal(got.cpu().numpy(), 2 * O.table_of((cell // c).cpu(), (cell % c).cpu(), r, c))


def test_count_past_the_float32_integers():
    n = 2**24 + 2
    z = torch.zeros(n, dtype=torch.int32, device=DEV)
    for slice_size in SLICES:
        got = count(z, z, 2, 2, slice_size)
        assert got.tolist() == [[n, 0], [0, 0]]


# ----------------------------------------------------------------------------- statistics and values
def check_values(table, emi=True):
    """Statistics and values of a hand-made table against the oracle; returns the values."""
    table = np.asarray(table, dtype=np.int64)
    r, c = table.shape
    dev_table = torch.from_numpy(table).to(DEV)
    assert K.supported_table(dev_table)
    stats = K.contingency_stats(dev_table)
    m = [int(v) for v in stats["marginals"].cpu().numpy().astype(np.uint64)]
    P, Pa, Pb, N = O.pair_sums(table)
    assert m[:r] == [int(v) for v in table.sum(1)] and m[r:r + c] == [int(v) for v in table.sum(0)]
    assert m[r + c:] == [P, Pa, Pb, N, int((table.sum(1) > 0).sum()), int((table.sum(0) > 0).sum())]
    values, total = K.contingency_values(dev_table, emi)
    assert int(total) == N and values.dtype == torch.float64 and values.shape == (K.VALUES,)
    got = values.cpu().numpy()
    exact = None
    if emi and N > 0:
        e, mag = O.emi_oracle([int(v) for v in table.sum(1)], [int(v) for v in table.sum(0)])
        exact = (e, O.emi_bound(N, mag))
    want, bound = O.values_oracle(table, exact)
    for name, at in K.INDEX.items():
        ws, bs = want[name], bound[name]
        ws, bs = (ws, bs) if isinstance(ws, list) else ([ws], [bs])
        for k, (w, b) in enumerate(zip(ws, bs)):
            print(f"{name}[{k}] got {got[at + k]!r} want {w!r} bound {2 * b:.3e}")
            if math.isnan(w):
                assert math.isnan(got[at + k]), (name, k)
            else:
                assert abs(got[at + k] - w) <= 2 * b, (name, k, got[at + k], w, b)
    return got


@pytest.mark.parametrize("table", [
    [[5]],
    [[1, 2, 3, 4, 5, 6, 7]],
    [[1], [2], [3], [4], [5], [6], [7]],
    [[3, 0, 1, 0, 2], [0, 0, 4, 0, 1], [0, 0, 0, 0, 0], [5, 0, 0, 0, 7]],   # a zero row, zero columns
    [[4, 6], [6, 9]],                                                        # independent: ARI and MI 0
    [[40, 60, 1], [60, 91, 2]],                                              # ARI and MI near 0
    [[9, 0, 0], [0, 7, 0], [0, 0, 3]],                                       # a perfect match
    [[1, 1, 1, 1, 1, 1, 1]],                                                 # one cluster against singletons
    [[1], [1], [1]],
], ids=lambda t: f"{len(t)}x{len(t[0])}-{sum(map(sum, t))}")
def test_values_of_small_tables(table):
    check_values(table)


def test_values_of_large_counts():
    one = 2**31 - 1
    got = check_values([[one]], emi=False)
    assert got[K.INDEX["rand"]] == 1.0 and got[K.INDEX["adjusted_rand"]] == 1.0
    check_values([[0, 0, 0], [0, one, 0], [0, 0, 0]], emi=False)
    table = [[2**31, 2**30], [2**29, 2**29 - 1]]
    assert sum(map(sum, table)) == 2**32 - 1
    check_values(table, emi=False)  # its pair sums equal Python integers exactly
    wide = np.arange(1, 1 + 70 * 300, dtype=np.int64).reshape(70, 300) % 977  # several blocks, a ragged last segment
    check_values(wide, emi=False)


def test_degenerate_conventions():
    idx = K.INDEX
    v = check_values([[5]])
    assert v[idx["adjusted_rand"]] == 1.0 and (v[idx["normalized_mutual_info"]:idx["normalized_mutual_info"] + 4] == 1.0).all()
    assert (v[idx["adjusted_mutual_info"]:idx["adjusted_mutual_info"] + 4] == 1.0).all()
    for table in ([[1, 1, 1, 1]], [[1], [1], [1], [1]]):
        v = check_values(table)
        assert (v[idx["normalized_mutual_info"]:idx["normalized_mutual_info"] + 4] == 0.0).all()
        assert (v[idx["adjusted_mutual_info"]:idx["adjusted_mutual_info"] + 4] == 0.0).all()
        assert v[idx["fowlkes_mallows"]] == 0.0 and v[idx["mutual_info"]] == 0.0
    check_values([[4, 6], [6, 9]])  # MI 0 up to its rounding: NMI 0 or that rounding over the normalizer
    v = check_values([[0, 0], [0, 0]])
    assert np.isnan(v).all()  # N = 0
    v = check_values([[1, 0], [0, 0]])  # N = 1: no pair
    assert v[idx["rand"]] == 1.0 and v[idx["fowlkes_mallows"]] == 0.0


# ----------------------------------------------------------------------------- expected mutual information
def device_emi(a, b):
    table = torch.from_numpy(O.fill(a, b)).to(DEV)
    stats = K.contingency_stats(table)
    return K.contingency_emi(stats, len(a), len(b)).sum(dim=1).tolist()


@pytest.mark.parametrize("key", sorted(O.EMI_CASES))
def test_expected_mutual_information(key):
    a, b = O.EMI_CASES[key]
    assert sum(a) == sum(b) and min(b) >= 0
    n = sum(a)
    want, mag = O.emi_oracle(a, b)
    got, got_mag = device_emi(a, b)
    ceiling = 64 * O.U * math.lgamma(n + 1)
    ratio = abs(got - want) / mag if mag > 0 else float(got != want)
    print(f"EMI {key}: N {n} got {got!r} want {want!r} sum|term| {mag!r} ratio {ratio:.3e} ceiling {ceiling:.3e}")
    assert EMI_BOUND <= 64 * O.U * math.lgamma(20001)
    assert abs(got - want) <= min(EMI_BOUND, ceiling) * mag
    # the kernel's own sum of |term| (the benchmark's yardstick): no term cancels in it, so the
    # measured figure above says nothing about it and it is held to the model's ceiling
    assert abs(got_mag - mag) <= (ceiling + 8 * O.U) * mag


# ----------------------------------------------------------------------------- determinism and end to end
def test_bit_identical_runs_and_slices():
    t, p = labels(50000, 17, 241, 5)
    tables = [count(t, p, 17, 241, s) for s in SLICES for _ in range(2)]
    assert all(torch.equal(tables[0], x) for x in tables[1:])
    outs = [K.contingency_values(x)[0] for x in tables[:1] * 2 + tables[2:3]]
    assert all(torch.equal(outs[0].view(torch.int64), o.view(torch.int64)) for o in outs[1:])
    e = [K.contingency_emi(K.contingency_stats(tables[0]), 17, 241) for _ in range(2)]
    assert torch.equal(e[0].view(torch.int64), e[1].view(torch.int64))


@pytest.mark.parametrize("name", ["RandScore", "AdjustedRandScore", "MutualInfoScore", "NormalizedMutualInfoScore",
                                  "AdjustedMutualInfoScore", "HomogeneityScore", "CompletenessScore", "VMeasureScore",
                                  "FowlkesMallowsScore"])
def test_class_on_the_device_equals_the_class_on_cpu_copies(name):
    r, c = 7, 5
    t, p = labels(3000, r, c, 21)
    cls = getattr(MC, name)
    gpu = cls(r, c, device=DEV).update(t[:1000], p[:1000]).update(t[1000:].int(), p[1000:].int())
    cpu = cls(r, c).update(t.cpu(), p.cpu())
    assert gpu.contingency.device == DEV and torch.equal(gpu.contingency.cpu(), cpu.contingency)
    table = cpu.contingency.numpy()
    e, mag = O.emi_oracle([int(v) for v in table.sum(1)], [int(v) for v in table.sum(0)])
    _, bound = O.values_oracle(table, (e, O.emi_bound(3000, mag)))
    got, want = gpu.compute(), cpu.compute()
    assert got.device == DEV and got.dtype == torch.float64 and got.dim() == 0
    key = {"VMeasureScore": None}.get(name, cls._name)
    b = 4 * (bound["homogeneity"] + bound["completeness"]) + 8 * O.U if key is None else bound[key]
    b = b[2] if isinstance(b, list) else b
    print(f"{name}: device {float(got)!r} cpu {float(want)!r} bound {2 * b:.3e}")
    assert abs(float(got) - float(want)) <= 2 * b
    # a bad label: counted nowhere, raised once at compute()
    gpu.update(torch.tensor([0, r], device=DEV), torch.tensor([0, 0], device=DEV))
    assert gpu.contingency.sum() == 3001
    with pytest.raises(ValueError, match="outside"):
        gpu.compute()
    assert torch.isfinite(gpu.compute())
    gpu.reset()
    assert math.isnan(float(gpu.compute()))


def test_bad_label_on_another_device_than_the_state():
    """The flag of an update whose labels are not on the state's device reaches the state's flag."""
    t, p = torch.tensor([0, 3, 1]), torch.tensor([0, 0, 1])  # 3 is outside [0, 3)
    on_gpu = MC.RandScore(3, 3, device=DEV).update(t, p)  # host labels, ROCm state
    on_cpu = MC.RandScore(3, 3).update(t.to(DEV), p.to(DEV))  # ROCm labels, host state
    for m in (on_gpu, on_cpu):
        assert m.contingency.sum() == 2
        with pytest.raises(ValueError, match="outside"):
            m.compute()
        assert float(m.compute()) == 1.0  # raised once
    moved = MC.RandScore(3, 3).update(t[:1], p[:1]).to(DEV)  # a state moved after construction
    moved.update(t.to(DEV), p.to(DEV))
    with pytest.raises(ValueError, match="outside"):
        moved.compute()


def test_compute_of_a_total_past_the_kernels_range_takes_the_aten_form():
    """A ROCm state whose total is 2^32 or more: compute() reads that bit with its flag and takes the
    ATen form, whose pair sums are FP64 there (bounds: pair_bounds_f64 of the oracle module)."""
    table = np.array([[2**32, 5], [3, 2**31]], dtype=np.int64)
    want, _ = O.values_oracle(table)
    bound = O.pair_bounds_f64(table)
    for cls, key in ((MC.RandScore, "rand"), (MC.AdjustedRandScore, "adjusted_rand"),
                     (MC.FowlkesMallowsScore, "fowlkes_mallows")):
        m = cls(2, 2, device=DEV)
        m.contingency.copy_(torch.from_numpy(table))
        got = m.compute()
        assert got.device == DEV and abs(float(got) - want[key]) <= 2 * bound[key], (key, float(got), want[key])

