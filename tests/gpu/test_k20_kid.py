"""K20 (csrc/kernels/kid.hip) on the device: the Kernel Inception Distance against an independent
numpy oracle written here.

The sharp tests use exact data: integer features in [0, 4) as float32, ``gamma = 2^-p``, ``coef = 1``.
Then ``k 2^(p degree) = (d + 2^p)^degree`` is an integer, the three sums are computed in integers
and asserted below 2^53, and every product and partial sum of the kernel is representable, so its
sums must equal them exactly in any summation order: one masked-in padding element, one diagonal
element or one wrong weight changes the result.  Random float32 data is compared under a bound
computed from the data (docstring of ``float_tolerance``).
"""

import numpy as np
import pytest
import torch

from torcheval_amd.metrics import KernelInceptionDistance
from torcheval_amd.metrics.functional import kernel_inception_distance
from torcheval_amd.metrics.functional.image.kid import _draw, _kid_sums, _kid_values
from torcheval_amd.ops import kid as K

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
T = K.TILE
SIZES = [2, 3, 31, 32, 33, T - 1, T, T + 1, 2 * T + 1]
WIDTHS = [1, 3, 4, 31, 32, 33, 64, 100, 256]


# ----------------------------------------------------------------------------- oracles
def integer_sums(real, fake, idx_r, idx_f, degree, p):
    """The three sums times 2^(p degree), in integers (asserted below 2^53), as exact floats."""
    x, y = real.cpu().numpy().astype(np.int64), fake.cpu().numpy().astype(np.int64)
    ir, jf = idx_r.cpu().numpy(), idx_f.cpu().numpy()
    out = np.zeros((ir.shape[0], 3))
    for s in range(ir.shape[0]):
        gx, gy = x[ir[s]], y[jf[s]]
        for c, (a, b, off_diagonal) in enumerate(((gx, gx, True), (gy, gy, True), (gx, gy, False))):
            v = a @ b.T + (1 << p)
            assert int(v.max()) ** degree * v.size < 2**63  # so int64 holds every power and the sum
            k = v**degree
            if off_diagonal:
                np.fill_diagonal(k, 0)
            total = int(k.sum())
            assert 0 < total < 2**53
            out[s, c] = float(total) * 2.0 ** (-p * degree)  # exact: a power of two
    return out


def oracle_sums(real, fake, idx_r, idx_f, degree, gamma, coef):
    x, y = real.cpu().double().numpy(), fake.cpu().double().numpy()
    ir, jf = idx_r.cpu().numpy(), idx_f.cpu().numpy()
    out = np.zeros((ir.shape[0], 3))
    for s in range(ir.shape[0]):
        gx, gy = x[ir[s]], y[jf[s]]
        for c, (a, b, off_diagonal) in enumerate(((gx, gx, True), (gy, gy, True), (gx, gy, False))):
            v = gamma * (a @ b.T) + coef
            k = v.copy()
            for _ in range(degree - 1):
                k = k * v
            if off_diagonal:
                np.fill_diagonal(k, 0.0)
            out[s, c] = k.sum()
    return out


def oracle_values(sums, m):
    return (sums[:, 0] + sums[:, 1]) / (m * (m - 1)) - 2.0 * sums[:, 2] / (m * m)


def float_tolerance(real, fake, idx_r, idx_f, degree, gamma, coef):
    """``4 max_pairs[degree (|gamma| S + |coef|)^(degree - 1) |gamma| S] eps`` with
    ``S = sum |a| |b|`` and ``eps = min(D 2^-24, 4e-7)``: ``D 2^-24`` is the first-order bound of a
    k-ordered float32 fmaf chain (which the FP32-input MFMA is), 4e-7 rounds up its measured
    3.5e-7 for K <= 4096, the bracket is the derivative of the kernel function at the bound of its
    argument, and 4 covers the four terms of mmd2 at weight <= 1 each."""
    x, y = real.cpu().double().abs().numpy(), fake.cpu().double().abs().numpy()
    ir, jf = idx_r.cpu().numpy(), idx_f.cpu().numpy()
    eps = min(real.shape[1] * 2.0**-24, 4e-7)
    worst = 0.0
    for s in range(ir.shape[0]):
        gx, gy = x[ir[s]], y[jf[s]]
        for a, b in ((gx, gx), (gy, gy), (gx, gy)):
            sab = abs(gamma) * (a @ b.T)
            worst = max(worst, float((degree * (sab + abs(coef)) ** (degree - 1) * sab).max()))
    return 4.0 * worst * eps


# ----------------------------------------------------------------------------- data
def integer_features(n_r, n_f, d, seed):
    """Integers in [0, 4).  Row i of the real side is non-zero only in its first 1 + i d // n_r
    columns, so its norm grows with the row number and the rows are not exchangeable."""
    g = torch.Generator().manual_seed(seed)
    real = torch.randint(0, 4, (n_r, d), generator=g).float()
    real = real * (torch.arange(d)[None, :] <= (torch.arange(n_r)[:, None] * d) // n_r)
    fake = torch.randint(0, 4, (n_f, d), generator=g).float()
    return real.to(DEV), fake.to(DEV)


def random_indices(subsets, n, m, seed):
    """Independent rows, drawn with replacement: subsets share rows and a subset repeats some."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, n, (subsets, m), generator=g, dtype=torch.int32).to(DEV)


def power_of(d):
    return max(1, (d - 1).bit_length())  # gamma = 2^-p >= 1 / d


def check_exact(real, fake, idx_r, idx_f, degree, p):
    want = integer_sums(real, fake, idx_r, idx_f, degree, p)
    got = _kid_sums(real, fake, idx_r, idx_f, degree, 2.0**-p, 1.0)
    assert got.dtype == torch.float64 and got.device == DEV
    assert np.array_equal(got.cpu().numpy(), want), (got.cpu().numpy() - want)
    values = _kid_values(real, fake, idx_r, idx_f, degree, 2.0**-p, 1.0).cpu().numpy()
    np.testing.assert_allclose(values, oracle_values(want, idx_r.shape[1]), rtol=1e-12, atol=1e-11)


# ----------------------------------------------------------------------------- exact data
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("m", SIZES)
def test_exact_sums_at_every_tile_and_width_edge(m, d):
    """Every (m, D) pair: with gamma = 2^-ceil(log2 D) and degree 3 the largest possible sum is
    (9 D + 2^p)^3 m^2 <= 2560^3 * 257^2 = 1.1e15 < 2^53 at (256, 2 T + 1), so no pair is dropped."""
    real, fake = integer_features(m + 5, m + 2, d, 1000 * m + d)
    idx_r, idx_f = random_indices(3, m + 5, m, m + d), random_indices(3, m + 2, m, m + d + 1)
    check_exact(real, fake, idx_r, idx_f, 3, power_of(d))


@pytest.mark.parametrize("d,m,p", [(64, 129, 6), (256, 257, 8), (100, 33, 8)])
@pytest.mark.parametrize("subsets", [1, 3, 70])
def test_exact_sums_with_more_subsets_than_finish_waves(d, m, p, subsets):
    real, fake = integer_features(m + 40, m, d, d + m)
    # without replacement, as the functional draws them
    idx_r = _draw(subsets, m + 40, m, DEV, torch.Generator(device=DEV).manual_seed(subsets))
    idx_f = _draw(subsets, m, m, DEV, torch.Generator(device=DEV).manual_seed(subsets + 1))
    check_exact(real, fake, idx_r, idx_f, 3, p)


@pytest.mark.parametrize("degree", [1, 2, 4, 5])
def test_exact_sums_at_other_degrees(degree):
    real, fake = integer_features(T + 9, T + 3, 32, degree)
    idx_r, idx_f = random_indices(2, T + 9, T + 1, 7), random_indices(2, T + 3, T + 1, 8)
    check_exact(real, fake, idx_r, idx_f, degree, 5)


def test_duplicate_indices_are_positional():
    real, fake = integer_features(50, 60, 64, 3)
    idx_r = torch.tensor([[7] * 33, list(range(33))], dtype=torch.int32, device=DEV)
    idx_f = torch.tensor([[2, 2, 5] * 11, [59] * 33], dtype=torch.int32, device=DEV)
    check_exact(real, fake, idx_r, idx_f, 3, 6)


def test_coef_zero_degree_one_is_a_masked_gram_sum():
    real, fake = integer_features(T + 30, T + 20, 100, 4)
    idx_r, idx_f = random_indices(3, T + 30, T + 1, 9), random_indices(3, T + 20, T + 1, 10)
    x, y = real.cpu().numpy().astype(np.int64), fake.cpu().numpy().astype(np.int64)
    want = np.zeros((3, 3))
    for s in range(3):
        gx, gy = x[idx_r[s].cpu().numpy()], y[idx_f[s].cpu().numpy()]
        gxx, gyy = gx @ gx.T, gy @ gy.T
        want[s] = [gxx.sum() - np.trace(gxx), gyy.sum() - np.trace(gyy), (gx @ gy.T).sum()]
    got = _kid_sums(real, fake, idx_r, idx_f, 1, 1.0, 0.0)
    assert np.array_equal(got.cpu().numpy(), want)


def test_strided_and_misaligned_features_take_the_element_arm():
    m, d = T + 1, 64
    real, fake = integer_features(m + 5, m + 2, d, 5)
    idx_r, idx_f = random_indices(2, m + 5, m, 11), random_indices(2, m + 2, m, 12)
    want = _kid_sums(real, fake, idx_r, idx_f, 3, 2.0**-6, 1.0)
    check_exact(real, fake, idx_r, idx_f, 3, 6)
    # a column slice of a wider parent: row stride 200, still 16-byte aligned rows
    parent = torch.full((m + 5, 200), 3.0, device=DEV)
    parent[:, 8 : 8 + d] = real
    view = parent[:, 8 : 8 + d]
    assert view.stride() == (200, 1) and view.data_ptr() % 16 == 0
    assert torch.equal(_kid_sums(view, fake, idx_r, idx_f, 3, 2.0**-6, 1.0), want)
    # the same slice one column on: rows 4 bytes off a 16-byte boundary
    parent[:, 9 : 9 + d] = real
    view = parent[:, 9 : 9 + d]
    assert view.data_ptr() % 16 == 4
    assert torch.equal(_kid_sums(view, fake, idx_r, idx_f, 3, 2.0**-6, 1.0), want)
    # a contiguous tensor whose base is 4 bytes off, on the other side
    flat = torch.zeros((m + 2) * d + 1, device=DEV)
    off = flat[1:].view(m + 2, d)
    off.copy_(fake)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    assert torch.equal(_kid_sums(real, off, idx_r, idx_f, 3, 2.0**-6, 1.0), want)
    # a row stride that is no multiple of 4 floats
    parent = torch.zeros(m + 5, d + 3, device=DEV)
    parent[:, :d] = real
    assert torch.equal(_kid_sums(parent[:, :d], fake, idx_r, idx_f, 3, 2.0**-6, 1.0), want)


def test_non_unit_inner_stride_takes_the_aten_form():
    real, fake = integer_features(40, 40, 16, 6)
    idx_r, idx_f = random_indices(2, 40, 20, 13), random_indices(2, 40, 20, 14)
    wide = torch.zeros(40, 32, device=DEV)
    wide[:, ::2] = real
    assert not K.supported(wide[:, ::2], fake, idx_r, idx_f)
    assert K.supported(real, fake, idx_r, idx_f)
    got = _kid_sums(wide[:, ::2], fake, idx_r, idx_f, 3, 2.0**-4, 1.0)
    assert torch.equal(got, _kid_sums(real, fake, idx_r, idx_f, 3, 2.0**-4, 1.0))
    got = _kid_sums(real.double(), fake.double(), idx_r, idx_f, 3, 2.0**-4, 1.0)  # float64: ATen too
    assert np.array_equal(got.cpu().numpy(), integer_sums(real, fake, idx_r, idx_f, 3, 4))


def test_half_features_equal_the_float32_call_on_the_widened_copy():
    real, fake = integer_features(T + 5, T + 2, 48, 7)
    real, fake = real + 0.5, fake * 0.25
    idx_r, idx_f = random_indices(2, T + 5, T, 15), random_indices(2, T + 2, T, 16)
    for dtype in (torch.float16, torch.bfloat16):
        r, f = real.to(dtype), fake.to(dtype)
        assert K.supported(r, f, idx_r, idx_f)
        assert torch.equal(_kid_values(r, f, idx_r, idx_f, 3, 1 / 48, 1.0),
                           _kid_values(r.float(), f.float(), idx_r, idx_f, 3, 1 / 48, 1.0))


# ----------------------------------------------------------------------------- float data
@pytest.mark.parametrize("d,m,subsets", [(2048, 2 * T + 1, 2), (33, T + 1, 3), (768, 100, 5)])
@pytest.mark.parametrize("shifted", [False, True])
def test_random_features_inside_the_computed_bound(d, m, subsets, shifted):
    g = torch.Generator().manual_seed(d + m)
    real = torch.rand(m + 50, d, generator=g).to(DEV)
    fake = torch.rand(m + 20, d, generator=g)
    fake = (0.8 * fake + 0.3 if shifted else fake).to(DEV)
    idx_r = _draw(subsets, m + 50, m, DEV, torch.Generator(device=DEV).manual_seed(1))
    idx_f = _draw(subsets, m + 20, m, DEV, torch.Generator(device=DEV).manual_seed(2))
    gamma = 1.0 / d
    want = oracle_values(oracle_sums(real, fake, idx_r, idx_f, 3, gamma, 1.0), m)
    tol = float_tolerance(real, fake, idx_r, idx_f, 3, gamma, 1.0)
    a = _kid_values(real, fake, idx_r, idx_f, 3, gamma, 1.0)
    err = np.abs(a.cpu().numpy() - want).max()
    print(f"D={d} m={m} S={subsets} shifted={shifted}: max |mmd2 - oracle| = {err:.3e}, bound {tol:.3e}, "
          f"mmd2 = {want.mean():.4f}")
    assert err <= tol
    # bit-identical from run to run
    assert torch.equal(_kid_values(real, fake, idx_r, idx_f, 3, gamma, 1.0), a)
    assert torch.equal(_kid_sums(real, fake, idx_r, idx_f, 3, gamma, 1.0),
                       _kid_sums(real, fake, idx_r, idx_f, 3, gamma, 1.0))


# ----------------------------------------------------------------------------- functional, class, compile
@pytest.mark.parametrize("subsets", [1, 9])
def test_functional_mean_and_std_against_numpy_on_the_kernels_values(subsets):
    g = torch.Generator().manual_seed(21)
    real = torch.rand(300, 64, generator=g).to(DEV)
    fake = (0.8 * torch.rand(260, 64, generator=g) + 0.3).to(DEV)
    mean, std = kernel_inception_distance(real, fake, subsets=subsets, subset_size=T + 1,
                                          generator=torch.Generator(device=DEV).manual_seed(4))
    assert mean.dtype == torch.float32 and std.dtype == torch.float32 and mean.shape == () and std.shape == ()
    assert mean.device == DEV and std.device == DEV
    gen = torch.Generator(device=DEV).manual_seed(4)
    idx_r = _draw(subsets, 300, T + 1, DEV, gen)
    idx_f = _draw(subsets, 260, T + 1, DEV, gen)
    for idx, n in ((idx_r, 300), (idx_f, 260)):
        assert int(idx.min()) >= 0 and int(idx.max()) < n
        assert all(len(set(row)) == T + 1 for row in idx.tolist())
    values = _kid_values(real, fake, idx_r, idx_f, 3, 1 / 64, 1.0).cpu().numpy()
    assert float(mean) == pytest.approx(values.mean(), rel=2e-7)
    if subsets == 1:
        assert float(std) == 0.0
    else:
        assert float(std) == pytest.approx(values.std(ddof=0), rel=1e-6)


def test_class_on_device_equals_the_functional_on_the_concatenation():
    g = torch.Generator().manual_seed(22)
    real = torch.rand(200, 32, generator=g).to(DEV)
    fake = (0.8 * torch.rand(170, 32, generator=g) + 0.3).to(DEV)
    m = KernelInceptionDistance(model=torch.nn.Identity(), feature_dim=32, subsets=4, subset_size=T + 1, seed=9,
                                device=DEV)
    for lo, hi in ((0, 1), (1, 130), (130, 200)):
        m.update_activations(real[lo:hi], True)
    for lo, hi in ((0, 100), (100, 170)):
        m.update_activations(fake[lo:hi].cpu(), False)  # moved to the metric's device
    got = m.compute()
    want = kernel_inception_distance(real, fake, subsets=4, subset_size=T + 1,
                                     generator=torch.Generator(device=DEV).manual_seed(9))
    assert got[0].device == DEV and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    again = m.compute()
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
    other = KernelInceptionDistance(model=torch.nn.Identity(), feature_dim=32, subsets=4, subset_size=T + 1, seed=9,
                                    device=DEV)
    other.update_activations(real[:60], True).update_activations(fake, False)
    rest = KernelInceptionDistance(model=torch.nn.Identity(), feature_dim=32, subsets=4, subset_size=T + 1, seed=9,
                                   device=DEV).update_activations(real[60:], True)
    other.merge_state([rest])
    merged = other.compute()
    assert torch.equal(merged[0], got[0]) and torch.equal(merged[1], got[1])


def test_compiled_call_matches_eager():
    real, fake = integer_features(T + 9, T + 3, 64, 23)
    idx_r, idx_f = random_indices(3, T + 9, T + 1, 17), random_indices(3, T + 3, T + 1, 18)
    torch._dynamo.reset()
    fn = torch.compile(lambda r, f, i, j: K.kid(r, f, i, j, 3, 2.0**-6, 1.0), fullgraph=True)
    out, values, sums = fn(real, fake, idx_r, idx_f)
    e_out, e_values, e_sums = K.kid(real, fake, idx_r, idx_f, 3, 2.0**-6, 1.0)
    assert torch.equal(out, e_out) and torch.equal(values, e_values) and torch.equal(sums, e_sums)
    assert np.array_equal(sums.cpu().numpy(), integer_sums(real, fake, idx_r, idx_f, 3, 6))
    # 16-bit features: the widening copy stays in the graph
    out16 = fn(real.half(), fake.bfloat16(), idx_r, idx_f)[0]
    assert torch.equal(out16, e_out)
