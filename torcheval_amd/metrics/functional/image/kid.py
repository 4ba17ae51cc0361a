"""Kernel Inception Distance (Binkowski et al. 2018), functional API.

Not in the reference tree (docs/parity.md, "Not in the reference"): the unbiased polynomial-kernel
MMD^2 between real and generated features, averaged over random subsets.  ROCm float32 / float16 /
bfloat16 features run K20 (csrc/kernels/kid.hip): the three Gram blocks of every subset on FP32
MFMA with the kernel function, the mask and the sum applied in registers, two launches per call.
CPU tensors, float64 features and features whose inner stride is not 1 run the ATen form below,
which evaluates the definition in FP64, a bounded chunk of subsets at a time.
"""

from typing import Optional, Tuple

import torch

import torcheval_amd.ops as _ops
from torcheval_amd.ops import kid as _k20

__all__ = ["kernel_inception_distance"]

# the ATen form keeps its [chunk, m, max(m, D)] temporaries at or below this many elements
_ATEN_CHUNK_ELEMENTS = 1 << 24


def kernel_inception_distance(
    real_features: torch.Tensor,
    fake_features: torch.Tensor,
    *,
    subsets: int = 100,
    subset_size: int = 1000,
    degree: int = 3,
    gamma: Optional[float] = None,
    coef: float = 1.0,
    generator: Optional[torch.Generator] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Kernel Inception Distance of ``[n_r, D]`` real against ``[n_f, D]`` generated features.

    With ``k(a, b) = (gamma <a, b> + coef)^degree`` (the power by left-to-right repeated
    multiplication in FP64) and ``m = subset_size`` rows ``x`` of the real and ``y`` of the
    generated features::

        sxx = sum_{i != j} k(x_i, x_j)   syy = sum_{i != j} k(y_i, y_j)   sxy = sum_{i, j} k(x_i, y_j)
        mmd2 = (sxx + syy) / (m (m - 1)) - 2 sxy / m^2

    The result is the mean and the population standard deviation (``unbiased=False``, as
    torchmetrics) of ``mmd2`` over ``subsets`` subsets, whose rows are drawn uniformly without
    replacement, independently per side (the ``subset_size`` largest of one row of uniform numbers
    per subset, one batched call per side).  The draws are not those of torchmetrics, so values
    agree with it in distribution, not bit for bit.  Class version: ``KernelInceptionDistance``.

    Args:
        real_features, fake_features: ``[n, D]`` with the same ``D``; each ``n >= subset_size``.
        subsets: number of subsets, ``>= 1``.
        subset_size: rows per subset and side, ``>= 2``.
        degree: integer ``1 .. 16``.
        gamma: ``1 / D`` when ``None``.
        coef: the kernel's additive constant.
        generator: source of the draws, on the features' device; the global RNG when ``None``.

    Returns ``(mean, std)``, float32 scalars on the features' device.
    """
    _kid_param_check(subsets, subset_size, degree)
    _kid_input_check(real_features, fake_features, subset_size)
    if gamma is None:
        gamma = 1.0 / real_features.shape[1]
    if _ops.compiling():
        # no inference mode inside a traced graph (as spearman_corrcoef)
        return _kid_compute(real_features, fake_features, subsets, subset_size, degree, gamma, coef, generator)
    with torch.inference_mode():
        return _kid_compute(real_features, fake_features, subsets, subset_size, degree, gamma, coef, generator)


def _kid_param_check(subsets: int, subset_size: int, degree: int) -> None:
    if not isinstance(subsets, int) or subsets < 1:
        raise ValueError(f"`subsets` should be an integer greater than or equal to 1, but received {subsets}.")
    if not isinstance(subset_size, int) or subset_size < 2:
        raise ValueError(f"`subset_size` should be an integer greater than or equal to 2, but received {subset_size}.")
    if not isinstance(degree, int) or isinstance(degree, bool) or not 1 <= degree <= 16:
        raise ValueError(f"`degree` should be an integer in 1 .. 16, but received {degree}.")


def _kid_input_check(real: torch.Tensor, fake: torch.Tensor, subset_size: int) -> None:
    if real.dim() != 2 or fake.dim() != 2 or real.shape[1] != fake.shape[1] or real.shape[1] < 1:
        raise ValueError(
            "The features should be two-dimensional with the same, non-zero width, "
            f"got shapes {tuple(real.shape)} and {tuple(fake.shape)}."
        )
    if real.shape[0] < subset_size or fake.shape[0] < subset_size:
        raise ValueError(
            f"`subset_size` = {subset_size} needs at least that many rows on each side, "
            f"got {real.shape[0]} real and {fake.shape[0]} generated."
        )


def _draw(subsets: int, n: int, m: int, device: torch.device, generator: Optional[torch.Generator]) -> torch.Tensor:
    """int32 ``[subsets, m]``: per row ``m`` of ``n`` indices, uniform without replacement (the
    positions of the ``m`` largest of ``n`` uniform numbers); one batched call."""
    u = torch.rand(subsets, n, device=device, generator=generator)
    return torch.topk(u, m, dim=1, sorted=False).indices.to(torch.int32)


def _kid_compute(real, fake, subsets, m, degree, gamma, coef, generator) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean, std) of checked features."""
    idx_r = _draw(subsets, real.shape[0], m, real.device, generator)
    idx_f = _draw(subsets, fake.shape[0], m, fake.device, generator)
    if _k20.supported(real, fake, idx_r, idx_f):
        out = _k20.kid(real, fake, idx_r, idx_f, degree, gamma, coef)[0]
        return out[0], out[1]
    values = _mmd2(_kid_sums_aten(real, fake, idx_r, idx_f, degree, gamma, coef), m)
    return values.mean().to(torch.float32), values.std(unbiased=False).to(torch.float32)


def _kid_values(real, fake, idx_r, idx_f, degree: int, gamma: float, coef: float) -> torch.Tensor:
    """float64 ``[S]``: ``mmd2`` of the subsets that the ``[S, m]`` index tensors name, from
    whichever path the tensors take."""
    with torch.inference_mode():
        if _k20.supported(real, fake, idx_r, idx_f):
            return _k20.kid(real, fake, idx_r, idx_f, degree, gamma, coef)[1]
        return _mmd2(_kid_sums_aten(real, fake, idx_r, idx_f, degree, gamma, coef), idx_r.shape[1])


def _kid_sums(real, fake, idx_r, idx_f, degree: int, gamma: float, coef: float) -> torch.Tensor:
    """float64 ``[S, 3]``: ``(sxx, syy, sxy)`` per subset, from whichever path the tensors take."""
    with torch.inference_mode():
        if _k20.supported(real, fake, idx_r, idx_f):
            return _k20.kid(real, fake, idx_r, idx_f, degree, gamma, coef)[2]
        return _kid_sums_aten(real, fake, idx_r, idx_f, degree, gamma, coef)


def _mmd2(sums: torch.Tensor, m: int) -> torch.Tensor:
    sums = sums.double()
    return (sums[:, 0] + sums[:, 1]) / (m * (m - 1)) - 2.0 * sums[:, 2] / (m * m)


def _kid_sums_aten(real, fake, idx_r, idx_f, degree: int, gamma: float, coef: float,
                   dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """The definition in ATen, in ``dtype`` (FP64; benchmarks/bench_kid.py also times float32, the
    form torchmetrics runs): per chunk of subsets two gathers, three ``bmm`` Gram blocks, the
    power, a zeroed diagonal on XX and YY, and the sums."""
    x, y = real.to(dtype), fake.to(dtype)
    subsets, m = idx_r.shape
    chunk = max(1, _ATEN_CHUNK_ELEMENTS // (m * max(m, x.shape[1])))

    def block(a: torch.Tensor, b: torch.Tensor, off_diagonal: bool) -> torch.Tensor:
        v = torch.bmm(a, b.transpose(1, 2)) * gamma + coef
        p = v
        for _ in range(degree - 1):
            p = p * v
        if off_diagonal:
            p.diagonal(dim1=1, dim2=2).zero_()  # positional: a row named twice still pairs with itself
        return p.sum(dim=(1, 2))

    out = []
    for lo in range(0, subsets, chunk):
        gx = x[idx_r[lo : lo + chunk].long()]
        gy = y[idx_f[lo : lo + chunk].long()]
        out.append(torch.stack([block(gx, gx, True), block(gy, gy, True), block(gx, gy, False)], dim=1))
    return torch.cat(out)
