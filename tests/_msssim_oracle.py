"""Multi-scale SSIM oracle: the definition of docs/parity.md in float64 plain torch on the CPU.

Tolerance (K12's rule): the same code evaluated in float32 (``values(..., dtype=torch.float32)``, which
shares nothing with the package) shows what float32 arithmetic of the definition costs on the very
inputs of a case; an implementation may sum in another order, so it gets 4 times that error plus
1e-6.  Inputs are correlated pairs (``y = x +`` small noise), which keep every level's
contrast-structure mean far from 0, where ``x^beta`` is ill-conditioned.
"""

import torch
import torch.nn.functional as F

BETAS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def terms(x, y, data_range=1.0, ks=11, sigma=1.5, k1=0.01, k2=0.03, betas=BETAS, dtype=torch.float64) -> torch.Tensor:
    """``[M, N, C]`` in ``dtype``: the mean of cs at the levels before the last, of ssim at the last."""
    x, y = x.to(dtype), y.to(dtype)
    c = x.shape[1]
    i = torch.arange(ks, dtype=torch.float64)
    g = torch.exp(-((i - (ks - 1) / 2) ** 2) / (2 * sigma**2))
    win = torch.outer(g / g.sum(), g / g.sum()).to(dtype).expand(c, 1, ks, ks).contiguous()
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    out = []
    for j in range(len(betas)):
        if j:
            x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
        mx, my = F.conv2d(x, win, groups=c), F.conv2d(y, win, groups=c)
        sxx = F.conv2d(x * x, win, groups=c) - mx * mx
        syy = F.conv2d(y * y, win, groups=c) - my * my
        sxy = F.conv2d(x * y, win, groups=c) - mx * my
        t = (2 * sxy + c2) / (sxx + syy + c2)
        if j == len(betas) - 1:
            t = t * (2 * mx * my + c1) / (mx * mx + my * my + c1)
        out.append(t.mean(dim=(2, 3)))
    return torch.stack(out)


def values(x, y, dtype=torch.float64, **kw) -> torch.Tensor:
    """Per-image values ``[N]`` in ``dtype``: the clamped terms to their exponents, the product per
    plane, the mean over the channels."""
    t = terms(x, y, dtype=dtype, **kw)
    return (t.clamp(min=0) ** torch.tensor(kw.get("betas", BETAS), dtype=dtype)[:, None, None]).prod(0).mean(1)


def oracle(x, y, **kw):
    """(float64 per-image values ``[N]``, the tolerance the float32 form earns on these inputs)."""
    want = values(x, y, **kw)
    return want, 4 * float((values(x, y, dtype=torch.float32, **kw).double() - want).abs().max()) + 1e-6


def images(shape, seed, kind="rand"):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g)
    if kind == "uint8":
        return (x * 255).round(), (x * 255 + 10 * torch.randn(shape, generator=g)).clamp(0, 255).round()
    return x, (x + 0.05 * torch.randn(shape, generator=g)).clamp(0, 1)


def check(got, x, y, reduction="none", **kw):
    want, tol = oracle(x, y, **kw)
    want = want.mean() if reduction == "mean" else want
    assert got.dtype == torch.float32 and got.shape == want.shape
    err = float((got.double().cpu() - want).abs().max())
    print(f"err {err:.3e} tol {tol:.3e}")
    assert err <= tol, (err, tol)
