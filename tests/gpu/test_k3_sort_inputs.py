"""K3a radix sort (csrc/kernels/radix.hip) on its hardest inputs, against
torch.sort(stable=True): continuous and clustered scores, a 40% tie group, seven-level scores,
NaN / +-0 / +-inf, scores crowded under 1.0, a constant row, a row whose strided sample is all one
value, payloads of every dtype, ascending order, and several rows - at 64k to 2M keys a row; then
the arms of the pass body that both sorts share: tile and wave edges, every payload instantiation
and 16-round tiles, on the onesweep and on the upsweep / downsweep sort."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _check(x: torch.Tensor, payload=None, kind: int = 0, ascending: bool = False) -> None:
    from torcheval_amd.ops import native

    xd = x.to(DEV)
    s = torch.empty_like(xd)
    idx = torch.empty(xd.shape, dtype=torch.int32, device=DEV)
    native().sort_desc(xd, s, idx, None if payload is None else payload.to(DEV), kind, ascending)
    ref_vals, ref_idx = torch.sort(x, dim=-1, descending=not ascending, stable=True)
    torch.testing.assert_close(s.cpu(), ref_vals, equal_nan=True, rtol=0, atol=0)
    got = idx.cpu().long()
    if kind == 0:
        assert torch.equal(got, ref_idx), "permutation differs from the stable reference"
    elif kind == 1:
        want = torch.gather(payload.float().expand(x.shape) if payload.dim() == 1 else payload.float(), 1, ref_idx)
        torch.testing.assert_close(idx.cpu().view(torch.float32), want, rtol=0, atol=0)
    else:
        want = torch.gather(payload.long().expand(x.shape) if payload.dim() == 1 else payload.long(), 1, ref_idx)
        assert torch.equal(got, want)


def _gen(kind: str, n: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    if kind == "uniform":
        return torch.rand(1, n, generator=g)
    if kind == "logits":
        return torch.randn(1, n, generator=g) * 3
    if kind == "sigmoid_confident":  # most scores crowd just below 1.0
        return torch.sigmoid(torch.randn(1, n, generator=g) * 3 + 6)
    if kind == "ties40":  # a 40% tie group: one digit run spanning hundreds of tiles
        x = torch.rand(1, n, generator=g)
        x[:, torch.rand(n, generator=g) < 0.4] = 0.5
        return x
    if kind == "levels":
        return torch.randint(0, 7, (1, n), generator=g).float() / 7
    if kind == "special":
        x = torch.rand(1, n, generator=g) * 2 - 1
        m = torch.rand(n, generator=g)
        x[:, m < 0.01] = float("nan")
        x[:, (m >= 0.01) & (m < 0.02)] = -0.0
        x[:, (m >= 0.02) & (m < 0.03)] = 0.0
        x[:, (m >= 0.03) & (m < 0.035)] = float("inf")
        x[:, (m >= 0.035) & (m < 0.04)] = float("-inf")
        return x
    if kind == "constant":
        return torch.full((1, n), 0.25)
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["uniform", "logits", "sigmoid_confident", "ties40", "levels", "special", "constant"])
@pytest.mark.parametrize("n", [65536, 1_000_000, 2_000_000])
def test_sort_matches_stable_sort(kind, n):
    _check(_gen(kind, n, n + len(kind)))


@pytest.mark.parametrize("n", [70_001, 1_000_000])
def test_payloads_and_ascending(n):
    g = torch.Generator().manual_seed(n)
    x = torch.rand(1, n, generator=g)
    x[:, ::97] = 0.5  # ties
    t = torch.randint(0, 2, (n,), generator=g)
    _check(x, t, 1)
    _check(x, t.bool(), 1)
    _check(x, t.float(), 1)
    _check(x, torch.randint(0, 5, (1, n), generator=g), 2)
    _check(x, ascending=True)
    _check(_gen("special", n, 3), ascending=True)


def test_multi_row():
    g = torch.Generator().manual_seed(5)
    x = torch.rand(4, 300_000, generator=g)
    x[1] = (x[1] * 10).floor() / 10
    x[2, ::3] = float("nan")
    _check(x)


def test_constant_strided_sample():
    # every strided sample position (i * n / 8192) holds 0.5 among otherwise distinct keys
    n = 1 << 20
    g = torch.Generator().manual_seed(9)
    x = torch.rand(1, n, generator=g)
    pos = (torch.arange(8192) * n) // 8192
    x[0, pos] = 0.5
    _check(x)
    t = torch.randint(0, 2, (n,), generator=g)
    _check(x, t, 1)


def test_binary_auroc_matches_cpu_on_hard_inputs():
    from torcheval_amd.metrics.functional import binary_auprc, binary_auroc

    g = torch.Generator().manual_seed(11)
    for kind in ("uniform", "ties40", "sigmoid_confident"):
        x = _gen(kind, 1_000_000, 21)[0]
        t = torch.randint(0, 2, x.shape, generator=g)
        for fn in (binary_auroc, binary_auprc):
            got = float(fn(x.to(DEV), t.to(DEV)))
            want = float(fn(x.double(), t))
            assert got == pytest.approx(want, abs=1e-6), (kind, fn.__name__)


# ---- the arms of the pass body that both sorts share: rows <= 8 (and <= 1024 tiles) take the
# onesweep sort, 9 rows the upsweep / downsweep sort; below 4 << 20 keys in all a tile is 2048 keys
# (8 rounds), from there 4096 keys (16 rounds)


def _mix(rows: int, n: int, seed: int) -> torch.Tensor:
    """Rows cycle through uniform scores, seven-level scores and a constant 0.25 (ties and the
    all-one-digit tile in every shape); NaN, +-0 and +-inf in row 0, NaN as the very last key."""
    g = torch.Generator().manual_seed(seed)
    x = torch.empty(rows, n)
    for r in range(rows):
        if r % 3 == 0:
            x[r] = torch.rand(n, generator=g)
        elif r % 3 == 1:
            x[r] = torch.randint(0, 7, (n,), generator=g).float() / 7
        else:
            x[r] = 0.25
    if n > 12:
        x[0, 3] = float("nan")
        x[0, 5] = -0.0
        x[0, 6] = 0.0
        x[0, 7] = float("inf")
        x[0, 8] = float("-inf")
        x[-1, n - 1] = float("nan")
    return x


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049, 4096, 67_589])
@pytest.mark.parametrize("rows", [2, 9])
def test_tile_and_wave_edges(rows, n):
    # 67_589 = 33 full 2048-key tiles + 5 keys: two groups of tiles and a tail tile, so the
    # full-tile write-out, the tail write-out and the group prefix in one sort
    _check(_mix(rows, n, 1000 * rows + n % 997))


_N_PAY = 4100  # two full 2048-key tiles and a 4-key tail


@pytest.mark.parametrize("dtype", [torch.float32, torch.int64, torch.int32, torch.uint8, torch.bool])
@pytest.mark.parametrize("rows", [2, 9])
def test_target_payload_every_dtype(rows, dtype):
    g = torch.Generator().manual_seed(31 + rows)
    x = _mix(rows, _N_PAY, 40 + rows)
    t = torch.randint(0, 2, (_N_PAY,), generator=g)
    _check(x, t.float() * 0.75 if dtype == torch.float32 else t.to(dtype), 1)
    if dtype == torch.uint8:  # one dtype per kind also as a [rows, n] payload
        _check(x, torch.randint(0, 2, (rows, _N_PAY), generator=g).to(dtype), 1)


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("rows", [2, 9])
def test_label_payload_every_dtype(rows, dtype):
    g = torch.Generator().manual_seed(57 + rows)
    x = _mix(rows, _N_PAY, 60 + rows)
    _check(x, torch.randint(0, 100, (_N_PAY,), generator=g).to(dtype), 2)
    if dtype == torch.int64:
        _check(x, torch.randint(0, 100, (rows, _N_PAY), generator=g).to(dtype), 2)


@pytest.mark.parametrize("rows,n,payload,kind,ascending", [
    (8, 524_288, None, 0, False),         # exactly 4 << 20 keys: 128 full 4096-key tiles a row
    (8, 524_289, torch.uint8, 1, False),  # a 1-key tail tile
    (9, 466_034, None, 0, False),
    (9, 466_034, torch.int64, 2, False),
    (9, 466_034, None, 0, True),
])
def test_sixteen_round_tiles(rows, n, payload, kind, ascending):
    assert rows * n >= 4 << 20
    g = torch.Generator().manual_seed(n + kind)
    x = _mix(rows, n, rows + n % 1009)
    p = None if payload is None else torch.randint(0, 2 if kind == 1 else 100, (n,), generator=g).to(payload)
    _check(x, p, kind, ascending)


def test_ascending_on_the_eight_round_legacy_sort():
    _check(_mix(9, 2049, 77), ascending=True)


def test_no_lookback_timeout_after_the_sorts_above():
    from torcheval_amd.ops import native

    assert native().sort_desc_timeouts(torch.empty(1, device=DEV), False) == 0
