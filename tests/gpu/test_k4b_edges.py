"""K4b (csrc/kernels/binned_auroc.hip) against the literal FP64 oracle of tests/_binned_auroc_oracle.py,
bit for bit (hipcc's float32 division is correctly rounded and the build passes no fast-math flag;
the rest of the argument is in that module), where scores equal thresholds and are infinite, NaN or
-0.0: both edges of every lane-group arm, the true class in the first, the last and the shifted tail
lane's first column, strided rows at every 4-B alignment, the second grid-stride trip, thresholds
searched in global memory, and the label error flag in the first, the last and a second-trip row."""

import pytest
import torch

from tests import _binned_auroc_oracle as O
from torcheval_amd.metrics.functional import multiclass_binned_auroc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LABEL_ERROR = "Class values must be smaller than num_classes"

# launch_g of the kernel file: 256 threads per block, 8 samples per lane group, at most 2048 blocks
K_BLOCK, K_U, K_GRID_CAP = 256, 8, 2048


def _first_trip_rows(n: int, g: int) -> int:
    """The rows the first trip of the ``s0`` loop covers with ``g`` lanes per sample."""
    groups = -(-n // K_U)
    grid = min(max(-(-groups // (K_BLOCK // g)), 1), K_GRID_CAP)
    return grid * (K_BLOCK // g) * K_U


def _per_sample(x: torch.Tensor, y: torch.Tensor, thr: torch.Tensor) -> torch.Tensor:
    got, thr_out = multiclass_binned_auroc(x.to(DEV), y.to(DEV), num_classes=x.shape[1], threshold=thr.to(DEV),
                                           average=None)
    assert got.dtype == torch.float32 and got.shape == (x.shape[0],) and thr_out.device.type == "cuda"
    return got.cpu()


@pytest.mark.parametrize("c", O.WIDTHS)
def test_shared_cases_match_the_oracle_bit_for_bit(c):
    bad = []
    for case in O.cases_for(c):
        x, y, thr = case.tensors()
        want = O.per_sample_binned_auroc_fp64(x, y, thr)
        bad += O.describe(case.id, x, y, _per_sample(x, y, thr), want)
    assert not bad, O.report(bad)


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("c", [3, 257])
def test_strided_rows_at_every_alignment(c, offset):
    """Columns ``offset : offset + c`` of a wider tensor: the row stride is no multiple of 4 and the
    base is off 16-B alignment.  The gaps hold 0.5, which counts at or above thr_0 if ever read."""
    n = 257
    key = f"strided-c{c}-o{offset}"
    x = O.grid_scores(n, c, key)
    wide = torch.full((n, c + 6), 0.5)
    wide[:, offset:offset + c] = x
    y = torch.randint(0, c, (n,), generator=torch.Generator().manual_seed(c + offset))
    y[:3] = torch.tensor([0, c - 1, max(c - 4, 0)])
    y = y.to(torch.int32 if offset == 2 else torch.int64)
    thr = O.thresholds("dup6")
    xd = wide.to(DEV)[:, offset:offset + c]
    assert xd.stride() == (c + 6, 1) and (c + 6) % 4 != 0 and xd.storage_offset() == offset
    got, _ = multiclass_binned_auroc(xd, y.to(DEV), num_classes=c, threshold=thr.to(DEV), average=None)
    bad = O.describe(key, x, y, got.cpu(), O.per_sample_binned_auroc_fp64(x, y, thr))
    assert not bad, O.report(bad)


LARGE_N, LARGE_C = 65545, 129


@pytest.fixture(scope="module")
def large():
    """The one large input: G = 64 lanes per sample, 2048 blocks x 4 groups x 8 samples = 65 536 rows
    in the first trip, so the last 9 rows take the second one, next to clamped duplicates."""
    assert _first_trip_rows(LARGE_N, 64) == 65536 == LARGE_N - 9
    x = O.grid_scores(LARGE_N, LARGE_C, "large")
    y = torch.randint(0, LARGE_C, (LARGE_N,), generator=torch.Generator().manual_seed(65545))
    y[-3:] = torch.tensor([0, LARGE_C - 1, LARGE_C - 4])
    thr = O.thresholds("dup6")
    return x, x.to(DEV), y, thr, O.per_sample_binned_auroc_fp64(x, y, thr)


def test_second_grid_stride_trip(large):
    x, xd, y, thr, want = large
    got, _ = multiclass_binned_auroc(xd, y.to(DEV), num_classes=LARGE_C, threshold=thr.to(DEV), average=None)
    bad = O.describe("large", x, y, got.cpu(), want)
    assert not bad, O.report(bad)
    assert len(set(want[-9:].tolist())) > 2  # the second-trip rows are no constant


@pytest.mark.parametrize("bad_label", [LARGE_C, -1])
def test_label_error_in_the_second_trip(large, bad_label):
    _, xd, y, thr, _ = large
    bad = y.clone()
    bad[LARGE_N - 4] = bad_label
    with pytest.raises(RuntimeError, match=LABEL_ERROR):
        multiclass_binned_auroc(xd, bad.to(DEV), num_classes=LARGE_C, threshold=thr.to(DEV), average=None)


@pytest.mark.parametrize("t", [4096, 4097])
def test_exact_hits_among_thresholds_searched_in_global_memory(t):
    """T = 4097 is past the LDS stage (4096, its last staged size).  Every score is a threshold or
    the float32 next to one, the first and the last threshold among them."""
    n, c = 257, 5
    g = torch.Generator().manual_seed(t)
    thr = torch.sort(torch.rand(t, generator=g))[0]
    idx = torch.randint(0, t, (n, c), generator=g)
    idx[:32] = torch.tensor([0, t - 1])[torch.randint(0, 2, (32, c), generator=g)]
    x = thr[idx]
    side = torch.randint(0, 3, (n, c), generator=g)
    x = torch.where(side == 1, torch.nextafter(x, torch.tensor(float("inf"))), x)
    x = torch.where(side == 2, torch.nextafter(x, torch.tensor(float("-inf"))), x)
    assert int((x.view(-1, 1) == thr.view(1, -1)).any(1).sum()) > n * c // 4
    y = torch.randint(0, c, (n,), generator=g)
    bad = O.describe(f"T{t}", x, y, _per_sample(x, y, thr), O.per_sample_binned_auroc_fp64(x, y, thr))
    assert not bad, O.report(bad)


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("c", [3, 5, 129])
def test_label_error_flag_in_the_first_and_the_last_row(c, dtype):
    """n = 9: one lane group holds row 8 and seven clamped copies of it, which must neither hide the
    flag nor raise it twice over a valid label."""
    thr = O.thresholds("lin9").to(DEV)
    for n in (1, 9):
        x = O.grid_scores(n, c, f"flag-{n}-{c}").to(DEV)
        y = torch.randint(0, c, (n,), generator=torch.Generator().manual_seed(n + c)).to(dtype)
        multiclass_binned_auroc(x, y.to(DEV), num_classes=c, threshold=thr, average=None)  # valid: no error
        for row in sorted({0, n - 1}):
            for value in (c, -1):
                bad = y.clone()
                bad[row] = value
                with pytest.raises(RuntimeError, match=LABEL_ERROR):
                    multiclass_binned_auroc(x, bad.to(DEV), num_classes=c, threshold=thr, average=None)
        multiclass_binned_auroc(x, y.to(DEV), num_classes=c, threshold=thr)  # and none is left behind


def test_macro_is_the_float32_mean_of_the_per_sample_values():
    case = next(k for k in O.cases_for(129) if k.n == 257 and k.thr == "dup6")
    x, y, thr = case.tensors()
    xd, yd, td = x.to(DEV), y.to(DEV), thr.to(DEV)
    per, _ = multiclass_binned_auroc(xd, yd, num_classes=129, threshold=td, average=None)
    mac, _ = multiclass_binned_auroc(xd, yd, num_classes=129, threshold=td)
    assert mac.dtype == torch.float32 and mac.shape == () and torch.equal(mac, per.mean())
    assert O.mismatches(per, O.per_sample_binned_auroc_fp64(x, y, thr)) == []
