"""The ATen form of ``_per_sample_binned_auroc`` (CPU tensors: searchsorted, a histogram of bins and
its suffix sums) against the literal FP64 oracle of tests/_binned_auroc_oracle.py, bit for bit (the
argument is in that module), on the cases the K4b kernel runs in tests/gpu/test_k4b_edges.py; and a
census of those cases, so that they cannot quietly stop reaching the comparisons they are there for."""

import pytest
import torch

from tests import _binned_auroc_oracle as O
from torcheval_amd.metrics.functional import multiclass_binned_auroc
from torcheval_amd.metrics.functional.classification.binned_auroc import _per_sample_binned_auroc

INF = float("inf")


def test_oracle_by_hand():
    """The oracle on the reference's docstring example and on rows small enough to check on paper."""
    x = torch.tensor([[0.1, 0.2, 0.1], [0.4, 0.2, 0.1], [0.6, 0.1, 0.2], [0.4, 0.2, 0.3], [0.6, 0.2, 0.4]])
    y = torch.tensor([0, 1, 2, 1, 0])
    assert O.per_sample_binned_auroc_fp64(x, y, torch.linspace(0, 1, 5)).tolist() == [0.5, 0.25, 0.25, 0.0, 1.0]
    thr = torch.tensor([0.0, 0.5, 1.0])
    rows = [
        # true score, rivals, value
        (1.0, [0.5, 0.0, -0.125], 1.0),  # two rivals at or above thr_0, both in lower bins
        (0.5, [0.5, 0.0, 1.0], 0.5),  # bins 2, 1, 3 against the true bin 2: (1 + 0.5) / 3
        (0.5, [0.75, 0.5, INF], 1 / 3),  # bins 2, 2, 3: (0 + 0.5 * 2) / 3
        (INF, [INF, 1.0, 0.0], 2 / 3),  # +inf is in the top bin with 1.0: (1 + 0.5 * 2) / 3
        (1.0, [INF, -INF, float("nan")], 0.5),  # one rival counts, in the true bin
        (-0.0, [0.0, 0.25, -0.125], 0.5),  # -0.0 >= 0: bin 1 with both counted rivals
        (float("nan"), [0.5, 0.5, 0.5], 0.5),  # tp_0 = 0
        (-0.125, [0.5, 0.5, 0.5], 0.5),  # tp_0 = 0
        (0.5, [-0.125, -INF, float("nan")], 0.5),  # fp_0 = 0
    ]
    x = torch.tensor([[r[0]] + r[1] for r in rows])
    want = torch.tensor([r[2] for r in rows], dtype=torch.float64).to(torch.float32)
    got = O.per_sample_binned_auroc_fp64(x, torch.zeros(len(rows), dtype=torch.int64), thr)
    assert got.dtype == torch.float32 and O.mismatches(got, want) == []
    # the same rows with the true class moved to the last column
    got = O.per_sample_binned_auroc_fp64(x.flip(1), torch.full((len(rows),), 3), thr)
    assert O.mismatches(got, want) == []


@pytest.mark.parametrize("c", O.WIDTHS)
def test_aten_form_matches_the_oracle_bit_for_bit(c):
    bad = []
    for case in O.cases_for(c):
        x, y, thr = case.tensors()
        want = O.per_sample_binned_auroc_fp64(x, y, thr)
        got = _per_sample_binned_auroc(x, y, c, thr)
        bad += O.describe(case.id, x, y, got, want)
    assert not bad, O.report(bad)


def test_public_function_on_cpu_and_its_macro_mean():
    case = O.cases_for(18)[-1]
    x, y, thr = case.tensors()
    want = O.per_sample_binned_auroc_fp64(x, y, thr)
    got, _ = multiclass_binned_auroc(x, y.long(), num_classes=18, threshold=thr, average=None)
    assert O.mismatches(got, want) == []
    mac, _ = multiclass_binned_auroc(x, y.long(), num_classes=18, threshold=thr)
    assert torch.equal(mac, want.mean())


def test_case_lists_name_every_arm_and_pattern():
    assert O.WIDTHS == (2, 3, 4, 5, 16, 17, 18, 32, 33, 64, 65, 128, 129, 256, 257, 515)
    for arm, widths in O.ARMS.items():
        for c in widths:
            need = (c + 3) // 4  # launch_sample_binned_auroc: the lanes a row needs
            g = "narrow" if c < 4 else next(f"g{g}" for g in (4, 8, 16, 32, 64) if need <= g or g == 64)
            assert g == arm, (c, g, arm)
    assert {c % 4 for c in O.WIDTHS} == {0, 1, 2, 3}
    for c in O.WIDTHS:
        cases = O.cases_for(c)
        assert {k.n for k in cases} == set(O.NS) and {k.thr for k in cases} == set(O.THRESHOLD_SETS)
        pairs = {(k.pattern, k.label_dtype) for k in cases}
        assert pairs >= {(p, d) for p in O.PATTERNS for d in O.LABEL_DTYPES}, c
        for n in O.NS:
            assert {k.pattern for k in cases if k.n == n} == set(O.PATTERNS), (c, n)
            assert {k.label_dtype for k in cases if k.n == n} == {d for _, d in pairs}, (c, n)
        for k in cases:
            _, y, _ = k.tensors()
            assert y.dtype == k.label_dtype and int(y.min()) >= 0 and int(y.max()) < c
            if k.pattern != "random":
                assert (y == {"first": 0, "last": c - 1, "tail": max(c - 4, 0)}[k.pattern]).all()
    assert any(k.label_dtype == torch.int16 for k in O.cases_for(O.SMALL_LABEL_WIDTH))


def test_census_of_the_cases():
    """How many samples of the whole case set reach each comparison's edge.  The count of 20 is a
    condition on the inputs: a generator change that falls below it has to be mended there."""
    count = dict.fromkeys((
        "true score equals a threshold", "rival equals thr[b_true - 1]", "rival equals thr[b_true]",
        "rival equals thr[0]", "true score is +inf", "rival is +inf while b_true == T", "true score is NaN",
        "b_true == 0", "no rival at or above thr[0]", "true score is -0.0 against thr[0] == 0",
        "true score equals the last threshold"), 0)
    for case in O.all_cases():
        x, y, thr = case.tensors()
        n, c = x.shape
        T = thr.numel()
        true = torch.arange(c).view(1, -1) == y.long().view(-1, 1)
        xt = x[true].view(n, 1)
        b = (xt >= thr.view(1, -1)).sum(1)  # b_true, counted: thresholds ascending, NaN in bin 0
        lo = thr[(b - 1).clamp(min=0)].view(n, 1)  # thr[b_true - 1] where b_true >= 1
        hi = thr[b.clamp(max=T - 1)].view(n, 1)  # thr[b_true] where b_true < T
        rival = ~true
        count["true score equals a threshold"] += int((xt == thr.view(1, -1)).any(1).sum())
        count["rival equals thr[b_true - 1]"] += int((((x == lo) & rival).any(1) & (b >= 1)).sum())
        count["rival equals thr[b_true]"] += int((((x == hi) & rival).any(1) & (b < T)).sum())
        count["rival equals thr[0]"] += int(((x == thr[0]) & rival).any(1).sum())
        count["true score is +inf"] += int((xt == INF).sum())
        count["rival is +inf while b_true == T"] += int((((x == INF) & rival).any(1) & (b == T)).sum())
        count["true score is NaN"] += int(torch.isnan(xt).sum())
        count["b_true == 0"] += int((b == 0).sum())
        count["no rival at or above thr[0]"] += int((((x >= thr[0]) & rival).sum(1) == 0).sum())
        neg0 = (xt == 0) & torch.signbit(xt)
        count["true score is -0.0 against thr[0] == 0"] += int(neg0.sum()) if float(thr[0]) == 0.0 else 0
        count["true score equals the last threshold"] += int((xt == thr[-1]).sum())
    assert all(v >= 20 for v in count.values()), count
