"""K2 (csrc/kernels/multilabel.hip) on the GPU: every dispatch arm of ``launch_kinds``, every
score and target dtype, each term of the vector-load guard, the second trip of the row loop, the
shared fold workspace, the dispatcher op and the two classes.

Every check is exact.  The oracle (tests/_k2_cases.py) is the documented top-k rule - value order
with -0.0 == +0.0, NaN above +inf, lowest index among equals - through a stable float64 sort, and
float64 counts by the formulas of ``_multilabel_update``; ATen's ``topk`` is no oracle under ties.
``multilabel_counts`` adds into destinations pre-filled with 3.0 and 5.0, and both are compared
with ``torch.equal`` to the oracle's integers.  That the fixtures tell the rule from the
signed-zero and highest-index rules is asserted on the CPU, in
tests/metrics/classification/test_k2_oracle.py.
"""

import pytest
import torch

from tests._k2_cases import (
    FIXTURES,
    N_ROWS,
    SCALAR_C,
    SCORE_DTYPES,
    TARGET_DTYPES,
    VEC_C,
    VIEW_C,
    all_counts,
    counts,
    fixture,
    k2_targets,
    ks_for,
    odd_targets,
    tie_free_rows,
    tie_rows,
    topk_arm,
    topk_pred,
    total,
)
from tests._threshold_edges import CRITERIA, dtype_id, edge_scores, oracle_pred
from torcheval_amd import metrics as M
from torcheval_amd.metrics import functional as F
from torcheval_amd.ops.classification import ML_CRITERIA, multilabel_counts, native_multilabel

pytestmark = pytest.mark.gpu
DEV = "cuda"
_dt_ids = dict(ids=dtype_id)
NAN = float("nan")


class _Batch:
    """Runs ``multilabel_counts`` into (num_correct, num_total) cells pre-filled with (3, 5) and
    compares all of them with the oracle's integers at once, naming the launches that differ."""

    FILL = (3.0, 5.0)

    def __init__(self):
        self._chunks, self._want, self._labels = [], [], []

    def run(self, xd, td, *, k, criteria, want, tot, label, threshold=0.5):
        j = len(self._want) % 256
        if j == 0:
            self._chunks.append(torch.tensor(self.FILL, device=DEV).repeat(256, 1))
        cell = self._chunks[-1][j]
        multilabel_counts(xd, td, threshold=threshold, k=k, criteria=criteria, num_correct=cell[0], num_total=cell[1])
        assert self.FILL[1] + tot < 2**24
        self._want.append((self.FILL[0] + want, self.FILL[1] + tot))
        self._labels.append(label)

    def check(self):
        got = torch.cat(self._chunks)[: len(self._want)].cpu()
        want = torch.tensor(self._want, dtype=torch.float64).float()
        if not torch.equal(got, want):
            bad = (got != want).any(dim=1).nonzero().flatten().tolist()
            lines = [f"  {self._labels[i]}: got {got[i].tolist()} want {want[i].tolist()}" for i in bad[:16]]
            raise AssertionError(
                f"{len(bad)} of {len(self._want)} launches differ (num_correct, num_total):\n" + "\n".join(lines)
            )


def _place(t: torch.Tensor, layout: str, fill) -> torch.Tensor:
    """The CPU matrix ``t`` [n, w] on the device in a given layout.  A view's parent holds
    ``fill`` elsewhere (NaN for scores: it would win every top-k if it were read).
    contig   its own allocation, row stride w
    pad1     columns [0, w) of a [n, w + 1] parent: aligned pointer, row stride w + 1
    coloffJ  columns [J, J + w) of a parent whose width is a multiple of 4: misaligned pointer
    rows2    every second row of a [2n, w] parent: aligned pointer, row stride 2w
    cols2    every second column of a [n, 2w] parent: column stride 2
    """
    n, w = t.shape
    if layout == "contig":
        return t.contiguous().to(DEV)
    if layout == "pad1":
        parent, view = (n, w + 1), (slice(None), slice(0, w))
    elif layout.startswith("coloff"):
        off = int(layout[len("coloff"):])
        parent, view = (n, (w + 7) // 4 * 4), (slice(None), slice(off, off + w))
    elif layout == "rows2":
        parent, view = (2 * n, w), (slice(None, None, 2), slice(None))
    elif layout == "cols2":
        parent, view = (n, 2 * w), (slice(None), slice(None, None, 2))
    else:
        raise ValueError(layout)
    p = torch.full(parent, fill, dtype=t.dtype)
    p[view] = t
    out = p.to(DEV)[view]
    assert out.shape == t.shape
    return out


def _is_vec(xd: torch.Tensor, td: torch.Tensor) -> bool:
    """The ``vec`` guard of ``launch_kinds``."""
    ta = min(4 * td.element_size(), 16)
    return (xd.shape[1] % 4 == 0 and xd.stride(0) % 4 == 0 and td.stride(0) % 4 == 0
            and xd.data_ptr() % (4 * xd.element_size()) == 0 and td.data_ptr() % ta == 0)


def _topk_launches(b, x, t, k, pred, x_layout="contig", t_layout="contig", label="", vec=None):
    xd, td = _place(x, x_layout, NAN), _place(t, t_layout, 1)
    if vec is not None:
        assert _is_vec(xd, td) == vec, f"{label}: the layout does not select the arm this case is for"
    want = all_counts(pred, t)
    for crit in CRITERIA:
        b.run(xd, td, k=k, criteria=crit, want=want[crit], tot=total(t, crit), label=f"{label} top-k k={k} {crit}")


def _threshold_launches(b, x, t, thr, pred, x_layout="contig", t_layout="contig", label="", vec=None):
    xd, td = _place(x, x_layout, NAN), _place(t, t_layout, 1)
    if vec is not None:
        assert _is_vec(xd, td) == vec, f"{label}: the layout does not select the arm this case is for"
    want = all_counts(pred, t)
    for crit in CRITERIA:
        b.run(xd, td, k=0, threshold=thr, criteria=crit, want=want[crit], tot=total(t, crit),
              label=f"{label} threshold {thr} {crit}")


def _threshold_case(dtype, n, c, thr, seed):
    x = edge_scores(dtype, thr, n * c, seed=seed).view(n, c)
    return x, oracle_pred(x, thr)


# ------------------------------------------------------------------ every top-k arm
def _arm_cases():
    for c in SCALAR_C:
        yield pytest.param(c, "contig", False, id=f"{topk_arm(c, False)}-c{c}")
    for c in VIEW_C:
        yield pytest.param(c, "coloff1", False, id=f"{topk_arm(c, False)}-c{c}-coloff1")
    for c in VEC_C:
        yield pytest.param(c, "contig", True, id=f"{topk_arm(c, True)}-c{c}")


@pytest.mark.parametrize("c, layout, vec", list(_arm_cases()))
@pytest.mark.parametrize("dtype", SCORE_DTYPES, **_dt_ids)
def test_topk_every_arm(dtype, c, layout, vec):
    b = _Batch()
    for k in ks_for(c):
        for kind in FIXTURES:
            x = fixture(kind, dtype, c, k)
            pred = topk_pred(x, k)
            t = k2_targets(pred, seed=c + k)
            _topk_launches(b, x, t, k, pred, layout, layout, label=kind, vec=vec)
    b.check()


# ------------------------------------------------------------------ every target dtype, both layouts
@pytest.mark.parametrize("c", [256, 257, 260, 2048])
@pytest.mark.parametrize("tdtype", TARGET_DTYPES, **_dt_ids)
def test_every_target_dtype(tdtype, c):
    families = [k2_targets] if tdtype == torch.bool else [k2_targets, odd_targets]
    b = _Batch()
    for dtype in (torch.float32, torch.bfloat16):
        for make in families:
            label = f"{dtype_id(dtype)} {make.__name__}"
            for k in (3, c // 2):
                x = fixture("tie", dtype, c, k)
                pred = topk_pred(x, k)
                _topk_launches(b, x, make(pred, seed=c + k, dtype=tdtype), k, pred, label=label, vec=c % 4 == 0)
            x, pred = _threshold_case(dtype, N_ROWS, c, 0.5, seed=c)
            _threshold_launches(b, x, make(pred, seed=c, dtype=tdtype), 0.5, pred, label=label, vec=c % 4 == 0)
    b.check()


# ------------------------------------------------------------------ each term of the vec guard alone
# (id, columns cut from c, score layout, target layout, target dtype, vec)
_GUARD = [
    ("c_not_multiple_of_4", 1, "pad1", "pad1", torch.int64, False),
    ("score_row_stride", 0, "pad1", "contig", torch.int64, False),
    ("target_row_stride", 0, "contig", "pad1", torch.int64, False),
    ("score_pointer_off1", 0, "coloff1", "contig", torch.int64, False),
    ("score_pointer_off2", 0, "coloff2", "contig", torch.int64, False),
    ("score_pointer_off3", 0, "coloff3", "contig", torch.int64, False),
    ("target_pointer_off1_uint8", 0, "contig", "coloff1", torch.uint8, False),
    ("target_pointer_off1_int64", 0, "contig", "coloff1", torch.int64, False),
    ("row_strided_all_terms_true", 0, "rows2", "rows2", torch.int64, True),
    ("row_strided_all_terms_true_uint8", 0, "rows2", "rows2", torch.uint8, True),
]


@pytest.mark.parametrize("name, cut, x_layout, t_layout, tdtype, vec", _GUARD, ids=[g[0] for g in _GUARD])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], **_dt_ids)
def test_vec_guard_terms(dtype, name, cut, x_layout, t_layout, tdtype, vec):
    b = _Batch()
    c = 256 - cut
    for k in (1, 3, 128):
        x = fixture("tie", dtype, 256, k)[:, :c]
        pred = topk_pred(x, k)
        _topk_launches(b, x, k2_targets(pred, seed=k, dtype=tdtype), k, pred, x_layout, t_layout, label=name, vec=vec)
    c = 1000 - cut
    x, pred = _threshold_case(dtype, N_ROWS, 1000, 0.5, seed=17)
    x, pred = x[:, :c], pred[:, :c]
    _threshold_launches(b, x, k2_targets(pred, seed=17, dtype=tdtype), 0.5, pred, x_layout, t_layout, label=name,
                        vec=vec)
    b.check()


def test_column_strided_view_takes_the_aten_path():
    # x[:, ::2] has no unit column stride: the functional must not hand it to K2, and ATen's
    # device topk is defined on tie-free rows
    c, k = 65, 3
    x = tie_free_rows(torch.float32, N_ROWS, c, seed=5)
    pred = topk_pred(x, k)
    t = k2_targets(pred, seed=5)
    xd, td = _place(x, "cols2", NAN), _place(t, "cols2", 1)
    assert xd.stride(1) == 2 and not native_multilabel(xd, td, k)
    for crit, want in all_counts(pred, t).items():
        got = F.topk_multilabel_accuracy(xd, td, criteria=crit, k=k).cpu()
        exp = torch.tensor(want, dtype=torch.float32) / torch.tensor(total(t, crit), dtype=torch.float32)
        assert torch.equal(got, exp), f"{crit}: got {got.item()!r} want {exp.item()!r}"


# ------------------------------------------------------------------ the row loop's second trip
@pytest.mark.parametrize("c, vec", [(8, True), (5, False)], ids=["c8-vectorised", "c5-scalar"])
def test_row_loop_second_trip(c, vec):
    # the grid is capped at 2048 blocks of 4 rows: rows 8192.. are a block's second iteration
    n = 8197
    b = _Batch()
    for k in (2, c):
        x = tie_rows(torch.float32, n, c, k, seed=c + k)
        pred = topk_pred(x, k)
        t = k2_targets(pred, seed=c + k)
        for crit in CRITERIA:  # rows 8192 and 8196 equal the prediction: the second trip counts
            assert counts(pred[8192:], t[8192:], crit) > 0
        _topk_launches(b, x, t, k, pred, label=f"n={n}", vec=vec)
    x = tie_rows(torch.float32, n, c, 1, seed=c)
    pred = oracle_pred(x, 1.0)
    t = k2_targets(pred, seed=c)
    for crit in CRITERIA:
        assert counts(pred[8192:], t[8192:], crit) > 0
    _threshold_launches(b, x, t, 1.0, pred, label=f"n={n}", vec=vec)
    b.check()


# ------------------------------------------------------------------ the shared, self-cleaning fold
def _fold_sequence(ns):
    """K2 launches of changing grid size into ONE num_correct on the current stream, alternating
    threshold and top-k, with a K1 (MulticlassAccuracy) update + compute between them: K1 and K2
    share one fold workspace per (device, stream).  Every running sum is checked."""
    c, k = 12, 3
    cases = []
    for i, n in enumerate(ns):  # inputs first: the launches then follow each other closely
        crit = CRITERIA[i % len(CRITERIA)]
        x = tie_rows(torch.float32, n, c, k, seed=100 + i)
        pred = topk_pred(x, k) if i % 2 else oracle_pred(x, 1.0)
        t = k2_targets(pred, seed=100 + i)
        g = torch.Generator().manual_seed(200 + i)
        xm, ym = torch.rand(n, 10, generator=g), torch.randint(0, 10, (n,), generator=g)
        cases.append((n, crit, k if i % 2 else 0, x.to(DEV), t.to(DEV), counts(pred, t, crit), total(t, crit),
                      xm.to(DEV), ym.to(DEV), int((xm.argmax(dim=1) == ym).sum())))
    nc, nt = torch.zeros((), device=DEV), torch.zeros((), device=DEV)
    acc = M.MulticlassAccuracy(device=torch.device(DEV))
    run_c = run_t = run_mc = run_mt = 0
    for n, crit, kk, xd, td, want, tot, xm, ym, mc in cases:
        multilabel_counts(xd, td, threshold=1.0, k=kk, criteria=crit, num_correct=nc, num_total=nt)
        run_c, run_t = run_c + want, run_t + tot
        got = torch.stack([nc, nt]).cpu()
        assert torch.equal(got, torch.tensor([float(run_c), float(run_t)])), (
            f"after n={n} k={kk} {crit}: got {got.tolist()} want {[run_c, run_t]}")
        acc.update(xm, ym)
        run_mc, run_mt = run_mc + mc, run_mt + n
        ratio = acc.compute().cpu()
        got = torch.stack([acc.num_correct.reshape(()), acc.num_total.reshape(())]).cpu()
        assert torch.equal(got, torch.tensor([float(run_mc), float(run_mt)])), (
            f"MulticlassAccuracy after n={n}: got {got.tolist()} want {[run_mc, run_mt]}")
        torch.testing.assert_close(ratio, torch.tensor(run_mc / run_mt, dtype=torch.float32))


def test_fold_workspace_is_self_cleaning():
    _fold_sequence([1, 4, 5, 255, 256, 257, 260, 8192, 8197, 3])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _fold_sequence([5, 8197, 1, 260])
    side.synchronize()
    _fold_sequence([3, 257])  # and the first stream's workspace is as it was left


# ------------------------------------------------------------------ dispatcher op == pybind entry
@pytest.mark.parametrize("k", [0, 3], ids=["threshold", "topk"])
def test_dispatcher_op_matches_pybind_entry(k):
    c = 260
    x = fixture("tie", torch.bfloat16, c, max(k, 1))
    pred = topk_pred(x, k) if k else oracle_pred(x, 1.0)
    t = k2_targets(pred, seed=c, dtype=torch.int32)
    xd, td = x.to(DEV), t.to(DEV)
    for crit in CRITERIA:
        a, b = torch.tensor([3.0, 5.0], device=DEV), torch.tensor([3.0, 5.0], device=DEV)
        multilabel_counts(xd, td, threshold=1.0, k=k, criteria=crit, num_correct=a[0], num_total=a[1])
        torch.ops.torcheval_amd.multilabel_counts(xd, td, 1.0, k, ML_CRITERIA[crit], b[0], b[1],
                                                  float(total(t, crit)))
        want = torch.tensor([3.0 + counts(pred, t, crit), 5.0 + total(t, crit)])
        assert torch.equal(a.cpu(), want), f"pybind {crit}: got {a.tolist()} want {want.tolist()}"
        assert torch.equal(b.cpu(), want), f"dispatcher {crit}: got {b.tolist()} want {want.tolist()}"


# ------------------------------------------------------------------ the two classes
@pytest.mark.parametrize("c", [37, 260])
@pytest.mark.parametrize("tdtype", [torch.int32, torch.bool], **_dt_ids)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], **_dt_ids)
def test_classes_hold_the_oracles_integers(dtype, tdtype, c):
    dev = torch.device(DEV)
    for crit in CRITERIA:
        for k in (0, 2, 7):  # 0: MultilabelAccuracy at threshold 1.0 (a score equal to it is positive)
            m = (M.TopKMultilabelAccuracy(criteria=crit, k=k, device=dev) if k
                 else M.MultilabelAccuracy(threshold=1.0, criteria=crit, device=dev))
            run_c = run_t = 0
            for n in (5, 64, 130):
                x = tie_rows(dtype, n, c, max(k, 1), seed=n + c + k)
                pred = topk_pred(x, k) if k else oracle_pred(x, 1.0)
                t = k2_targets(pred, seed=n + c + k, dtype=tdtype)
                m.update(x.to(DEV), t.to(DEV))
                run_c, run_t = run_c + counts(pred, t, crit), run_t + total(t, crit)
                got = torch.stack([m.num_correct.reshape(()), m.num_total.reshape(())]).cpu()
                assert got.dtype == torch.float32
                assert torch.equal(got, torch.tensor([float(run_c), float(run_t)])), (
                    f"{type(m).__name__} {crit} k={k} after n={n}: got {got.tolist()} want {[run_c, run_t]}")
            exp = torch.tensor(float(run_c)) / torch.tensor(float(run_t))
            got = m.compute().cpu()
            assert torch.equal(got, exp), f"{type(m).__name__} {crit} k={k}: compute {got.item()!r} want {exp.item()!r}"
