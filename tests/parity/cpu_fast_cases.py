"""Inputs of ``tests/test_cpu_fast_paths.py`` and the reference's side of every comparison in it.

The test compares against ``tests/golden/cpu_fast_paths.pt``: the value of ``reference_records``
as ``gen_goldens.py`` recorded it from the reference on CPU.  Inputs come from seeded CPU
generators, so the test rebuilds the very tensors the recording saw.
"""

import contextlib
import logging

import torch

NUM_CLASSES = 6

MACRO_WEIGHTED = [
    ("multiclass_accuracy", ("macro",)),
    ("multiclass_f1_score", ("macro", "weighted")),
    ("multiclass_precision", ("macro", "weighted")),
    ("multiclass_recall", ("macro", "weighted")),
]
MACRO_WEIGHTED_SEEDS = range(6)
TOP_K = [2, 3]
CONFUSION_SEEDS = range(4)
CLASS_CASES = [
    ("MulticlassF1Score", {"num_classes": 6, "average": "macro"}),
    ("MulticlassF1Score", {"num_classes": 6, "average": "weighted"}),
    ("MulticlassPrecision", {"num_classes": 6, "average": "macro"}),
    # (recall over batches where every class occurs: the reference crashes otherwise)
    ("MulticlassRecall", {"num_classes": 6, "average": "weighted"}),
    ("MulticlassAccuracy", {"num_classes": 6, "average": "macro"}),
    ("MulticlassConfusionMatrix", {"num_classes": 6}),
    ("MulticlassConfusionMatrix", {"num_classes": 6, "normalize": "true"}),
]
REGRESSION_SHAPES = [(8,), (8, 4), (1, 3), (5, 1)]
SAMPLE_STORE_CLASSES = ["BinaryAUROC", "BinaryAUPRC"]
R2_STATES = ("sum_squared_obs", "sum_obs", "sum_squared_residual", "num_obs")


def batches(seed: int, n: int = 8, c: int = NUM_CLASSES):
    g = torch.Generator().manual_seed(seed)
    scores = torch.randn(n, c, generator=g)
    scores[0, 1] = float("nan") if seed % 3 == 0 else scores[0, 1]
    scores[1] = 0.25  # an all-tie row: argmax is the first index
    target = torch.randint(0, c - 2, (n,), generator=g)  # the last two classes never appear
    labels = torch.randint(0, c, (n,), generator=g)
    return scores, target, labels


def macro_weighted_inputs(seed: int, averages):
    """(average, input, target) of every call of one macro / weighted case, in order."""
    scores, target, labels = batches(seed)
    for avg in averages:
        for inp in (scores, labels, scores.double()):
            for tgt in (target, target.int()) if inp is scores else (target,):
                yield avg, inp, tgt


def confusion_inputs(seed: int):
    """(name, args, kwargs) of every confusion-matrix call of one seed, in order."""
    scores, target, labels = batches(seed)
    for inp in (scores, labels, scores.double()):
        yield "multiclass_confusion_matrix", (inp, target), {"num_classes": 6}
    yield "multiclass_confusion_matrix", (scores, target.int()), {"num_classes": 6}
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(9, generator=g)
    x[2] = float("nan")
    x[4] = 0.5  # on the threshold: predicts 1
    y = torch.randint(0, 2, (9,), generator=g)
    for thr in (0.5, 0.3):
        yield "binary_confusion_matrix", (x, y), {"threshold": thr}
    yield "binary_confusion_matrix", (x, y), {"normalize": "all"}


def class_updates(cls: str):
    """Two runs of (scores, target) updates for one class case; compute() follows every update."""
    first = []
    for seed in range(3):
        scores, target, _ = batches(seed)
        if cls == "MulticlassRecall":
            target = torch.arange(8) % 6
        first.append((scores, target))
    scores, target, _ = batches(7)
    if cls == "MulticlassRecall":
        target = torch.arange(8).flip(0) % 6
    return first, [(scores, target)]


def regression_updates(shape, weighted: bool):
    """Three (input, target, sample_weight or None) updates for one regression case."""
    g = torch.Generator().manual_seed(len(shape) * 10 + shape[0])
    out = []
    for _ in range(3):
        x, t = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
        w = torch.rand(shape[0], generator=g) if weighted else None
        out.append((x, t, w))
    return out


def sample_store_updates():
    g = torch.Generator().manual_seed(3)
    return [(torch.rand(8, generator=g), torch.randint(0, 2, (8,), generator=g)) for _ in range(4)]


def class_key(cls: str, kw: dict) -> str:
    return "class/" + cls + "/" + ",".join(f"{k}={v}" for k, v in sorted(kw.items()))


def regression_key(shape, weighted: bool) -> str:
    return f"regression/{'x'.join(map(str, shape))}/{'weighted' if weighted else 'plain'}"


class _Records(logging.Handler):
    def __init__(self) -> None:
        super().__init__(level=logging.WARNING)
        self.messages = []

    def emit(self, record: logging.LogRecord) -> None:
        self.messages.append(record.getMessage())


@contextlib.contextmanager
def warnings_logged():
    """The messages logged at WARNING or above inside the block (what ``caplog`` would hold)."""
    h = _Records()
    root = logging.getLogger()
    root.addHandler(h)
    try:
        yield h.messages
    finally:
        root.removeHandler(h)


def reference_records(RM, RF) -> dict:
    """Every value the test expects, computed by the reference (``RM`` metrics, ``RF`` functional)."""
    out = {}
    for fn, averages in MACRO_WEIGHTED:
        for seed in MACRO_WEIGHTED_SEEDS:
            rows = []
            for avg, inp, tgt in macro_weighted_inputs(seed, averages):
                try:
                    with warnings_logged() as log:
                        value = getattr(RF, fn)(inp, tgt.long(), num_classes=6, average=avg)
                    rows.append({"value": value, "log": list(log)})
                except RuntimeError:
                    rows.append({"raises": "RuntimeError"})
            out[f"macro_weighted/{fn}/{seed}"] = rows
    scores, target, _ = batches(11)
    for k in TOP_K:
        out[f"top_k/{k}"] = RF.multiclass_accuracy(scores, target, average="macro", num_classes=6, k=k)
    for seed in CONFUSION_SEEDS:
        out[f"confusion/{seed}"] = [getattr(RF, name)(*a, **kw) for name, a, kw in confusion_inputs(seed)]
    for cls, kw in CLASS_CASES:
        m, values = getattr(RM, cls)(**kw), []
        first, second = class_updates(cls)
        for run in (first, second):
            for scores, target in run:
                m.update(scores, target)
                values.append(m.compute().clone())
            m.reset()
        out[class_key(cls, kw)] = values
    for shape in REGRESSION_SHAPES:
        for weighted in (False, True):
            mse, r2 = RM.MeanSquaredError(), RM.R2Score()
            for x, t, w in regression_updates(shape, weighted):
                if weighted:
                    mse.update(x, t, sample_weight=w)
                else:
                    mse.update(x, t)
                if shape[0] >= 2:
                    r2.update(x, t)
            rec = {"sum_squared_error": mse.sum_squared_error, "sum_weight": mse.sum_weight, "mse": mse.compute()}
            if shape[0] >= 2:
                for name in R2_STATES:
                    rec[name] = getattr(r2, name)
                rec["r2"] = r2.compute()
            out[regression_key(shape, weighted)] = rec
    for cls in SAMPLE_STORE_CLASSES:
        m = getattr(RM, cls)()
        for x, y in sample_store_updates():
            m.update(x, y)
        out[f"sample_store/{cls}"] = m.compute()
    return out
