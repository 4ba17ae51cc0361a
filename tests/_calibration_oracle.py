"""The numpy FP64 oracle of the multiclass calibration error (docs/parity.md, "Not in the
reference"), shared by tests/metrics/classification/test_calibration_error.py and
tests/gpu/test_k15_calibration.py.  It takes the confidences as given, so that a test chooses
which confidence it bins: the scores' own float32 maxima (probabilities), a float32 softmax, or
the FP64 softmax of rows kept off the edges."""

import numpy as np


def edges(n_bins: int) -> np.ndarray:
    """float32(b / n_bins), the quotient in FP64."""
    return (np.arange(n_bins + 1, dtype=np.float64) / n_bins).astype(np.float32)


def bins_of(conf: np.ndarray, n_bins: int) -> np.ndarray:
    e = edges(n_bins).astype(conf.dtype) if conf.dtype == np.float64 else edges(n_bins)
    return np.clip(np.searchsorted(e, conf, side="left") - 1, 0, n_bins - 1)


def softmax_confidence(x: np.ndarray) -> np.ndarray:
    """1 / sum_j exp(x_j - max) per row of FP64 logits (-inf logits contribute 0)."""
    x = x.astype(np.float64)
    return 1.0 / np.exp(x - x.max(axis=1, keepdims=True)).sum(axis=1)


def states(conf: np.ndarray, pred: np.ndarray, target: np.ndarray, n_bins: int):
    """(bin_count, correct_sum, conf_sum) in FP64 of rows with the given confidences."""
    b = bins_of(conf, n_bins)
    count = np.bincount(b, minlength=n_bins).astype(np.float64)
    correct = np.bincount(b, weights=(pred == target).astype(np.float64), minlength=n_bins)
    conf_sum = np.bincount(b, weights=conf.astype(np.float64), minlength=n_bins)
    return count, correct, conf_sum


def value(count: np.ndarray, correct: np.ndarray, conf_sum: np.ndarray, norm: str) -> float:
    total = 0.0
    for c in count:
        total += c
    if total == 0 or np.isnan(conf_sum[0]):
        return float("nan")
    acc = 0.0
    for b in range(len(count)):
        if count[b] == 0:
            continue
        d = abs(correct[b] - conf_sum[b])
        if norm == "l1":
            acc += d
        elif norm == "max":
            acc = max(acc, d / count[b])
        else:
            acc += d * d / (count[b] * total)
    return acc / total if norm == "l1" else acc if norm == "max" else float(np.sqrt(acc))


def argmax_first(x: np.ndarray) -> np.ndarray:
    """The lowest index among each row's maxima (numpy's rule too)."""
    return np.argmax(x, axis=1)
