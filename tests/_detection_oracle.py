"""Numpy oracle of COCO-style detection mean average precision: the definition of docs/parity.md
transliterated, loop by loop (images, classes, thresholds, detections, ground truths; the
right-to-left envelope; ``searchsorted`` over the 101 recall points).  Shares no code with the
package."""

import numpy as np

RECALL_GRID = np.linspace(0.0, 1.0, 101)


def default_thresholds():
    return np.linspace(0.5, 0.95, 10)


def iou(d, g):
    """One FP64 operation per step; numpy scalars never fuse a multiply and an add."""
    d = [np.float64(v) for v in d]
    g = [np.float64(v) for v in g]
    area_d = (d[2] - d[0]) * (d[3] - d[1])
    area_g = (g[2] - g[0]) * (g[3] - g[1])
    iw = max(np.float64(0.0), min(d[2], g[2]) - max(d[0], g[0]))
    ih = max(np.float64(0.0), min(d[3], g[3]) - max(d[1], g[1]))
    inter = iw * ih
    union = (area_d + area_g) - inter
    return inter / union if union > 0 else np.float64(0.0)


def match(pred_boxes, pred_scores, pred_labels, pred_counts, target_boxes, target_labels, target_counts,
          num_classes, thresholds, max_detections):
    """(scores f32 [M], labels [M], hits [M], gt_count [C], matched_gt [M, T]) in the matching order
    of every image: class ascending, score descending, equal scores in input order."""
    pred_boxes = np.asarray(pred_boxes, dtype=np.float64).reshape(-1, 4)
    target_boxes = np.asarray(target_boxes, dtype=np.float64).reshape(-1, 4)
    pred_scores = np.asarray(pred_scores, dtype=np.float32)
    pred_labels = np.asarray(pred_labels, dtype=np.int64)
    target_labels = np.asarray(target_labels, dtype=np.int64)
    thresholds = np.asarray(thresholds, dtype=np.float64)
    m, t = len(pred_scores), len(thresholds)
    scores = np.zeros(m, dtype=np.float32)
    labels = np.full(m, -1, dtype=np.int64)
    hits = np.zeros(m, dtype=np.int64)
    matched_gt = np.full((m, t), -1, dtype=np.int64)
    gt_count = np.zeros(num_classes, dtype=np.int64)
    d0 = g0 = 0
    for nd, ng in zip(pred_counts, target_counts):
        out = d0
        present = set(pred_labels[d0:d0 + nd].tolist()) | set(target_labels[g0:g0 + ng].tolist())
        assert all(0 <= c < num_classes for c in present), "the oracle takes valid labels only"
        for c in sorted(present):  # the classes without a box of the image do nothing
            dets = [i for i in range(d0, d0 + nd) if pred_labels[i] == c]
            gts = [i for i in range(g0, g0 + ng) if target_labels[i] == c]
            gt_count[c] += len(gts)
            if not dets:
                continue
            order = np.argsort(-pred_scores[dets].astype(np.float64), kind="mergesort")
            dets = [dets[i] for i in order]
            for rank, i in enumerate(dets):
                scores[out + rank] = pred_scores[i]
            kept = dets[:max_detections]
            seen = {}  # an IoU is the same number under every threshold
            for k in range(t):
                taken = set()
                for rank, i in enumerate(kept):
                    best, found = min(thresholds[k], 1 - 1e-10), None
                    for g in gts:
                        if g in taken:
                            continue
                        if (i, g) not in seen:
                            seen[i, g] = iou(pred_boxes[i], target_boxes[g])
                        v = seen[i, g]
                        if v < best:
                            continue
                        best, found = v, g
                    if found is not None:
                        taken.add(found)
                        hits[out + rank] |= 1 << k
                        matched_gt[out + rank, k] = found - g0
            labels[out:out + len(kept)] = c
            out += len(dets)
        assert out == d0 + nd
        d0, g0 = d0 + nd, g0 + ng
    return scores, labels, hits, gt_count, matched_gt


def tables(scores, labels, hits, gt_count, num_thresholds):
    """AP and REC [T, C] (float64, NaN for a class without ground truth) of stored detections."""
    scores = np.asarray(scores, dtype=np.float64)
    labels = np.asarray(labels)
    hits = np.asarray(hits).astype(np.int64)
    c = len(gt_count)
    ap = np.full((num_thresholds, c), np.nan)
    rec = np.full((num_thresholds, c), np.nan)
    for cls in np.flatnonzero(np.asarray(gt_count) > 0):
        n_gt = int(gt_count[cls])
        idx = np.flatnonzero(labels == cls)
        idx = idx[np.argsort(-scores[idx], kind="mergesort")]
        for k in range(num_thresholds):
            if len(idx) == 0:
                ap[k, cls] = 0.0
                rec[k, cls] = 0.0
                continue
            hit = (hits[idx] >> k) & 1
            tp = np.cumsum(hit).astype(np.float64)
            fp = np.cumsum(1 - hit).astype(np.float64)
            recall = tp / n_gt
            precision = tp / (fp + tp + np.spacing(1))
            envelope = precision.copy()
            for j in range(len(envelope) - 1, 0, -1):
                if envelope[j] > envelope[j - 1]:
                    envelope[j - 1] = envelope[j]
            at = np.searchsorted(recall, RECALL_GRID, side="left")
            samples = np.zeros(101)
            for q, j in enumerate(at):
                if j < len(envelope):
                    samples[q] = envelope[j]
            ap[k, cls] = np.mean(samples)
            rec[k, cls] = tp[-1] / n_gt
    return ap, rec


def _nanmean(x):
    x = np.asarray(x, dtype=np.float64)
    good = x[~np.isnan(x)]
    return np.float64(np.nan) if good.size == 0 else good.mean()


def results(ap, rec, thresholds):
    """The float64 results; callers round to float32."""
    thresholds = np.asarray(thresholds, dtype=np.float64)

    def row(value):
        at = np.flatnonzero(thresholds == value)
        return _nanmean(ap[at[0]]) if len(at) else np.float64(np.nan)

    with np.errstate(invalid="ignore"):
        return {
            "map": _nanmean(ap),
            "map_50": row(0.5),
            "map_75": row(0.75),
            "mar": _nanmean(rec),
            "map_per_class": ap.mean(axis=0),
            "mar_per_class": rec.mean(axis=0),
        }


def evaluate(pred_boxes, pred_scores, pred_labels, pred_counts, target_boxes, target_labels, target_counts,
             num_classes, thresholds=None, max_detections=100):
    thresholds = default_thresholds() if thresholds is None else np.asarray(thresholds, dtype=np.float64)
    scores, labels, hits, gt_count, _ = match(pred_boxes, pred_scores, pred_labels, pred_counts, target_boxes,
                                              target_labels, target_counts, num_classes, thresholds, max_detections)
    ap, rec = tables(scores, labels, hits, gt_count, len(thresholds))
    return results(ap, rec, thresholds)
