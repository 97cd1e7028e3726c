"""Test helper, not a test: numpy references for the ranking metrics, written from the definitions and independent of
octcubem_amd/metrics.py.

``rank_counts``   the four counts of octmae_rank_counts as a plain O(n^2) comparison table (IEEE comparisons of float32 values).
``auroc`` / ``average_precision`` / ``auprc`` / ``max_f1``   sort-based float64, one class: the ROC and precision-recall curves are
built threshold by threshold (one point per distinct score, from the highest down) from cumulative true / false positive counts, the
way the definitions read, and integrated with the trapezoid rule / the step rule.  Nothing here knows about rank counts."""
import numpy as np


def rank_counts(scores, labels) -> np.ndarray:
    """int32 [n, C, 4] = {gt_all, gt_pos, ge_all, ge_pos}; accepts numpy arrays or torch tensors."""
    s = np.asarray(scores.cpu() if hasattr(scores, "cpu") else scores, dtype=np.float32)
    lab = np.asarray(labels.cpu() if hasattr(labels, "cpu") else labels) != 0
    n, C = s.shape
    out = np.empty((n, C, 4), dtype=np.int32)
    for c in range(C):
        col, pos = s[:, c], lab[:, c]
        gt = col[None, :] > col[:, None]          # [i, j]: s[j] > s[i]
        ge = col[None, :] >= col[:, None]
        out[:, c, 0] = gt.sum(1)
        out[:, c, 1] = (gt & pos[None, :]).sum(1)
        out[:, c, 2] = ge.sum(1)
        out[:, c, 3] = (ge & pos[None, :]).sum(1)
    return out


def _curve(scores, labels):
    """Cumulative (tp, fp) at every distinct threshold, highest first."""
    s = np.asarray(scores, dtype=np.float64)
    y = (np.asarray(labels) != 0).astype(np.float64)
    order = np.argsort(-s, kind="stable")
    s, y = s[order], y[order]
    last = np.r_[np.nonzero(s[1:] != s[:-1])[0], s.size - 1]   # the last sample of every run of equal scores (inf == inf, -0.0 == 0.0)
    tp = np.cumsum(y)[last]
    fp = (1 + last) - tp
    return tp, fp


def auroc(scores, labels) -> float:
    tp, fp = _curve(scores, labels)
    P, N = tp[-1], fp[-1]
    if P == 0 or N == 0:
        raise ValueError("only one label value present")
    tpr, fpr = np.r_[0.0, tp / P], np.r_[0.0, fp / N]
    return float(np.sum((fpr[1:] - fpr[:-1]) * (tpr[1:] + tpr[:-1]) * 0.5))


def _pr(scores, labels):
    tp, fp = _curve(scores, labels)
    return tp / tp[-1], tp / (tp + fp)                      # recall, precision; thresholds from the highest down


def average_precision(scores, labels) -> float:
    recall, precision = _pr(scores, labels)
    return float(np.sum(np.diff(np.r_[0.0, recall]) * precision))


def auprc(scores, labels) -> float:
    """Trapezoid rule over the precision-recall points, with the conventional end point (recall 0, precision 1)."""
    recall, precision = _pr(scores, labels)
    r, p = np.r_[0.0, recall], np.r_[1.0, precision]
    return float(np.sum((r[1:] - r[:-1]) * (p[1:] + p[:-1]) * 0.5))


def max_f1(scores, labels) -> float:
    recall, precision = _pr(scores, labels)
    r, p = np.r_[0.0, recall], np.r_[1.0, precision]
    return float(np.max(2 * p * r / (p + r + 1e-8)))


def macro(fn, scores, labels) -> float:
    """The mean over the columns of [n, C] scores / labels of a one-class function above."""
    s, y = np.asarray(scores), np.asarray(labels)
    return float(np.mean([fn(s[:, c], y[:, c]) for c in range(s.shape[1])]))
