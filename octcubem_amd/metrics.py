"""The metrics of the reference's fine-tune evaluation (OCTCube/engine_finetune.py: ``misc_measures`` :346-382,
``misc_measures_multi_label`` :251-343, and the scikit-learn calls of ``evaluate`` :786-792), finished on the host in float64 from
INTEGERS: the rank counts of ``ops.rank_counts`` (csrc/metrics.hip) and a confusion matrix.  scikit-learn and pycm are no dependencies.

What scikit-learn computes, restated from its definitions with ties handled as it handles them (one curve point per distinct score).
For one class with P positives and N negatives, and per sample the counts {gt_all, gt_pos, ge_all, ge_pos}:
  roc_auc_score             sum over positives of (neg_lt + neg_eq / 2) / (P N), neg_ge = ge_all - ge_pos, neg_gt = gt_all - gt_pos,
                            neg_lt = N - neg_ge, neg_eq = neg_ge - neg_gt  (the Mann-Whitney statistic; the trapezoid under the ROC curve)
  average_precision_score   sum over positives of ge_pos / ge_all / P  (sum over thresholds of (R_k - R_k-1) P_k: the recall step at a
                            threshold is the share of the positives that tie there)
  precision_recall_curve    the points (recall, precision) = (ge_pos / P, ge_pos / ge_all), one per distinct ge_all, and (0, 1);
                            ``auc(recall, precision)`` is the trapezoid rule over them, the reference's ``max_f1`` scans them with
                            2 p r / (p + r + 1e-8).  (Newer scikit-learn keeps the points past full recall: they have zero width and a
                            smaller F1, so neither number depends on the version.)
The reference's own ``1e-8`` deltas stand exactly where it has them.  Provenance: a RESTATEMENT of the reference's formulas, call-compatible
with its two functions; nothing here is on a hot path."""
from __future__ import annotations

from typing import Callable, Dict, Optional

import numpy as np
import torch

DELTA = 1e-8


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def binary_rank_metrics(counts, labels) -> Dict[str, np.ndarray]:
    """``counts`` int [n, C, 4] (ops.rank_counts), ``labels`` [n, C] (!= 0 = positive)  ->  dict(roc_auc, AP, auprc, max_f1), each a
    float64 [C] array: per class (one-vs-rest) roc_auc_score, average_precision_score, auc(recall, precision) of
    precision_recall_curve, and the reference's best F1 along that curve.  ValueError when a class has no positive or no negative
    (roc_auc_score raises there)."""
    cnt = _host(counts).astype(np.int64)
    lab = _host(labels) != 0
    if cnt.ndim != 3 or cnt.shape[2] != 4 or lab.shape != cnt.shape[:2]:
        raise ValueError(f"binary_rank_metrics: expected counts [n, C, 4] and labels [n, C], got {cnt.shape} and {lab.shape}")
    n, C = lab.shape
    out = {k: np.empty(C, dtype=np.float64) for k in ("roc_auc", "AP", "auprc", "max_f1")}
    for c in range(C):
        pos = lab[:, c]
        P = int(pos.sum())
        N = n - P
        if P == 0 or N == 0:
            raise ValueError(f"class {c}: only one label value present ({P} positives of {n}); AUROC is not defined")
        gt_all, gt_pos, ge_all, ge_pos = (cnt[pos, c, k] for k in range(4))
        neg_ge, neg_gt = ge_all - ge_pos, gt_all - gt_pos
        # twice the Mann-Whitney statistic, an exact integer
        out["roc_auc"][c] = float(np.sum(2 * (N - neg_ge) + (neg_ge - neg_gt))) / (2.0 * P * N)
        out["AP"][c] = float(np.sum(ge_pos / ge_all)) / P
        # one curve point per distinct score, from the highest threshold down; every sample of a tie carries the same pair
        ga, first = np.unique(cnt[:, c, 2], return_index=True)
        gp = cnt[first, c, 3]
        recall = np.concatenate(([0.0], gp / P))
        precision = np.concatenate(([1.0], gp / ga))
        out["auprc"][c] = float(np.sum(np.diff(recall) * (precision[1:] + precision[:-1]) / 2.0))
        out["max_f1"][c] = max(0.0, float(np.max(2 * precision * recall / (precision + recall + DELTA))))
    return out


def misc_measures(confusion_matrix, start_cls_idx: int = 0):
    """engine_finetune.py:346-382 on a one-vs-rest confusion matrix [C, 2, 2] ([[tn, fp], [fn, tp]] per class): the class means
    ``(acc, sensitivity, specificity, precision, G, F1, mcc, balanced_acc)``."""
    cm = _host(confusion_matrix).astype(np.float64)
    cm = cm[start_cls_idx:]
    tn, fp, fn, tp = cm[:, 0, 0], cm[:, 0, 1], cm[:, 1, 0], cm[:, 1, 1]
    acc = (tn + tp) / (cm.sum(axis=(1, 2)) + DELTA)
    sensitivity = tp / (fn + tp + DELTA)
    specificity = tn / (fp + tn + DELTA)
    precision = tp / (tp + fp + DELTA)
    balanced = (tn / (tn + fp + DELTA) + tp / (fn + tp + DELTA)) / 2
    G = np.sqrt(sensitivity * specificity)
    f1 = 2 * precision * sensitivity / (precision + sensitivity + DELTA)
    mcc = (tn * tp - fp * fn) / (np.sqrt((tn + fp) * (tn + fn) * (tp + fn) * (tp + fp)) + DELTA)
    return (acc.mean(), sensitivity.mean(), specificity.mean(), precision.mean(), G.mean(), f1.mean(), mcc.mean(), balanced.mean())


def multilabel_confusion(true_idx: torch.Tensor, pred_idx: torch.Tensor, num_class: int) -> torch.Tensor:
    """sklearn's ``multilabel_confusion_matrix(true, pred, labels=range(num_class))`` of class indices: int64 [C, 2, 2] with
    [[tn, fp], [fn, tp]] per class, computed where the inputs live (three bincounts)."""
    t, p = true_idx.reshape(-1).long(), pred_idx.reshape(-1).long()
    n = t.numel()
    tp = torch.bincount(t[t == p], minlength=num_class)[:num_class]
    true_sum = torch.bincount(t, minlength=num_class)[:num_class]
    pred_sum = torch.bincount(p, minlength=num_class)[:num_class]
    fp, fn = pred_sum - tp, true_sum - tp
    tn = n - tp - fp - fn
    return torch.stack([tn, fp, fn, tp], dim=1).reshape(num_class, 2, 2)


def confusion_counts(true_idx: torch.Tensor, pred_idx: torch.Tensor, num_class: int) -> torch.Tensor:
    """The plain confusion matrix int64 [C, C] (rows: true class, columns: predicted class), one bincount where the inputs live."""
    t, p = true_idx.reshape(-1).long(), pred_idx.reshape(-1).long()
    return torch.bincount(t * num_class + p, minlength=num_class * num_class).reshape(num_class, num_class)


def _device_rank_counts(scores, labels):
    if not isinstance(scores, torch.Tensor) or not isinstance(labels, torch.Tensor):
        raise TypeError("the rank counts come from the HIP kernel, which takes GPU tensors (there is no CPU path): pass tensors on the "
                        "device, or a rank_counts function")
    from . import ops
    return ops.rank_counts(scores, labels)


def _safe_div(a, b):
    """scikit-learn's zero_division="warn" value: 0 where the denominator is 0."""
    return np.divide(a, b, out=np.zeros_like(a, dtype=np.float64), where=b != 0)


def misc_measures_multi_label(y_true, y_prob, threshold: float = 0.5, rank_counts: Optional[Callable] = None, **kwargs):
    """engine_finetune.py:251-343: ``{"macro": {...}, "classwise": {...}}`` with the reference's keys for multi-label targets
    ``y_true`` [n, C] (0 / 1) and scores ``y_prob`` [n, C].  The ranking entries (roc_auc, AP, auprc, max_f1, micro_AP) come from rank
    counts: ``rank_counts(scores float32 [m, K], labels uint8 [m, K]) -> int [m, K, 4]``, by default the HIP kernel, for which the
    inputs must be GPU tensors (there is no CPU fallback; tests pass a numpy restatement).  It is called twice: per class, and on the
    flattened [n * C, 1] problem that scikit-learn's average="micro" poses.  Every other entry comes from the per-class 2 x 2 table of
    ``y_prob > threshold``; ``kappa`` is Cohen's kappa of that table.  ``**kwargs`` is accepted and unused, as in the reference."""
    rank_counts = rank_counts or _device_rank_counts
    if isinstance(y_prob, torch.Tensor):
        scores = y_prob.detach().float()
        lab = (y_true.detach().to(scores.device) != 0).to(torch.uint8)
        flat_s, flat_l = scores.reshape(-1, 1), lab.reshape(-1, 1)
    else:
        scores = np.ascontiguousarray(y_prob, dtype=np.float32)
        lab = (np.asarray(y_true) != 0).astype(np.uint8)
        flat_s, flat_l = scores.reshape(-1, 1), lab.reshape(-1, 1)
    ranks = binary_rank_metrics(rank_counts(scores, lab), lab)
    micro = binary_rank_metrics(rank_counts(flat_s, flat_l), flat_l)
    y = _host(lab).astype(bool)
    pred = _host(scores) > threshold
    n, C = y.shape
    tp = (y & pred).sum(0).astype(np.float64)
    fp = (~y & pred).sum(0).astype(np.float64)
    fn = (y & ~pred).sum(0).astype(np.float64)
    tn = (~y & ~pred).sum(0).astype(np.float64)
    cw = {}
    cw["accuracy"] = (tp + tn) / n
    cw["roc_auc"] = ranks["roc_auc"]
    cw["precision"] = _safe_div(tp, tp + fp)
    cw["recall"] = _safe_div(tp, tp + fn)
    cw["f1"] = _safe_div(2 * tp, 2 * tp + fp + fn)
    cw["AP"] = ranks["AP"]
    cw["auprc"] = list(ranks["auprc"])
    cw["specificity"] = list(tn / (tn + fp + DELTA))
    cw["sensitivity"] = list(tp / (tp + fn + DELTA))
    cw["mcc"] = list((tp * tn - fp * fn) / np.sqrt((tp + fp) * (tp + fn) * (tn + fp) * (tn + fn) + DELTA))
    cw["G"] = np.sqrt(cw["recall"] * np.asarray(cw["specificity"]))
    cw["balanced_acc"] = list((np.asarray(cw["sensitivity"]) + np.asarray(cw["specificity"])) / 2)
    # Cohen's kappa of [[tn, fp], [fn, tp]]: 1 - observed disagreement / the disagreement expected from the margins (0 / 0: nan)
    expected = ((tn + fp) * (fp + tp) + (fn + tp) * (tn + fn)) / n
    with np.errstate(invalid="ignore", divide="ignore"):
        cw["kappa"] = list(1.0 - (fp + fn) / expected)
    cw["max_f1"] = list(ranks["max_f1"])
    order = ("accuracy", "roc_auc", "precision", "recall", "f1", "AP", "auprc", "specificity", "sensitivity", "mcc", "G")
    macro = {k: float(np.mean(cw[k])) for k in order}
    macro["micro_AP"] = float(micro["AP"][0])
    for k in ("balanced_acc", "kappa", "max_f1"):
        macro[k] = float(np.mean(cw[k]))
    classwise = {k: cw[k] for k in order + ("balanced_acc", "kappa", "max_f1")}
    return {"macro": macro, "classwise": classwise}
