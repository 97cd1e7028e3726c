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
with its functions; nothing here is on a hot path.  ``misc_measures_multi_task`` (:86-242) ranks every task over its own population
from the masked counts of ``ops.rank_counts_masked``; ``regression_measures`` restates the scipy / scikit-learn values of :642-660.
``bootstrap_rank_metrics`` / ``bootstrap_compare`` (no counterpart in the reference) put percentile intervals on the four ranking
metrics and compare two score sets on the same resamples, from the weighted-rank kernel of ``ops.bootstrap_rank_metrics``."""
from __future__ import annotations

from typing import Callable, Dict, Optional

import numpy as np
import torch

DELTA = 1e-8


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def binary_rank_metrics(counts, labels, valid=None) -> Dict[str, np.ndarray]:
    """``counts`` int [n, C, 4] (ops.rank_counts), ``labels`` [n, C] (!= 0 = positive)  ->  dict(roc_auc, AP, auprc, max_f1), each a
    float64 [C] array: per class (one-vs-rest) roc_auc_score, average_precision_score, auc(recall, precision) of
    precision_recall_curve, and the reference's best F1 along that curve.  ValueError when a class has no positive or no negative
    (roc_auc_score raises there).  ``valid`` [n, C] (!= 0 = in the population) goes with the counts of ops.rank_counts_masked: class c
    is finished over its valid rows alone, as if the others had been filtered out first; an empty population raises ValueError."""
    cnt = _host(counts).astype(np.int64)
    lab = _host(labels) != 0
    if cnt.ndim != 3 or cnt.shape[2] != 4 or lab.shape != cnt.shape[:2]:
        raise ValueError(f"binary_rank_metrics: expected counts [n, C, 4] and labels [n, C], got {cnt.shape} and {lab.shape}")
    val = None
    if valid is not None:
        val = _host(valid) != 0
        if val.shape != lab.shape:
            raise ValueError(f"binary_rank_metrics: expected valid {lab.shape}, got {val.shape}")
    n, C = lab.shape
    out = {k: np.empty(C, dtype=np.float64) for k in ("roc_auc", "AP", "auprc", "max_f1")}
    for c in range(C):
        rows, pos, m = cnt[:, c], lab[:, c], n
        if val is not None:
            rows, pos = rows[val[:, c]], pos[val[:, c]]
            m = int(val[:, c].sum())
            if m == 0:
                raise ValueError(f"class {c}: the population is empty")
        P = int(pos.sum())
        N = m - P
        if P == 0 or N == 0:
            raise ValueError(f"class {c}: only one label value present ({P} positives of {m}); AUROC is not defined")
        gt_all, gt_pos, ge_all, ge_pos = (rows[pos, k] for k in range(4))
        neg_ge, neg_gt = ge_all - ge_pos, gt_all - gt_pos
        # twice the Mann-Whitney statistic, an exact integer
        out["roc_auc"][c] = float(np.sum(2 * (N - neg_ge) + (neg_ge - neg_gt))) / (2.0 * P * N)
        out["AP"][c] = float(np.sum(ge_pos / ge_all)) / P
        # one curve point per distinct score, from the highest threshold down; every sample of a tie carries the same pair
        ga, first = np.unique(rows[:, 2], return_index=True)
        gp = rows[first, 3]
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


def _device_rank_counts_masked(scores, labels, valid=None):
    if valid is None:
        return _device_rank_counts(scores, labels)
    if not all(isinstance(t, torch.Tensor) for t in (scores, labels, valid)):
        raise TypeError("the rank counts come from the HIP kernel, which takes GPU tensors (there is no CPU path): pass tensors on the "
                        "device, or a rank_counts function")
    from . import ops
    return ops.rank_counts_masked(scores, labels, valid)


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


_TASK_KEYS = ("accuracy", "roc_auc", "precision", "recall", "f1", "max_f1", "AP", "auprc", "balanced_acc", "specificity", "sensitivity", "mcc",
              "G", "kappa")


def multi_task_problem(y_true, y_pred, multi_task_type: str = "multi_task_default"):
    """The per-task binary problems of the multi-task modes as three [n, 2T] arrays ``(scores float32, labels uint8, valid uint8)``,
    torch tensors where ``y_pred`` lives when it is a tensor and numpy arrays otherwise.  Columns (2i, 2i + 1) belong to task i: the
    float32 softmax over its logit pair (``y_pred`` [n, 2T] read as [n, T, 2] for 'multi_task_default', columns (0, i + 1) of
    ``y_pred`` [n, T + 1] for any other type), the labels (y_true[:, 0], y_true[:, i + 1]), and twice the task's population
    ``y_true[:, 0] + y_true[:, i + 1] > 0`` (engine_finetune.py:95-111)."""
    as_tensor = isinstance(y_pred, torch.Tensor)
    logits = y_pred.detach().float() if as_tensor else torch.from_numpy(np.ascontiguousarray(y_pred, dtype=np.float32))
    truth = y_true.detach().to(logits.device) if isinstance(y_true, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(y_true))
    if logits.dim() != 2 or truth.dim() != 2 or truth.shape[0] != logits.shape[0] or truth.shape[1] < 2:
        raise ValueError(f"misc_measures_multi_task: expected y_true [n, T + 1] and y_pred [n, ...], got {tuple(truth.shape)} and "
                         f"{tuple(logits.shape)}")
    n, T = truth.shape[0], truth.shape[1] - 1
    if multi_task_type == "multi_task_default":
        if logits.shape[1] != 2 * T:
            raise ValueError(f"misc_measures_multi_task: {T} tasks need y_pred [n, {2 * T}] in the default layout, got {tuple(logits.shape)}")
        pairs = logits.reshape(n, T, 2)
    else:
        if logits.shape[1] != T + 1:
            raise ValueError(f"misc_measures_multi_task: {T} tasks need y_pred [n, {T + 1}] in the shared-column layout, got "
                             f"{tuple(logits.shape)}")
        pairs = torch.stack([logits[:, :1].expand(n, T), logits[:, 1:]], dim=2)
    scores = torch.softmax(pairs, dim=2).reshape(n, 2 * T).contiguous()
    pos = truth != 0
    labels = torch.stack([pos[:, :1].expand(n, T), pos[:, 1:]], dim=2)
    valid = ((truth[:, :1] + truth[:, 1:]) > 0).unsqueeze(2).expand(n, T, 2)
    labels = labels.reshape(n, 2 * T).to(torch.uint8).contiguous()
    valid = valid.reshape(n, 2 * T).to(torch.uint8).contiguous()
    if as_tensor:
        return scores, labels, valid
    return scores.numpy(), labels.numpy(), valid.numpy()


def multi_task_confusion(scores, labels, valid, threshold: float = 0.5) -> np.ndarray:
    """int64 [T, 2, 2]: [[tn, fp], [fn, tp]] of every task from the arrays of ``multi_task_problem`` -- the task's column-1 score
    against ``threshold`` and its column-1 label, over the task's own population."""
    s, y, v = _host(scores)[:, 1::2], _host(labels)[:, 1::2] != 0, _host(valid)[:, 1::2] != 0
    p = s > threshold
    return np.stack([(~y & ~p & v).sum(0), (~y & p & v).sum(0), (y & ~p & v).sum(0), (y & p & v).sum(0)], axis=1).reshape(-1, 2, 2)


def misc_measures_multi_task(y_true, y_pred, threshold: float = 0.5, multi_task_type: str = "multi_task_default",
                             rank_counts: Optional[Callable] = None):
    """engine_finetune.py:86-242: ``{"macro": {...}, "classwise": {...}}`` with the reference's keys for multi-task targets ``y_true``
    [n, T + 1] (column 0 the shared "normal" label) and LOGITS ``y_pred`` (see ``multi_task_problem`` for the two layouts).  Task i is
    judged over its own population, the samples with ``y_true[:, 0] + y_true[:, i + 1] > 0``: the threshold entries from the column-1
    softmax score against ``threshold`` with the reference's own formulas and ``1e-8`` terms, roc_auc / AP / auprc / max_f1 as the mean
    over the task's two columns, ``micro_AP`` as the average precision over the flattened pairs of all populations.

    The ranking entries come from rank counts: ``rank_counts(scores, labels, valid)`` once over the 2T columns (by default
    ops.rank_counts_masked) and ``rank_counts(scores, labels)`` once on the flattened micro problem (ops.rank_counts); the default needs
    GPU tensors, tests pass a numpy restatement.  ValueError, naming the task: an empty population, or a population in which a column
    has no positive or no negative (roc_auc_score raises there in the reference)."""
    rank_counts = rank_counts or _device_rank_counts_masked
    scores, lab, valid = multi_task_problem(y_true, y_pred, multi_task_type)
    s, y, v = _host(scores), _host(lab) != 0, _host(valid) != 0
    T = y.shape[1] // 2
    for i in range(T):
        m = int(v[:, 2 * i].sum())
        if m == 0:
            raise ValueError(f"task {i}: no sample carries the normal label or the task's label: its population is empty")
        for col in (0, 1):
            P = int((y[:, 2 * i + col] & v[:, 2 * i + col]).sum())
            if P == 0 or P == m:
                raise ValueError(f"task {i}, column {col}: only one label value present ({P} positives of {m}); AUROC is not defined")
    ranks = binary_rank_metrics(rank_counts(scores, lab, valid), y, valid=v)
    keep = valid != 0
    flat_s, flat_l = scores[keep].reshape(-1, 1), lab[keep].reshape(-1, 1)
    micro = binary_rank_metrics(rank_counts(flat_s, flat_l), flat_l)
    cm = multi_task_confusion(s, y, v, threshold).astype(np.float64)
    tn, fp, fn, tp = cm[:, 0, 0], cm[:, 0, 1], cm[:, 1, 0], cm[:, 1, 1]
    m = tn + fp + fn + tp
    cw = {}
    cw["accuracy"] = (tp + tn) / (m + DELTA)
    cw["sensitivity"] = tp / (tp + fn + DELTA)
    cw["specificity"] = tn / (tn + fp + DELTA)
    cw["precision"] = tp / (tp + fp + DELTA)
    cw["recall"] = tp / (tp + fn + DELTA)
    cw["f1"] = 2 * cw["precision"] * cw["recall"] / (cw["precision"] + cw["recall"] + DELTA)
    cw["mcc"] = (tp * tn - fp * fn) / np.sqrt((tp + fp) * (tp + fn) * (tn + fp) * (tn + fn) + DELTA)
    cw["G"] = np.sqrt(cw["sensitivity"] * cw["specificity"])
    cw["balanced_acc"] = (cw["sensitivity"] + cw["specificity"]) / 2
    # Cohen's kappa of [[tn, fp], [fn, tp]], as in misc_measures_multi_label (0 / 0: nan)
    expected = ((tn + fp) * (fp + tp) + (fn + tp) * (tn + fn)) / m
    with np.errstate(invalid="ignore", divide="ignore"):
        cw["kappa"] = 1.0 - (fp + fn) / expected
    for key in ("roc_auc", "AP", "auprc", "max_f1"):
        cw[key] = ranks[key].reshape(T, 2).mean(axis=1)
    macro = {"micro_AP": float(micro["AP"][0])}
    macro.update({k: float(np.mean(cw[k])) for k in _TASK_KEYS})
    return {"macro": macro, "classwise": {k: [float(x) for x in cw[k]] for k in _TASK_KEYS}}


# ---- bootstrap intervals of the ranking metrics.  A resample draws U resampling units with replacement (the samples themselves, or
# with ``groups`` the patients, each with all its samples: a cluster bootstrap) and is held as one int32 multiplicity per unit; the
# kernel of ops.bootstrap_rank_metrics (csrc/bootstrap.hip) sorts once and walks every resample over the sorted columns.  The host
# divides, drops the resamples in which a class has no positive or no negative (counted in ``n_defined``, not redrawn) and reads
# percentile intervals off the rest.  ``kernel=`` replaces the device op by any function of its signature (tests/bootstrap_ref.py:
# numpy), ``rank_counts=`` the counter behind the point estimates, as elsewhere in this file.
RANK_KEYS = ("roc_auc", "AP", "auprc", "max_f1")


def bootstrap_multiplicities(R: int, U: int, seed: int, device) -> torch.Tensor:
    """int32 [R, U]: row r counts how often each of U units is drawn when U units are drawn with replacement.  The draws are
    ``torch.randint(U, (R, U))`` from a ``torch.Generator`` of ``device`` seeded with ``seed``, counted by an integer ``scatter_add_``
    (integer atomics: the same tensor on every run).  The stream is torch's for that device: the CPU and the GPU differ, and numpy's
    resamples for the same seed differ from both."""
    if R < 1 or U < 1:
        raise ValueError(f"bootstrap_multiplicities: needs R >= 1 and U >= 1, got {R} and {U}")
    device = torch.device(device)
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    draws = torch.randint(U, (R, U), generator=gen, device=device)
    return torch.zeros((R, U), dtype=torch.int32, device=device).scatter_add_(1, draws, torch.ones((R, U), dtype=torch.int32, device=device))


def _device_bootstrap(scores, labels, mult, unit=None, valid=None):
    if not all(isinstance(t, torch.Tensor) for t in (scores, labels, mult)):
        raise TypeError("the resamples come from the HIP kernel, which takes GPU tensors (there is no CPU path): pass tensors on the "
                        "device, or a kernel function")
    from . import ops
    return ops.bootstrap_rank_metrics(scores, labels, mult, unit, valid)


def _dense_ids(groups):
    """ids of any hashable type -> (int64 ids in order of first occurrence [n], how many distinct ones), as coem._label_ids."""
    if isinstance(groups, (torch.Tensor, np.ndarray)):
        groups = groups.tolist()
    ids: dict = {}
    out = [ids.setdefault(g, len(ids)) for g in groups]
    return np.asarray(out, dtype=np.int64), len(ids)


def _bootstrap_problem(scores, labels, valid, resamples, seed, groups, mult):
    """The operands every score set of one call shares: ``(scores float32, labels uint8, valid uint8 or None, unit or None, mult)``,
    torch tensors where ``scores`` lives when it is a tensor and numpy arrays otherwise."""
    as_tensor = isinstance(scores, torch.Tensor)
    if as_tensor:
        s = scores.detach().float()
        lab = (torch.as_tensor(labels).detach().to(s.device) != 0).to(torch.uint8)
        val = None if valid is None else (torch.as_tensor(valid).detach().to(s.device) != 0).to(torch.uint8)
    else:
        s = np.ascontiguousarray(scores, dtype=np.float32)
        lab = (_host(labels) != 0).astype(np.uint8)
        val = None if valid is None else (_host(valid) != 0).astype(np.uint8)
    if s.ndim != 2 or tuple(lab.shape) != tuple(s.shape) or (val is not None and tuple(val.shape) != tuple(s.shape)):
        raise ValueError(f"bootstrap_rank_metrics: expected scores, labels and valid [n, C], got {tuple(s.shape)}, {tuple(lab.shape)}"
                         + ("" if val is None else f", {tuple(val.shape)}"))
    n = s.shape[0]
    unit, U = None, n
    if groups is not None:
        ids, U = _dense_ids(groups)
        if ids.shape[0] != n:
            raise ValueError(f"bootstrap_rank_metrics: {n} samples but {ids.shape[0]} group ids")
        unit = torch.from_numpy(ids).to(s.device) if as_tensor else ids
    if mult is None:
        mult = bootstrap_multiplicities(int(resamples), U, seed, s.device if as_tensor else "cpu")
        mult = mult if as_tensor else mult.numpy()
    elif tuple(mult.shape)[1:] != (U,) or len(mult.shape) != 2 or mult.shape[0] < 1:
        raise ValueError(f"bootstrap_rank_metrics: expected mult [R, {U}], got {tuple(mult.shape)}")
    return s, lab, val, unit, mult


def _bootstrap_samples(s, lab, val, unit, mult, kernel, rank_counts):
    """``(point {key: [C]}, samples {key: float64 [R, C], NaN where P == 0 or N == 0})`` of one score set."""
    if rank_counts is None:
        counts = _device_rank_counts_masked(s, lab, val)
    else:
        counts = rank_counts(s, lab) if val is None else rank_counts(s, lab, val)
    point = binary_rank_metrics(counts, lab, valid=val)
    raw = {k: _host(v) for k, v in (kernel or _device_bootstrap)(s, lab, mult, unit, val).items()}
    P, N = raw["P"].astype(np.int64), raw["N"].astype(np.int64)
    defined = (P > 0) & (N > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        samples = {"roc_auc": raw["U2"].astype(np.float64) / (2.0 * P * N), "AP": raw["ap_sum"].astype(np.float64) / P,
                   "auprc": raw["auprc"].astype(np.float64), "max_f1": raw["max_f1"].astype(np.float64)}
    return point, {k: np.where(defined, v, np.nan) for k, v in samples.items()}


def _macro_samples(samples: np.ndarray) -> np.ndarray:
    """[R, C] -> [R]: the mean over the classes, NaN unless every class is defined in the resample."""
    return samples.mean(axis=1)           # a NaN propagates through the mean


def _interval(samples: np.ndarray, alpha: float, what: str):
    """Percentile interval of the columns of ``samples`` [R, K] over their defined (non-NaN) rows: ``(low [K], high [K], n_defined
    [K])``; ValueError for a column that is never defined."""
    K = samples.shape[1]
    low, high, cnt = np.empty(K), np.empty(K), np.empty(K, dtype=np.int64)
    for k in range(K):
        col = samples[:, k]
        col = col[~np.isnan(col)]
        cnt[k] = col.size
        if col.size == 0:
            raise ValueError(f"{what} {k}: no resample holds both a positive and a negative: the interval is not defined")
        low[k], high[k] = np.quantile(col, alpha / 2), np.quantile(col, 1 - alpha / 2)
    return low, high, cnt


def bootstrap_rank_metrics(scores, labels, *, resamples: int = 1000, seed: int = 0, alpha: float = 0.05, groups=None, valid=None,
                           mult=None, kernel: Optional[Callable] = None, rank_counts: Optional[Callable] = None) -> dict:
    """Bootstrap percentile intervals of the four ranking metrics of ``binary_rank_metrics``: ``scores`` [n, C], ``labels`` [n, C]
    (!= 0 = positive), ``valid`` [n, C] or None (!= 0 = the sample belongs to the class's population).

    Returns, for each of ``roc_auc``, ``AP``, ``auprc``, ``max_f1``, a dict of ``point`` [C] (``binary_rank_metrics`` on the rank counts,
    unchanged), ``samples`` float64 [R, C] (NaN where the resample has no positive or no negative of the class), ``low`` / ``high`` [C]
    (``np.quantile`` at ``alpha / 2`` and ``1 - alpha / 2`` over the class's defined resamples, linear interpolation) and ``n_defined``
    [C]; under ``macro`` the same four keys for the mean over the classes (a float ``point``, ``samples`` [R], a resample counting only
    where every class is defined); and ``resamples`` (R) and ``level`` ("sample" or "group").  ValueError for a class without any
    defined resample.

    ``groups``: one hashable id per sample (a patient): units are drawn, and all their samples come with them.  ``mult`` int32 [R, U]
    overrides the draw of ``bootstrap_multiplicities(resamples, U, seed, device)``.  By default the resamples come from
    ops.bootstrap_rank_metrics and the point estimates from ops.rank_counts[_masked], for which the inputs must be GPU tensors (there
    is no CPU path); ``kernel`` / ``rank_counts`` replace them by functions of the same signatures."""
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"bootstrap_rank_metrics: alpha must lie in (0, 1), got {alpha}")
    s, lab, val, unit, mult = _bootstrap_problem(scores, labels, valid, resamples, seed, groups, mult)
    point, samples = _bootstrap_samples(s, lab, val, unit, mult, kernel, rank_counts)
    out: dict = {"macro": {}, "resamples": int(mult.shape[0]), "level": "sample" if groups is None else "group"}
    for key in RANK_KEYS:
        low, high, cnt = _interval(samples[key], alpha, "class")
        out[key] = {"point": point[key], "samples": samples[key], "low": low, "high": high, "n_defined": cnt}
        macro = _macro_samples(samples[key])
        low, high, cnt = _interval(macro[:, None], alpha, "macro over the classes: column")
        out["macro"][key] = {"point": float(np.mean(point[key])), "samples": macro, "low": float(low[0]), "high": float(high[0]),
                             "n_defined": int(cnt[0])}
    return out


def _delta_summary(delta: np.ndarray, alpha: float, what: str):
    """[R, K] differences (NaN where either side is undefined) -> (low [K], high [K], p [K], n_defined [K]): the percentile interval
    and the two-sided p = 2 min(share(delta <= 0), share(delta >= 0)) clipped to [1 / n_defined, 1]."""
    low, high, cnt = _interval(delta, alpha, what)
    p = np.empty(delta.shape[1])
    for k in range(delta.shape[1]):
        col = delta[:, k]
        col = col[~np.isnan(col)]
        p[k] = min(1.0, max(1.0 / col.size, 2.0 * min(np.mean(col <= 0), np.mean(col >= 0))))
    return low, high, p, cnt


def bootstrap_compare(scores_a, scores_b, labels, *, resamples: int = 1000, seed: int = 0, alpha: float = 0.05, groups=None, valid=None,
                      mult=None, kernel: Optional[Callable] = None, rank_counts: Optional[Callable] = None) -> dict:
    """Paired comparison of two score sets on one test set: both are walked with the SAME multiplicities, and per metric and class
    (and under ``macro`` for the mean over the classes) the result holds ``delta_point`` (a - b on the full set), ``delta_low`` /
    ``delta_high`` (the percentile interval of the resampled differences), ``p`` (two-sided: 2 min(share(delta <= 0), share(delta >=
    0)), clipped to [1 / n_defined, 1]) and ``n_defined`` (resamples defined for both).  Keywords as ``bootstrap_rank_metrics``."""
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"bootstrap_compare: alpha must lie in (0, 1), got {alpha}")
    sa, lab, val, unit, mult = _bootstrap_problem(scores_a, labels, valid, resamples, seed, groups, mult)
    sb = _bootstrap_problem(scores_b, labels, valid, resamples, seed, groups, mult)[0]
    if tuple(sa.shape) != tuple(sb.shape):
        raise ValueError(f"bootstrap_compare: the two score sets differ in shape: {tuple(sa.shape)} and {tuple(sb.shape)}")
    pa, xa = _bootstrap_samples(sa, lab, val, unit, mult, kernel, rank_counts)
    pb, xb = _bootstrap_samples(sb, lab, val, unit, mult, kernel, rank_counts)
    out: dict = {"macro": {}, "resamples": int(mult.shape[0]), "level": "sample" if groups is None else "group"}
    for key in RANK_KEYS:
        low, high, p, cnt = _delta_summary(xa[key] - xb[key], alpha, "class")
        out[key] = {"delta_point": pa[key] - pb[key], "delta_low": low, "delta_high": high, "p": p, "n_defined": cnt}
        macro = _macro_samples(xa[key]) - _macro_samples(xb[key])
        low, high, p, cnt = _delta_summary(macro[:, None], alpha, "macro over the classes: column")
        out["macro"][key] = {"delta_point": float(np.mean(pa[key]) - np.mean(pb[key])), "delta_low": float(low[0]),
                             "delta_high": float(high[0]), "p": float(p[0]), "n_defined": int(cnt[0])}
    return out


def regression_measures(pred, target) -> Dict[str, float]:
    """The regression block of the reference's ``evaluate`` (engine_finetune.py:642-660) on two vectors of equal length:
    ``pearsonr`` (scipy.stats.pearsonr), ``r2`` (r2_score), ``explained_variance`` (explained_variance_score), ``mse``, ``mae`` and
    ``R2 = pearsonr ** 2``, restated from their definitions in float64 in two-pass centred form (means first, then sums of centred
    terms): no scipy, no scikit-learn.  ValueError for fewer than two samples, and for constant targets or constant predictions --
    for the whole block, not only for the correlation, which is undefined there."""
    x = _host(pred).astype(np.float64).reshape(-1)
    y = _host(target).astype(np.float64).reshape(-1)
    if x.shape != y.shape or x.size < 2:
        raise ValueError(f"regression_measures: expected two vectors of one length >= 2, got {x.size} and {y.size}")
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        raise ValueError("regression_measures: non-finite predictions or targets")
    xc, yc = x - x.mean(), y - y.mean()
    sxx, syy = float(np.sum(xc * xc)), float(np.sum(yc * yc))
    if sxx == 0.0 or syy == 0.0:
        raise ValueError("regression_measures: constant " + ("predictions" if sxx == 0.0 else "targets") + ": the correlation and "
                         "the explained shares are not defined")
    r = float(np.sum(xc * yc)) / float(np.sqrt(sxx) * np.sqrt(syy))
    r = max(-1.0, min(1.0, r))
    d = y - x
    dc = d - d.mean()
    return {"pearsonr": r, "r2": 1.0 - float(np.sum(d * d)) / syy, "explained_variance": 1.0 - float(np.sum(dc * dc)) / syy,
            "mse": float(np.mean(d * d)), "mae": float(np.mean(np.abs(d))), "R2": r * r}


# ---- bootstrap intervals of the regression metrics.  Every entry of ``regression_measures`` of one resample is a function of eight
# weighted sums over the samples (count, sum a, sum b, sum a^2, sum b^2, sum a b, sum e^2, sum |e| with a = x - cx, b = y - cy,
# e = y - x), and a resample is a row of multiplicities: ops.bootstrap_moments (csrc/bootmoments.hip) forms all R rows of sums as one
# int32 x f64 matrix product in a fixed order, and the host finishes them here in float64.  The draws are those of the ranking
# metrics (``bootstrap_multiplicities``); ``kernel=`` replaces the device op by any function of its signature
# (tests/bootmoments_ref.py: numpy and exact rationals).
REGRESSION_KEYS = ("pearsonr", "r2", "explained_variance", "mse", "mae", "R2")


def _device_bootmoments(pred, target, mult, unit=None, valid=None, centre=None):
    if not all(isinstance(t, torch.Tensor) for t in (pred, target, mult)):
        raise TypeError("the resamples come from the HIP kernel, which takes GPU tensors (there is no CPU path): pass tensors on the "
                        "device, or a kernel function")
    from . import ops
    return ops.bootstrap_moments(pred, target, mult, unit, valid, centre)


def regression_variance_threshold(n: int) -> float:
    """tau(n) = (n + 8) 2^-50: a resample whose centred sum of squares Sxx = D3 - D1^2 / W is at most tau D3 has no variance that the
    sums can tell from zero, and counts as constant.

    Derivation, u = 2^-53, n the larger of the sample and the unit count.  D3 = sum w a^2 reaches the host with a relative error of at
    most (s + 6) u from the sums of a unit of s samples plus (U + 2) u from the product over U units, together below (2 n + 8) u of
    D3 (every term is positive, so the sum of the magnitudes is D3 itself).  D1 = sum w a carries the same share of sum w |a|, and by
    Cauchy-Schwarz (sum w |a|)^2 <= W D3, so D1^2 / W is off by at most (2 (2 n + 8) + 2) u of D3 (the square doubles the share; one
    rounding each for the product and the quotient).  The difference adds one rounding: in all (6 n + 27) u D3 <= (6 n + 30) 2^-53 D3.
    tau = (n + 8) 2^-50 = (8 n + 64) 2^-53 lies above that, so a resample of one sample drawn n times, whose exact Sxx is 0, computes
    an Sxx within its own error of zero and is caught, whatever the shift of the centre; a resample with two distinct values x1 != x2
    has Sxx / D3 of the order (x1 - x2)^2 / (n max a^2), far above tau unless the values agree to about 2^-25 of their distance from
    the centre -- float32 inputs centred near their mean do not."""
    return (n + 8) * 2.0 ** -50


def finish_regression_moments(moments, centre, n: int) -> dict:
    """``moments`` float64 [R, C, 8] and ``centre`` float64 [2, C] of ``ops.bootstrap_moments`` -> the six entries of
    ``regression_measures`` as float64 [R, C] each.  With W = D0:
    Sxx = D3 - D1^2 / W, Syy = D4 - D2^2 / W, Sxy = D5 - D1 D2 / W, sum e = D2 - D1 + (cy - cx) W,
    pearsonr = clip(Sxy / sqrt(Sxx Syy)), r2 = 1 - D6 / Syy, explained_variance = 1 - (D6 - (sum e)^2 / W) / Syy, mse = D6 / W,
    mae = D7 / W, R2 = pearsonr^2.  NaN (undefined): mse / mae only where W == 0; the four other keys where W < 2, Sxx <= tau D3 or
    Syy <= tau D4 with tau = ``regression_variance_threshold(n)``."""
    D = np.asarray(_host(moments), dtype=np.float64)
    c = np.asarray(_host(centre), dtype=np.float64)
    W, D1, D2, D3, D4, D5, D6, D7 = (D[:, :, k] for k in range(8))
    tau = regression_variance_threshold(n)
    with np.errstate(invalid="ignore", divide="ignore"):
        sxx, syy, sxy = D3 - D1 * D1 / W, D4 - D2 * D2 / W, D5 - D1 * D2 / W
        se = D2 - D1 + (c[1] - c[0])[None, :] * W
        bad = ~((W >= 2) & (sxx > tau * D3) & (syy > tau * D4))
        empty = ~(W > 0)
        r = np.clip(sxy / np.sqrt(sxx * syy), -1.0, 1.0)
        out = {"pearsonr": r, "r2": 1.0 - D6 / syy, "explained_variance": 1.0 - (D6 - se * se / W) / syy, "mse": D6 / W, "mae": D7 / W,
               "R2": r * r}
    return {k: np.where(empty if k in ("mse", "mae") else bad, np.nan, v) for k, v in out.items()}


def _regression_problem(pred, target, valid, resamples, seed, groups, mult, name):
    """``(pred float32 [n, C], target float32 [n, C], valid uint8 [n, C] or None, unit or None, mult)``: torch tensors where ``pred``
    lives when it is a tensor, numpy arrays otherwise; 1-D inputs become one column."""
    as_tensor = isinstance(pred, torch.Tensor)
    if as_tensor:
        x = pred.detach().float()
        y = torch.as_tensor(target).detach().to(x.device).float()
        val = None if valid is None else (torch.as_tensor(valid).detach().to(x.device) != 0).to(torch.uint8)
    else:
        x, y = np.asarray(_host(pred), dtype=np.float32), np.asarray(_host(target), dtype=np.float32)
        val = None if valid is None else (_host(valid) != 0).astype(np.uint8)
    if x.ndim == 1:
        x, y, val = x.reshape(-1, 1), y.reshape(-1, 1), None if val is None else val.reshape(-1, 1)
    if x.ndim != 2 or tuple(y.shape) != tuple(x.shape) or (val is not None and tuple(val.shape) != tuple(x.shape)) or x.shape[0] < 1:
        raise ValueError(f"{name}: expected pred, target and valid [n] or [n, C], got {tuple(x.shape)}, {tuple(y.shape)}"
                         + ("" if val is None else f", {tuple(val.shape)}"))
    n = x.shape[0]
    unit, U = None, n
    if groups is not None:
        ids, U = _dense_ids(groups)
        if ids.shape[0] != n:
            raise ValueError(f"{name}: {n} samples but {ids.shape[0]} group ids")
        unit = torch.from_numpy(ids).to(x.device) if as_tensor else ids
    if mult is None:
        mult = bootstrap_multiplicities(int(resamples), U, seed, x.device if as_tensor else "cpu")
        mult = mult if as_tensor else mult.numpy()
    elif len(mult.shape) != 2 or tuple(mult.shape)[1:] != (U,) or mult.shape[0] < 1:
        raise ValueError(f"{name}: expected mult [R, {U}], got {tuple(mult.shape)}")
    return x, y, val, unit, mult


def _regression_point(x, y, val) -> dict:
    """``regression_measures`` per column over the column's valid rows: key -> float64 [C]."""
    xh, yh = _host(x), _host(y)
    vh = None if val is None else _host(val) != 0
    cols = [regression_measures(xh[:, j] if vh is None else xh[vh[:, j], j], yh[:, j] if vh is None else yh[vh[:, j], j])
            for j in range(xh.shape[1])]
    return {k: np.asarray([m[k] for m in cols], dtype=np.float64) for k in REGRESSION_KEYS}


def _regression_samples(x, y, val, unit, mult, kernel) -> dict:
    raw = (kernel or _device_bootmoments)(x, y, mult, unit, val, None)
    return finish_regression_moments(raw["moments"], raw["centre"], max(int(x.shape[0]), int(mult.shape[1])))


def _require_defined(samples: np.ndarray, name: str, key: str):
    for j in range(samples.shape[1]):
        if np.isnan(samples[:, j]).all():
            raise ValueError(f"{name}: column {j}: no resample has a defined {key} (fewer than two distinct predictions or targets in "
                             "every one): the interval is not defined")


def bootstrap_regression_measures(pred, target, *, resamples: int = 1000, seed: int = 0, alpha: float = 0.05, groups=None, valid=None,
                                  mult=None, kernel: Optional[Callable] = None) -> dict:
    """Bootstrap percentile intervals of the six entries of ``regression_measures``: ``pred`` and ``target`` [n] or [n, C], ``valid``
    of the same shape or None (!= 0: the sample counts for the column).

    Returns, for each of ``pearsonr``, ``r2``, ``explained_variance``, ``mse``, ``mae``, ``R2``, a dict of ``point`` [C]
    (``regression_measures`` per column over its valid rows, unchanged: ValueError for a constant column), ``samples`` float64 [R, C]
    (NaN where the resample is undefined, see ``finish_regression_moments``), ``low`` / ``high`` [C] (``np.quantile`` at ``alpha / 2``
    and ``1 - alpha / 2`` over the column's defined resamples) and ``n_defined`` [C]; and ``resamples`` (R) and ``level`` ("sample" or
    "group").  Undefined resamples are dropped and counted, not redrawn; ValueError for a column without a defined resample.

    ``groups``, ``mult``, ``seed`` as in ``bootstrap_rank_metrics``: the same draws.  By default the sums come from
    ops.bootstrap_moments, for which the inputs must be GPU tensors (there is no CPU path); ``kernel`` replaces it by a function of the
    same signature."""
    name = "bootstrap_regression_measures"
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"{name}: alpha must lie in (0, 1), got {alpha}")
    x, y, val, unit, mult = _regression_problem(pred, target, valid, resamples, seed, groups, mult, name)
    point = _regression_point(x, y, val)
    samples = _regression_samples(x, y, val, unit, mult, kernel)
    out: dict = {"resamples": int(mult.shape[0]), "level": "sample" if groups is None else "group"}
    for key in REGRESSION_KEYS:
        _require_defined(samples[key], name, key)
        low, high, cnt = _interval(samples[key], alpha, "column")
        out[key] = {"point": point[key], "samples": samples[key], "low": low, "high": high, "n_defined": cnt}
    return out


def bootstrap_compare_regression(pred_a, pred_b, target, *, resamples: int = 1000, seed: int = 0, alpha: float = 0.05, groups=None,
                                 valid=None, mult=None, kernel: Optional[Callable] = None) -> dict:
    """Paired comparison of two prediction sets against one target set: both meet the SAME multiplicities, and per key of
    ``regression_measures`` the result holds ``delta_point`` (a - b on the full set), ``delta_low`` / ``delta_high``, ``p`` and
    ``n_defined`` as ``bootstrap_compare`` defines them, [C] each; plus ``resamples`` and ``level``."""
    name = "bootstrap_compare_regression"
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"{name}: alpha must lie in (0, 1), got {alpha}")
    xa, y, val, unit, mult = _regression_problem(pred_a, target, valid, resamples, seed, groups, mult, name)
    xb = _regression_problem(pred_b, target, valid, resamples, seed, groups, mult, name)[0]
    if tuple(xa.shape) != tuple(xb.shape):
        raise ValueError(f"{name}: the two prediction sets differ in shape: {tuple(xa.shape)} and {tuple(xb.shape)}")
    pa, pb = _regression_point(xa, y, val), _regression_point(xb, y, val)
    sa, sb = _regression_samples(xa, y, val, unit, mult, kernel), _regression_samples(xb, y, val, unit, mult, kernel)
    out: dict = {"resamples": int(mult.shape[0]), "level": "sample" if groups is None else "group"}
    for key in REGRESSION_KEYS:
        delta = sa[key] - sb[key]
        _require_defined(delta, name, key)
        low, high, p, cnt = _delta_summary(delta, alpha, "column")
        out[key] = {"delta_point": pa[key] - pb[key], "delta_low": low, "delta_high": high, "p": p, "n_defined": cnt}
    return out
