"""Fine-tuning loop and evaluation with the reference's signatures (OCTCube/engine_finetune.py:386-482 ``train_one_epoch``,
:498 ``evaluate``): per-iteration LR schedule (every ``accum_iter``), H2D, float targets for BCE-type criteria, optional
mixup callable, forward, non-finite guard, ``loss_scaler(loss / accum_iter, clip_grad=max_norm, update_grad=...)``,
zero_grad on step boundaries, min/max group LR logging, scalar loss all-reduce.

Not reproduced: the per-iteration ``torch.cuda.synchronize()`` and logits printing (pipeline stalls with no numerical effect),
and the 2-D/3-D ``variable_joint`` reshape (a model outside SURVEY §8).  The SLIViT reshape (:417-419, :572-574) is applied when
``args.patient_dataset_type == "convnext_slivit"``: the slices of a volume laid side by side for model_slivit_baseline.SLIViT.  ``evaluate`` returns loss, top-1 accuracy and
the gathered logits / targets for a caller with metric code of its own; ``evaluate_report`` is the reference's ``evaluate`` (:498-813)
with its signature, its return value and its CSV files, the ranking metrics from the rank-count kernel (ops.rank_counts,
octcubem_amd/metrics.py) in place of scikit-learn, and the confusion matrix as a CSV of integers in place of the pycm / matplotlib JPEG.

Provenance, stated once: this file is a RESTATEMENT of the reference's host loop, written to be call-compatible with it -- same
function signatures, same order of operations per iteration, same ``MetricLogger`` keys -- because it is the caller SURVEY section 8
(R14 / N1, N3) requires and the reference's drivers import it by name.  It holds no kernel logic; everything it calls (models, scaler,
optimizer, schedules) is this package's own.

``evaluate_task_report`` is that ``evaluate`` for all five task modes: the three of ``evaluate_report``, ``multi_task*`` (per-task
metrics over per-task populations from ops.rank_counts_masked, metrics.misc_measures_multi_task) and ``regression``."""
from __future__ import annotations

import csv
import math
import os
from typing import Iterable, Optional

import numpy as np
import torch

from . import losses, lr_sched, metrics, misc


def _slivit_reshape(samples: torch.Tensor, args) -> torch.Tensor:
    """engine_finetune.py:417-419 / :572-574, for ``patient_dataset_type`` ``convnext_slivit`` only: ``permute(0, 2, 3, 4, 1)`` then
    ``reshape(-1, s[1], s[2], s[3] * s[4])`` of the permuted shape ``s``, exactly as the reference writes it.  Anything else passes through."""
    if getattr(args, "patient_dataset_type", None) != "convnext_slivit":
        return samples
    samples = samples.permute(0, 2, 3, 4, 1)
    return samples.reshape(-1, samples.shape[1], samples.shape[2], samples.shape[3] * samples.shape[4])


def train_one_epoch(model: torch.nn.Module, criterion: torch.nn.Module, data_loader: Iterable, optimizer: torch.optim.Optimizer,
                    device: torch.device, epoch: int, loss_scaler, max_norm: float = 0, mixup_fn=None, log_writer=None, args=None):
    model.train(True)
    metric_logger = misc.MetricLogger(delimiter="  ")
    metric_logger.add_meter("lr", misc.SmoothedValue(window_size=1, fmt="{value:.6f}"))
    header = "Epoch: [{}]".format(epoch)
    print_freq = 20
    accum_iter = args.accum_iter
    optimizer.zero_grad()
    n_iter = len(data_loader)
    float_targets = isinstance(criterion, torch.nn.BCEWithLogitsLoss) or getattr(args, "task_mode", "") == "regression"
    # the reference's multi_task_loss (:45-70, called at :443): one two-class problem per task out of multi-label targets
    multi_task = (str(getattr(args, "task_mode", "")).startswith("multi_task")
                  and isinstance(criterion, losses.WeightedLabelSmoothingCrossEntropy))
    for data_iter_step, (samples, targets) in enumerate(metric_logger.log_every(misc.prefetched(data_loader, device, args, only=(0, 1)), print_freq, header)):
        if data_iter_step % accum_iter == 0:
            lr_sched.adjust_learning_rate(optimizer, data_iter_step / n_iter + epoch, args)
        samples = samples.to(device, non_blocking=True)
        targets = targets.to(device, non_blocking=True)
        if float_targets:
            targets = targets.float()
        samples = _slivit_reshape(samples, args)
        if mixup_fn is not None:
            samples, targets = mixup_fn(samples, targets)
        outputs = model(samples)
        loss = losses.multi_task_loss(outputs, targets, criterion, args.task_mode) if multi_task else criterion(outputs, targets)
        loss_value = loss.item()
        if not math.isfinite(loss_value):
            print("Loss is {}, stopping training".format(loss_value))
            return None
        loss = loss / accum_iter
        loss_scaler(loss, optimizer, clip_grad=max_norm, parameters=model.parameters(), create_graph=False,
                    update_grad=(data_iter_step + 1) % accum_iter == 0)
        if (data_iter_step + 1) % accum_iter == 0:
            optimizer.zero_grad()
        metric_logger.update(loss=loss_value)
        min_lr, max_lr = 10.0, 0.0
        for group in optimizer.param_groups:
            min_lr = min(min_lr, group["lr"])
            max_lr = max(max_lr, group["lr"])
        metric_logger.update(lr=max_lr)
        loss_value_reduce = misc.all_reduce_mean(loss_value)
        if log_writer is not None and (data_iter_step + 1) % accum_iter == 0:
            epoch_1000x = int((data_iter_step / n_iter + epoch) * 1000)
            log_writer.add_scalar("loss", loss_value_reduce, epoch_1000x)
            log_writer.add_scalar("lr", max_lr, epoch_1000x)
    metric_logger.synchronize_between_processes()
    print("Averaged stats:", metric_logger)
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


@torch.no_grad()
def evaluate(data_loader: Iterable, model: torch.nn.Module, device: torch.device, criterion: Optional[torch.nn.Module] = None, args=None):
    """Eval-mode pass: ``{"loss", "acc1", "logits" [n, C], "targets" [n]}`` (logits / targets on the host, fp32).  ``args`` is read for
    ``patient_dataset_type`` only (the SLIViT reshape)."""
    criterion = criterion or torch.nn.CrossEntropyLoss()
    model.eval()
    logits_all, targets_all, loss_sum, n = [], [], 0.0, 0
    for samples, targets in misc.prefetched(data_loader, device, None, only=(0, 1)):
        samples = samples.to(device, non_blocking=True)
        targets = targets.to(device, non_blocking=True)
        out = model(_slivit_reshape(samples, args)).float()
        t = targets.float() if isinstance(criterion, torch.nn.BCEWithLogitsLoss) else targets
        loss_sum += float(criterion(out, t)) * samples.shape[0]
        n += samples.shape[0]
        logits_all.append(out.cpu())
        targets_all.append(targets.cpu())
    logits = torch.cat(logits_all)
    tg = torch.cat(targets_all)
    acc1 = float((logits.argmax(-1) == (tg if tg.dim() == 1 else tg.argmax(-1))).float().mean()) if n else float("nan")
    return {"loss": loss_sum / max(n, 1), "acc1": acc1, "logits": logits, "targets": tg}


_REPORT_MODES = ("binary_cls", "multi_cls", "multi_label")
_UNBUILT_ARGS = ("frame_inference_all", "return_embeddings", "variable_joint")
METRICS_HEADER = ["acc", "balanced_acc", "sensitivity", "specificity", "precision", "auc_roc", "auc_pr", "F1", "mcc", "loss"]
MACRO_HEADER = ["Accuracy", "ROC AUC", "Average Precision", "AUPRC", "F1 Score", "Balanced Acc", "MCC", "G-Mean", "Precision", "Recall",
                "Sensitivity", "Specificity", "Micro AP", "Kappa", "Max F1", "loss"]
_MACRO_KEYS = ("accuracy", "roc_auc", "AP", "auprc", "f1", "balanced_acc", "mcc", "G", "precision", "recall", "sensitivity", "specificity",
               "micro_AP", "kappa", "max_f1")
CLASS_HEADER = ["Accuracy", "ROC AUC", "Average Precision", "AUPRC", "F1 Score", "Balanced Acc", "MCC", "G-Mean", "precision", "recall",
                "specificity", "sensitivity", "Max F1", "Kappa"]
_CLASS_KEYS = ("accuracy", "roc_auc", "AP", "auprc", "f1", "balanced_acc", "mcc", "G", "precision", "recall", "specificity", "sensitivity",
               "max_f1", "kappa")


def _append_row(path: str, header, row):
    """One row appended to a CSV, the header first when the file is empty."""
    with open(path, mode="a", newline="", encoding="utf8") as f:
        w = csv.writer(f)
        if f.tell() == 0:
            w.writerow(header)
        w.writerow([float(v) for v in row])


def _write_int_matrix(path: str, m):
    with open(path, mode="w", newline="", encoding="utf8") as f:
        csv.writer(f).writerows([[int(v) for v in r] for r in np.asarray(m)])


CI_HEADER = ["epoch", "metric", "class", "point", "low", "high", "n_defined", "resamples", "alpha", "seed", "level"]


def _bootstrap_report(task, epoch, mode, scores, labels, names, args):
    """The opt-in bootstrap of ``evaluate_report`` (``args.bootstrap`` = R > 0): percentile intervals of roc_auc / AP / auprc / max_f1
    of the scores the report has just ranked, appended to ``metrics_ci_<mode>.csv`` (CI_HEADER): per metric one row for ``macro`` and
    one per class, named through ``names``.  ``args.bootstrap_seed`` (0), ``args.bootstrap_alpha`` (0.05), ``args.bootstrap_groups``
    (None; one id per sample in the loader's order: patients are drawn instead of samples, ``level`` = group)."""
    R = int(args.bootstrap)
    seed, alpha = int(getattr(args, "bootstrap_seed", 0) or 0), float(getattr(args, "bootstrap_alpha", 0.05) or 0.05)
    groups = getattr(args, "bootstrap_groups", None)
    res = metrics.bootstrap_rank_metrics(scores, labels, resamples=R, seed=seed, alpha=alpha, groups=groups)
    with open(os.path.join(task, f"metrics_ci_{mode}.csv"), mode="a", newline="", encoding="utf8") as f:
        w = csv.writer(f)
        if f.tell() == 0:
            w.writerow(CI_HEADER)
        tail = [res["resamples"], alpha, seed, res["level"]]
        for key in metrics.RANK_KEYS:
            m = res["macro"][key]
            w.writerow([epoch, key, "macro", float(m["point"]), float(m["low"]), float(m["high"]), int(m["n_defined"])] + tail)
            for i, name in enumerate(names):
                c = res[key]
                w.writerow([epoch, key, name, float(c["point"][i]), float(c["low"][i]), float(c["high"][i]), int(c["n_defined"][i])] + tail)


@torch.no_grad()
def evaluate_report(data_loader, model, device, task, epoch, mode, num_class, criterion=torch.nn.CrossEntropyLoss(),
                    task_mode="binary_cls", disease_list=None, return_bal_acc=False, args=None):
    """The reference's ``evaluate`` (engine_finetune.py:498-813) for ``task_mode`` binary_cls, multi_cls and multi_label: an eval-mode
    pass over ``data_loader`` (batch[0] the input, batch[-1] the target), then the report under the directory ``task``.

    Returns ``({"loss", "acc1"}, auc_roc, auc_pr)``, or ``({...}, auc_roc, (auc_pr, balanced_acc))`` with ``return_bal_acc``.  For
    binary_cls / multi_cls ``auc_roc`` is the macro one-vs-rest AUROC of the softmax scores against the one-hot targets and ``auc_pr``
    the macro AVERAGE PRECISION (the reference's variable of that name holds average_precision_score); for multi_label they are
    ``macro["roc_auc"]`` and ``macro["auprc"]`` of ``metrics.misc_measures_multi_label`` on the sigmoid scores.  ``loss`` is the mean
    over samples and ``acc1`` the top-1 fraction, both as ``evaluate`` above defines them.

    Files: ``metrics_<mode>.csv`` (one row per call: METRICS_HEADER), or for multi_label ``macro_metrics_<mode>.csv`` (MACRO_HEADER) and
    ``class_<i>_<name>_metrics_<mode>.csv`` per class (CLASS_HEADER; names from ``disease_list``, a dict or a sequence), the header
    written when the file is empty; and, when ``mode`` starts with "test" and ``args.not_save_figs`` is not set,
    ``confusion_matrix_<mode>_epoch_<epoch>.csv`` (integers, rows = true class, columns = predicted class) or per class of a
    multi-label task ``confusion_matrix_<mode>_<i>_<name>_epoch_<epoch>.csv`` ([[tn, fp], [fn, tp]]).

    Logits, scores, targets and the running sums of loss and top-1 stay on the device for the whole loop: no ``.item()`` or ``.cpu()``
    per step, one synchronisation at the end.  The metrics cover what THIS rank's loader yields, as in the reference.
    ``regression`` and ``multi_task*`` raise NotImplementedError here: ``evaluate_task_report`` below serves them and hands the three
    modes of this function on unchanged, so a driver binds that one as ``evaluate``.  ``args.frame_inference_all`` /
    ``return_embeddings`` / ``variable_joint`` must be unset or falsy.

    Opt-in: ``args.bootstrap`` = R > 0 appends bootstrap percentile intervals of roc_auc / AP / auprc / max_f1 of the same scores
    (softmax one-vs-rest against the one-hot targets, or sigmoid against the multi-label targets) to ``metrics_ci_<mode>.csv``
    (``_bootstrap_report``; ``args.bootstrap_seed``, ``args.bootstrap_alpha``, ``args.bootstrap_groups``).  Absent, None or 0: nothing
    changes, neither a file nor the return value; set, the return value is still the one above."""
    if task_mode not in _REPORT_MODES:
        if task_mode == "regression" or str(task_mode).startswith("multi_task"):
            raise NotImplementedError(f"evaluate_report: task_mode {task_mode!r} is not built (built: {', '.join(_REPORT_MODES)})")
        raise ValueError(f"evaluate_report: unknown task_mode {task_mode!r}")
    for name in _UNBUILT_ARGS:
        assert not getattr(args, name, False), f"evaluate_report: args.{name} is not built"
    os.makedirs(task, exist_ok=True)
    device = torch.device(device)
    float_targets = isinstance(criterion, torch.nn.BCEWithLogitsLoss)
    model.eval()
    scores_all, targets_all = [], []
    loss_sum = torch.zeros((), dtype=torch.float64, device=device)
    correct = torch.zeros((), dtype=torch.int64, device=device)
    n = 0
    for batch in misc.prefetched(data_loader, device, args, only=(0, 1)):
        samples = batch[0].to(device, non_blocking=True)
        targets = batch[-1].to(device, non_blocking=True)
        out = model(_slivit_reshape(samples, args))
        with torch.autocast(device.type, enabled=False):
            out = out.float()
            loss = criterion(out, targets.float() if float_targets else targets)
            scores = torch.sigmoid(out) if task_mode == "multi_label" else torch.softmax(out, dim=1)
        bs = samples.shape[0]
        loss_sum += loss.double() * bs
        correct += (out.argmax(-1) == (targets if targets.dim() == 1 else targets.argmax(-1))).sum()
        n += bs
        scores_all.append(scores)
        targets_all.append(targets)
    if n == 0:
        raise ValueError("evaluate_report: the loader yielded no sample")
    scores, targets = torch.cat(scores_all), torch.cat(targets_all)
    if scores.shape[1] != num_class:
        raise ValueError(f"evaluate_report: the model has {scores.shape[1]} outputs, num_class is {num_class}")

    if task_mode == "multi_label":
        res = metrics.misc_measures_multi_label(targets, scores, threshold=0.5)
        macro, classwise = res["macro"], res["classwise"]
        stats = {"loss": float(loss_sum) / n, "acc1": int(correct) / n}
        _append_row(os.path.join(task, f"macro_metrics_{mode}.csv"), MACRO_HEADER, [macro[k] for k in _MACRO_KEYS] + [stats["loss"]])
        if disease_list is None:
            disease_list = {i: str(i) for i in range(num_class)}
        elif not isinstance(disease_list, dict):
            disease_list = dict(enumerate(disease_list))
        assert len(disease_list) == num_class
        pred = (scores > 0.5).cpu().numpy()
        true = (targets != 0).cpu().numpy()
        for i, name in disease_list.items():
            _append_row(os.path.join(task, f"class_{i}_{name}_metrics_{mode}.csv"), CLASS_HEADER, [classwise[k][i] for k in _CLASS_KEYS])
            if mode.startswith("test") and not getattr(args, "not_save_figs", False):
                t, p = true[:, i], pred[:, i]
                _write_int_matrix(os.path.join(task, f"confusion_matrix_{mode}_{i}_{name}_epoch_{epoch}.csv"),
                                  [[(~t & ~p).sum(), (~t & p).sum()], [(t & ~p).sum(), (t & p).sum()]])
        print("Metrics - Acc: {:.4f} AUC-roc: {:.4f}, AP: {:4f}, AUC-pr: {:.4f} F1-score: {:.4f}, Max F1: {:.4f}, Balanced Acc: {:.4f}, "
              "Kappa: {:.4f}, MCC: {:.4f}".format(macro["accuracy"], macro["roc_auc"], macro["AP"], macro["auprc"], macro["f1"],
                                                  macro["max_f1"], macro["balanced_acc"], macro["kappa"], macro["mcc"]))
        if getattr(args, "bootstrap", None):
            _bootstrap_report(task, epoch, mode, scores, targets != 0, [disease_list.get(i, str(i)) for i in range(num_class)], args)
        if return_bal_acc:
            return stats, macro["roc_auc"], (macro["auprc"], macro["balanced_acc"])
        return stats, macro["roc_auc"], macro["auprc"]

    true_idx = targets.long()
    pred_idx = scores.argmax(dim=1)
    onehot = torch.nn.functional.one_hot(true_idx, num_classes=num_class).to(torch.uint8)
    from . import ops
    ranks = metrics.binary_rank_metrics(ops.rank_counts(scores, onehot), onehot)
    ovr = metrics.multilabel_confusion(true_idx, pred_idx, num_class).cpu().numpy()
    confusion = metrics.confusion_counts(true_idx, pred_idx, num_class).cpu().numpy()
    stats = {"loss": float(loss_sum) / n, "acc1": int(correct) / n}
    acc, sensitivity, specificity, precision, G, F1, mcc, balanced_acc = (float(v) for v in metrics.misc_measures(ovr))
    auc_roc, auc_pr = float(ranks["roc_auc"].mean()), float(ranks["AP"].mean())
    print("Metrics - Acc: {:.4f} Balanced-Acc: {:.4f} AUC-roc: {:.4f} AUC-pr: {:.4f} F1-score: {:.4f} MCC: {:.4f}".format(
        acc, balanced_acc, auc_roc, auc_pr, F1, mcc))
    _append_row(os.path.join(task, f"metrics_{mode}.csv"), METRICS_HEADER,
                [acc, balanced_acc, sensitivity, specificity, precision, auc_roc, auc_pr, F1, mcc, stats["loss"]])
    if mode.startswith("test") and not getattr(args, "not_save_figs", False):
        _write_int_matrix(os.path.join(task, f"confusion_matrix_{mode}_epoch_{epoch}.csv"), confusion)
    if getattr(args, "bootstrap", None):
        named = {} if disease_list is None else disease_list if isinstance(disease_list, dict) else dict(enumerate(disease_list))
        _bootstrap_report(task, epoch, mode, scores, onehot, [named.get(i, str(i)) for i in range(num_class)], args)
    if return_bal_acc:
        return stats, auc_roc, (auc_pr, balanced_acc)
    return stats, auc_roc, auc_pr


REGRESSION_HEADER = ["Pearsonr", "R\u00b2", "ExplainedVariance", "MSE", "MAE", "R2", "Loss"]
_REGRESSION_KEYS = ("pearsonr", "r2", "explained_variance", "mse", "mae", "R2", "loss")


@torch.no_grad()
def evaluate_task_report(data_loader, model, device, task, epoch, mode, num_class, criterion=torch.nn.CrossEntropyLoss(),
                         task_mode="binary_cls", disease_list=None, return_bal_acc=False, args=None):
    """The reference's ``evaluate`` (engine_finetune.py:498-813) for all five task modes, the function a driver binds as ``evaluate``.
    ``binary_cls``, ``multi_cls`` and ``multi_label`` go to ``evaluate_report`` unchanged; an unknown mode raises ValueError;
    ``args.frame_inference_all`` / ``return_embeddings`` / ``variable_joint`` must be unset or falsy.  ``args.bootstrap`` (the
    bootstrap intervals of ``evaluate_report``) is refused here for ``multi_task*`` and ``regression``: set, it raises
    NotImplementedError.  Their intervals are a call of their own, ``bootstrap_task_report`` on the logits and targets that ``evaluate``
    returns; this function writes the same files with and without them.

    ``multi_task*`` (targets [n, T + 1], column 0 the shared "normal" label; ``num_class`` model outputs: 2T for
    'multi_task_default', T + 1 otherwise): returns ``({"loss", "acc1"}, macro roc_auc, macro auprc)`` of
    ``metrics.misc_measures_multi_task`` on the logits, ``acc1`` the macro accuracy as in the reference, and with ``return_bal_acc``
    ``(..., (auprc, balanced_acc))``.  Logits and targets stay on the device for the whole loop, one synchronisation at the end.
    Files: ``macro_metrics_<mode>.csv`` (MACRO_HEADER), ``class_<i+1>_<name>_metrics_<mode>.csv`` per task (CLASS_HEADER) and, when
    ``mode`` starts with "test" and ``args.not_save_figs`` is not set, ``confusion_matrix_<mode>_<i+1>_<name>_epoch_<epoch>.csv``
    ([[tn, fp], [fn, tp]] of the task over its own population).  Names: ``disease_list[args.multi_task_idx[i]]`` when
    ``args.multi_task_idx`` is given, else ``disease_list[i + 1]`` (without a list, ``str(i + 1)``).
    Two departures from the reference, both on purpose.  The loss: with ``WeightedLabelSmoothingCrossEntropy`` it is
    ``losses.multi_task_loss`` of ALL gathered logits and targets as one batch (the loss the mode trains, whose per-task means do not
    split over batches); the reference calls the criterion on the unsplit [B, 2T] / [B, T + 1] pair, which any other criterion still
    gets here, averaged over samples.  The confusion matrices: thresholded task softmax scores over the task's population; the
    reference thresholds raw logit columns of all samples.

    ``regression``: column 0 of a 2-D target with ``output[:, 0]``, both flattened; ``metrics.regression_measures`` in float64 on the
    host (ValueError for constant targets or predictions).  Appends ``regression_metrics_<mode>.csv`` (REGRESSION_HEADER, four
    decimals as in the reference) and returns the flat dict ``pearsonr, r2, explained_variance, mse, mae, R2, loss``, ``loss`` the
    mean over samples of ``criterion(output, target.float())``."""
    if task_mode in _REPORT_MODES:
        return evaluate_report(data_loader, model, device, task, epoch, mode, num_class, criterion=criterion, task_mode=task_mode,
                               disease_list=disease_list, return_bal_acc=return_bal_acc, args=args)
    multi_task = str(task_mode).startswith("multi_task")
    if not multi_task and task_mode != "regression":
        raise ValueError(f"evaluate_task_report: unknown task_mode {task_mode!r}")
    for name in _UNBUILT_ARGS:
        assert not getattr(args, name, False), f"evaluate_task_report: args.{name} is not built"
    if getattr(args, "bootstrap", None):
        raise NotImplementedError(f"evaluate_task_report: args.bootstrap is not built for task_mode {task_mode!r} (built: "
                                  f"{', '.join(_REPORT_MODES)})")
    os.makedirs(task, exist_ok=True)
    device = torch.device(device)
    whole_set_loss = multi_task and isinstance(criterion, losses.WeightedLabelSmoothingCrossEntropy)
    float_targets = task_mode == "regression" or isinstance(criterion, torch.nn.BCEWithLogitsLoss)
    model.eval()
    out_all, targets_all = [], []
    loss_sum = torch.zeros((), dtype=torch.float64, device=device)
    n = 0
    for batch in misc.prefetched(data_loader, device, args, only=(0, 1)):
        samples = batch[0].to(device, non_blocking=True)
        targets = batch[-1].to(device, non_blocking=True)
        out = model(_slivit_reshape(samples, args))
        with torch.autocast(device.type, enabled=False):
            out = out.float()
            if not whole_set_loss:
                loss_sum += criterion(out, targets.float() if float_targets else targets).double() * samples.shape[0]
        n += samples.shape[0]
        if task_mode == "regression":
            if targets.dim() > 1:
                targets, out = targets[:, 0], out[:, 0]
            targets, out = targets.reshape(-1), out.reshape(-1)
        out_all.append(out)
        targets_all.append(targets)
    if n == 0:
        raise ValueError("evaluate_task_report: the loader yielded no sample")
    logits, targets = torch.cat(out_all), torch.cat(targets_all)

    if task_mode == "regression":
        res = metrics.regression_measures(logits, targets)
        res["loss"] = float(loss_sum) / n
        print("Regression Metrics - Pearsonr: {:.4f} R\u00b2: {:.4f} ExplainedVariance: {:.4f} MSE: {:.4f} MAE: {:.4f}, R2: {:.4f}, "
              "Loss: {:.4f}".format(*(res[k] for k in _REGRESSION_KEYS)))
        with open(os.path.join(task, f"regression_metrics_{mode}.csv"), mode="a", newline="", encoding="utf8") as f:
            w = csv.writer(f)
            if f.tell() == 0:
                w.writerow(REGRESSION_HEADER)
            w.writerow([f"{res[k]:.4f}" for k in _REGRESSION_KEYS])
        return {k: res[k] for k in _REGRESSION_KEYS}

    if logits.shape[1] != num_class:
        raise ValueError(f"evaluate_task_report: the model has {logits.shape[1]} outputs, num_class is {num_class}")
    with torch.autocast(device.type, enabled=False):
        if whole_set_loss:
            loss_sum = losses.multi_task_loss(logits, targets, criterion, task_mode).double() * n
        res = metrics.misc_measures_multi_task(targets, logits, threshold=0.5, multi_task_type=task_mode)
        confusion = metrics.multi_task_confusion(*metrics.multi_task_problem(targets, logits, task_mode), threshold=0.5)
    macro, classwise = res["macro"], res["classwise"]
    stats = {"loss": float(loss_sum) / n, "acc1": macro["accuracy"]}
    _append_row(os.path.join(task, f"macro_metrics_{mode}.csv"), MACRO_HEADER, [macro[k] for k in _MACRO_KEYS] + [stats["loss"]])
    T = len(classwise["accuracy"])
    idx = getattr(args, "multi_task_idx", None)
    if disease_list is None:
        names = [str(i + 1) for i in range(T)]
    else:
        names = [disease_list[idx[i]] if idx is not None else disease_list[i + 1] for i in range(T)]
    for i, name in enumerate(names):
        _append_row(os.path.join(task, f"class_{i + 1}_{name}_metrics_{mode}.csv"), CLASS_HEADER, [classwise[k][i] for k in _CLASS_KEYS])
        if mode.startswith("test") and not getattr(args, "not_save_figs", False):
            _write_int_matrix(os.path.join(task, f"confusion_matrix_{mode}_{i + 1}_{name}_epoch_{epoch}.csv"), confusion[i])
    print("Metrics - Acc: {:.4f} AUC-roc: {:.4f}, AP: {:4f}, AUC-pr: {:.4f} F1-score: {:.4f}, Max F1: {:.4f}, Balanced Acc: {:.4f}, "
          "Kappa: {:.4f}, MCC: {:.4f}".format(macro["accuracy"], macro["roc_auc"], macro["AP"], macro["auprc"], macro["f1"],
                                              macro["max_f1"], macro["balanced_acc"], macro["kappa"], macro["mcc"]))
    if return_bal_acc:
        return stats, macro["roc_auc"], (macro["auprc"], macro["balanced_acc"])
    return stats, macro["roc_auc"], macro["auprc"]


def bootstrap_task_report(task, epoch, mode, logits, targets, task_mode, disease_list=None, args=None):
    """Bootstrap intervals for the two task modes whose report ``evaluate_task_report`` writes without them, from the ``logits`` and
    ``targets`` that ``evaluate`` returns (a driver calls it after the report).  Appends to ``metrics_ci_<mode>.csv`` under CI_HEADER,
    with ``args.bootstrap`` = R > 0 resamples and ``args.bootstrap_seed`` / ``bootstrap_alpha`` / ``bootstrap_groups`` as
    ``_bootstrap_report``; with ``args.bootstrap`` absent, None or 0 it writes nothing and returns None.  ``logits`` and ``targets``
    may live on the host, as ``evaluate`` returns them (tensors or numpy arrays): they are moved to ``args.device`` (default "cuda"),
    where the kernels run.

    ``regression``: ``logits[:, 0]`` against column 0 of ``targets`` (as the report), one row per key of
    ``metrics.regression_measures``, class "target", from ``metrics.bootstrap_regression_measures``.
    ``multi_task*``: ``metrics.multi_task_problem(targets, logits, task_mode)`` with its ``valid`` handed to
    ``metrics.bootstrap_rank_metrics``; a task's value in a resample is the mean over its two columns (as
    ``misc_measures_multi_task``), undefined unless both are defined; per ranking metric one row ``macro`` (the mean over the tasks)
    and one per task, named as ``evaluate_task_report`` names them.  Returns the result dict of the metrics call."""
    if not getattr(args, "bootstrap", None):
        return None
    multi_task = str(task_mode).startswith("multi_task")
    if not multi_task and task_mode != "regression":
        raise ValueError(f"bootstrap_task_report: task_mode {task_mode!r} is reported by evaluate_report (built here: regression, multi_task*)")
    R = int(args.bootstrap)
    seed, alpha = int(getattr(args, "bootstrap_seed", 0) or 0), float(getattr(args, "bootstrap_alpha", 0.05) or 0.05)
    groups = getattr(args, "bootstrap_groups", None)
    # ``evaluate`` returns host tensors; the kernels take device tensors and have no CPU path
    device = torch.device(getattr(args, "device", None) or "cuda")
    logits = torch.as_tensor(np.asarray(logits) if not isinstance(logits, torch.Tensor) else logits).detach().to(device)
    targets = torch.as_tensor(np.asarray(targets) if not isinstance(targets, torch.Tensor) else targets).detach().to(device)
    os.makedirs(task, exist_ok=True)
    rows = []
    if multi_task:
        scores, labels, valid = metrics.multi_task_problem(targets, logits, task_mode)
        res = metrics.bootstrap_rank_metrics(scores, labels, resamples=R, seed=seed, alpha=alpha, groups=groups, valid=valid)
        T = scores.shape[1] // 2
        idx = getattr(args, "multi_task_idx", None)
        if disease_list is None:
            names = [str(i + 1) for i in range(T)]
        else:
            names = [disease_list[idx[i]] if idx is not None else disease_list[i + 1] for i in range(T)]
        res["tasks"] = {}
        for key in metrics.RANK_KEYS:
            samples = res[key]["samples"].reshape(-1, T, 2).mean(axis=2)          # a NaN propagates through the mean
            point = np.asarray(res[key]["point"], dtype=np.float64).reshape(T, 2).mean(axis=1)
            low, high, cnt = metrics._interval(samples, alpha, "task")
            mlow, mhigh, mcnt = metrics._interval(samples.mean(axis=1)[:, None], alpha, "macro over the tasks: column")
            res["tasks"][key] = {"point": point, "samples": samples, "low": low, "high": high, "n_defined": cnt}
            rows.append([key, "macro", float(point.mean()), float(mlow[0]), float(mhigh[0]), int(mcnt[0])])
            rows += [[key, name, float(point[i]), float(low[i]), float(high[i]), int(cnt[i])] for i, name in enumerate(names)]
    else:
        out, tgt = logits, targets
        if tgt.dim() > 1:
            tgt = tgt[:, 0]
        if out.dim() > 1:
            out = out[:, 0]
        res = metrics.bootstrap_regression_measures(out.reshape(-1).float(), tgt.reshape(-1).float(), resamples=R, seed=seed, alpha=alpha,
                                                    groups=groups)
        rows = [[key, "target", float(res[key]["point"][0]), float(res[key]["low"][0]), float(res[key]["high"][0]),
                 int(res[key]["n_defined"][0])] for key in metrics.REGRESSION_KEYS]
    with open(os.path.join(task, f"metrics_ci_{mode}.csv"), mode="a", newline="", encoding="utf8") as f:
        w = csv.writer(f)
        if f.tell() == 0:
            w.writerow(CI_HEADER)
        for row in rows:
            w.writerow([epoch] + row + [res["resamples"], alpha, seed, res["level"]])
    return res
