"""The downstream fine-tune of a COEM checkpoint: regression of GA area, GA growth and BCVA from the OCT volume and its en-face images
-- the ``cls_dataset`` branch of ``retinal-COEM/src/training/train_retclip_finetune_more_cls_3mod.py`` (``train_one_epoch`` :95-378,
``evaluate`` :382-695) for ``args.multimodal_type`` in 'oct3d_paired_faf_cls', 'oct3d_paired_ir_cls' (coem.CustomTextCLIPClassification on
the OCT volume and the chosen en-face image) and 'oct3d_paired_faf_ir_cls' (coem.CustomTextCLIP3ModClassification, with
``args.single_modality``).  The contrastive branch of the reference's function is coem.train_one_epoch.

What differs from the reference, on purpose: no ``.item()`` / ``.cpu()`` per step -- logits and labels are collected on the device and
come to the host once per epoch, and the log line (two scalars read back) is written every ``args.log_every_n_steps``-th step and on the
last one, where the reference's inverted gate writes it on every step that is not such a multiple; the end-of-epoch statistics are float64 on the host from metrics.regression_measures (no scipy); a
``GradScaler``, horovod and wandb are refused by name; ``zero_shot_eval``, the scatter plots and the pickles of ``evaluate`` are left out
(the per-target JSON files beside the pickles are written)."""
from __future__ import annotations

import json
import logging
import math
import os
import time

import numpy as np
import torch

from . import coem
from .metrics import bootstrap_regression_measures, regression_measures

CLS_TYPES = ("oct3d_paired_faf_cls", "oct3d_paired_ir_cls", "oct3d_paired_faf_ir_cls")
METRIC_KEYS = ("pearsonr", "r2", "mse", "mae", "PearsonR", "R2")
PLOT_NAMES = ["GAArea", "BCVABASE", "GAGrowth", "BCVARATE", "BCVACHG72"]
PLOT_RANGES = ([0, 40, 0, -50, -50], [20, 80, 5, 20, 20])
PLOT_NAMES_GAGROWTH = ["GAArea", "GAGrowth"]
PLOT_RANGES_GAGROWTH = ([0, 0], [20, 5])
GAGROWTH_TYPES = ("GAGrowth", "GAGrowth_eyenotate", "GAGrowth_OCTCorr")


def regression_loss(logits: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
    """train_retclip_finetune_more_cls_3mod.py:191-200: per target column the mean squared and the mean absolute error over the batch,
    weighted [0.1, 1, ..., 1] and divided by 2 * sum(weights).  Plain torch on the device: at [B, <= 5] elements this is a handful of
    launches next to three ViT towers -- not worth a kernel of its own."""
    if logits.shape != label.shape or logits.dim() != 2:
        raise ValueError(f"regression_loss: logits and label must be one [B, C] shape, got {tuple(logits.shape)} and {tuple(label.shape)}")
    d = logits.float() - label.float()
    w = torch.ones(d.shape[1], dtype=torch.float32, device=d.device)
    w[0] = 0.1
    return (((d * d).mean(dim=0) + d.abs().mean(dim=0)) * w).sum() / (2.0 * (0.1 + (d.shape[1] - 1)))


def compute_r2(y_true, y_pred) -> float:
    """The reference's ``compute_r2`` (:37-39): Pearson's r squared -- NOT the coefficient of determination."""
    return regression_measures(y_pred, y_true)["R2"]


def column_metrics(logits, labels) -> dict:
    """``pearsonr_j``, ``r2_j`` (``compute_r2``), ``mse_j``, ``mae_j``, ``PearsonR_j`` (np.corrcoef's entry: the same number) and
    ``R2_j`` for every target column j, float64 on the host.  A column whose predictions or targets are constant has no correlation: the
    four correlation entries are NaN there (what np.corrcoef gives), ``mse_j`` / ``mae_j`` are still reported."""
    x = np.asarray(torch.as_tensor(logits).detach().cpu().numpy(), dtype=np.float64)
    y = np.asarray(torch.as_tensor(labels).detach().cpu().numpy(), dtype=np.float64)
    if x.shape != y.shape or x.ndim != 2:
        raise ValueError(f"column_metrics: two [N, C] arrays of one shape, got {x.shape} and {y.shape}")
    out = {}
    for j in range(x.shape[1]):
        d = y[:, j] - x[:, j]
        try:
            m = regression_measures(x[:, j], y[:, j])
            r, mse, mae = m["pearsonr"], m["mse"], m["mae"]
        except ValueError:
            if not (np.isfinite(x[:, j]).all() and np.isfinite(y[:, j]).all()) or x.shape[0] < 2:
                raise
            r, mse, mae = float("nan"), float(np.mean(d * d)), float(np.mean(np.abs(d)))
        out.update({f"pearsonr_{j}": r, f"r2_{j}": r * r, f"mse_{j}": mse, f"mae_{j}": mae, f"PearsonR_{j}": r, f"R2_{j}": r * r})
    return out


def bootstrap_column_metrics(logits, labels, point: dict, args) -> dict:
    """The opt-in bootstrap of ``evaluate`` (``args.bootstrap`` = R > 0): for every target column j the percentile bounds
    ``pearsonr_j_low`` / ``_high``, ``r2_j_low`` / ``_high`` (of r squared, which is what ``r2_j`` is here), ``mse_j_low`` / ``_high``,
    ``mae_j_low`` / ``_high`` and ``bootstrap_n_defined_j`` (the resamples with a defined correlation), from
    ``metrics.bootstrap_regression_measures`` on the same normalised ``logits`` and ``labels`` [N, C] as the point values ``point`` of
    ``column_metrics``.  ``args.bootstrap_seed`` (0), ``args.bootstrap_alpha`` (0.05), ``args.bootstrap_groups`` (None; one id per
    sample in the loader's order: patients are drawn instead of samples).  A column whose point correlation is NaN (constant
    predictions or targets) gets NaN bounds and ``bootstrap_n_defined_j`` 0."""
    R = int(args.bootstrap)
    seed, alpha = int(getattr(args, "bootstrap_seed", 0) or 0), float(getattr(args, "bootstrap_alpha", 0.05) or 0.05)
    groups = getattr(args, "bootstrap_groups", None)
    C = logits.shape[1]
    good = [j for j in range(C) if not math.isnan(point[f"pearsonr_{j}"])]
    res = bootstrap_regression_measures(logits[:, good], labels[:, good], resamples=R, seed=seed, alpha=alpha, groups=groups) if good else None
    out = {}
    for j in range(C):
        k = good.index(j) if j in good else None
        for name, key in (("pearsonr", "pearsonr"), ("r2", "R2"), ("mse", "mse"), ("mae", "mae")):
            out[f"{name}_{j}_low"] = float("nan") if k is None else float(res[key]["low"][k])
            out[f"{name}_{j}_high"] = float("nan") if k is None else float(res[key]["high"][k])
        out[f"bootstrap_n_defined_{j}"] = 0 if k is None else int(res["pearsonr"]["n_defined"][k])
    return out


def _check_type(name, args):
    mm = getattr(args, "multimodal_type", None)
    if mm not in CLS_TYPES:
        raise NotImplementedError(f"{name}: multimodal_type {mm!r} is not a regression fine-tune (only {', '.join(map(repr, CLS_TYPES))}); "
                                  "the contrastive loops are coem.train_one_epoch / coem.train_one_epoch_3modalities")
    return mm


def _forward(model, mm, batch, device, single_modality):
    """-> (logits, logit_scale, label on the device) for one loader item ({'oct', 'ir', 'f2_faf', 'label'}, (names, modalities, (h, true_idx)))"""
    x = batch[0]
    to = lambda t: t.to(device=device, non_blocking=True)
    label = to(x["label"]).float()
    images = to(x["oct"])
    if mm == "oct3d_paired_faf_ir_cls":
        out = model(images, to(x["ir"]), to(x["f2_faf"]), single_modality=single_modality)
    else:
        out = model(images, to(x["f2_faf"] if mm == "oct3d_paired_faf_cls" else x["ir"]))
    return out[0], out[1], label


def _scalar_prefix(prefix, fold):
    return f"{prefix}_fold_{fold}/" if fold != -1 else f"{prefix}/"


def train_one_epoch(model, data, epoch, optimizers, scaler, scheduler, args, tb_writer=None, reducers=None):
    """One epoch of the regression fine-tune in the reference's order of operations: ``data['train'].set_epoch(epoch)``, per batch
    ``scheduler(step)`` unless ``args.skip_scheduler``, forward, ``regression_loss``, backward, ``args.grad_clip_norm``, optimizer
    step(s), the ``logit_scale`` clamp, the reference's log line and ``tb_writer`` scalars under ``train/`` (``train_fold_{fold}/``);
    at the end of the epoch the per-column ``column_metrics`` over everything the epoch predicted, logged and written beside them.
    ``optimizers``: one optimizer or a list (one per tower arena, one for the classification head's, one for the temperatures);
    ``reducers``: coem.make_reducers.  Returns ``{"losses": [...], "micro_losses": [[...]], "steps": n, "logits": [N, C], "labels":
    [N, C]}`` (detached device tensors) plus the metrics."""
    name = "coem_finetune.train_one_epoch"
    coem._refuse_unsupported(name, scaler, args)
    mm = _check_type(name, args)
    if int(getattr(args, "accum_freq", 1)) != 1:
        raise NotImplementedError(f"{name}: the regression branch of the reference takes one optimizer step per batch (accum_freq 1)")
    optimizers = coem._optimizer_list(optimizers)
    device = torch.device(args.device)
    rank, world_size = getattr(args, "rank", 0), getattr(args, "world_size", 1)
    is_master = rank == 0
    clip = getattr(args, "grad_clip_norm", None)
    single = getattr(args, "single_modality", None)
    fold = getattr(args, "fold", -1)
    log_every = getattr(args, "log_every_n_steps", 100)
    prefix = _scalar_prefix("train", fold)
    model.train()
    data["train"].set_epoch(epoch)
    dataloader = data["train"].dataloader
    num_batches_per_epoch = dataloader.num_batches
    sample_digits = math.ceil(math.log(dataloader.num_samples + 1, 10))
    total_train_batch_size = args.batch_size * world_size
    record = {"losses": [], "micro_losses": [], "steps": 0}
    all_logits, all_labels = [], []
    loss_m, batch_time_m, data_time_m = coem.AverageMeter(), coem.AverageMeter(), coem.AverageMeter()
    end = time.time()
    step = num_batches_per_epoch * epoch
    for i, batch in enumerate(dataloader):
        step = num_batches_per_epoch * epoch + i
        if not getattr(args, "skip_scheduler", False):
            scheduler(step)
        data_time_m.update(time.time() - end)
        for o in optimizers:
            o.zero_grad()
        logits, logit_scale, label = _forward(model, mm, batch, device, single)
        total_loss = regression_loss(logits, label)
        if reducers:
            for r in reducers:
                r.begin_backward(sync=True)
        total_loss.backward()
        if reducers:
            for r in reducers:
                r.finish()
            coem._average_temperature_grads(model, reducers)
        if clip is not None:
            torch.nn.utils.clip_grad_norm_([p for p in model.parameters() if p.grad is not None], clip, norm_type=2.0)
        for o in optimizers:
            o.step()
        coem.clamp_logit_scale(model)
        total_loss = total_loss.detach()
        all_logits.append(logits.detach())
        all_labels.append(label)
        record["losses"].append(total_loss)
        record["micro_losses"].append([total_loss])
        record["steps"] += 1

        batch_time_m.update(time.time() - end)
        end = time.time()
        batch_count = i + 1
        # Departure: the reference's gate is `i_accum % log_every_n_steps or last batch`, which is true on every step that is NOT a multiple
        # -- two host reads on 99 of 100 steps at the default.  Here: every log_every_n_steps-th step and the last one.
        if is_master and (i % log_every == 0 or batch_count == num_batches_per_epoch):
            batch_size = label.shape[0]
            num_samples = batch_count * batch_size * world_size
            percent_complete = 100.0 * batch_count / num_batches_per_epoch
            # NOTE loss is coarsely sampled, just master node and per log update
            loss_m.update(total_loss.item(), batch_size)
            logit_scale_scalar = logit_scale.item()
            lr = optimizers[0].param_groups[0]["lr"]
            logging.info(
                f"Train Epoch: {epoch} [{num_samples:>{sample_digits}}/{dataloader.num_samples} ({percent_complete:.0f}%)] "
                f"Loss: {loss_m.val:#.5g} ({loss_m.avg:#.4g}) "
                f"Data (t): {data_time_m.avg:.3f} "
                f"Batch (t): {batch_time_m.avg:.3f}, {total_train_batch_size / batch_time_m.val:#g}/s "
                f"LR: {lr:5f} "
                f"Logit Scale: {logit_scale_scalar:.3f}")
            log_data = {"loss": loss_m.val, "data_time": data_time_m.val, "batch_time": batch_time_m.val,
                        "samples_per_second": total_train_batch_size / batch_time_m.val, "scale": logit_scale_scalar, "lr": lr}
            if tb_writer is not None:
                for key, val in log_data.items():
                    tb_writer.add_scalar(prefix + key, val, step)
            batch_time_m.reset()
            data_time_m.reset()
    if not all_logits:
        return record
    record["logits"], record["labels"] = torch.cat(all_logits), torch.cat(all_labels)
    if is_master:
        m = column_metrics(record["logits"], record["labels"])          # the epoch's one device-to-host copy
        for j in range(record["labels"].shape[1]):
            logging.info(", ".join(f"{k}_{j}: {m[f'{k}_{j}']}" for k in METRIC_KEYS))
        if tb_writer is not None:
            for key, val in m.items():
                tb_writer.add_scalar(prefix + key, val, step)
        record.update(m)
    return record


def _label_moments(dataset):
    mean, std = getattr(dataset, "preset_label_mean", None), getattr(dataset, "preset_label_std", None)
    if mean is None or std is None:
        mean, std = dataset.label_mean, dataset.label_std
    return (np.asarray(torch.as_tensor(mean).detach().cpu().numpy(), dtype=np.float32),
            np.asarray(torch.as_tensor(std).detach().cpu().numpy(), dtype=np.float32))


def evaluate(model, data, epoch, args, tb_writer=None, setting="val", dinfo_idx=0, return_prediction=False):
    """The regression branch of the reference's ``evaluate``: on the main process, when ``args.val_frequency`` says validation is due,
    run ``data[setting].dataloader`` (or ``data.dataloader``) without gradients; the loss is ``regression_loss`` per batch, weighted by
    batch size and summed on the device; logits and labels stay on the device until the loader is exhausted.  Returns ``{}`` off the
    main process or when validation is not due (also with ``return_prediction``, as the reference); otherwise ``column_metrics`` plus ``val_loss``, ``epoch``, ``num_samples`` -- with
    ``args.bootstrap`` = R > 0 also the keys of ``bootstrap_column_metrics`` (absent, None or 0: nothing changes) -- and, with
    ``return_prediction``, a second dict of the de-normalised ``original_labels`` / ``original_logits`` (float32: value * std + mean,
    with the dataset's ``preset_label_mean`` / ``preset_label_std``, else its ``label_mean`` / ``label_std``) and ``original_true_idx``.
    ``args.save_logs``: the scalars go to ``tb_writer`` under the reference's names, one line to
    ``results-{setting}-{dinfo_idx}[_fold_k].jsonl`` and one ``{target}.json`` per column to
    ``log_{setting}/{setting}_dataset_{i}/fold_{fold}/epoch_{epoch-1}/`` under ``args.checkpoint_path`` (the reference's ``plot_name``
    lists; its pickles, scatter plots, wandb and zero-shot evaluation are not part of this package)."""
    from . import misc
    if setting not in ("val", "test", "independent_test"):
        raise ValueError(f"evaluate: setting must be 'val', 'test' or 'independent_test', got {setting!r}")
    metrics = {}
    if getattr(args, "rank", 0) != 0 or not misc.is_main_process():
        return metrics
    name = "coem_finetune.evaluate"
    coem._refuse_unsupported(name, None, args)
    mm = _check_type(name, args)
    val_frequency = getattr(args, "val_frequency", 0)
    if not (val_frequency and ((epoch % val_frequency) == 0 or epoch == getattr(args, "epochs", None))):
        return metrics
    device = torch.device(getattr(args, "device", "cuda"))
    fold = getattr(args, "fold", -1)
    single = getattr(args, "single_modality", None)
    model.eval()
    dataloader = data[setting].dataloader if isinstance(data, dict) else data.dataloader
    samples_per_val = getattr(dataloader, "num_samples", None)
    label_mean, label_std = _label_moments(dataloader.dataset)
    num_samples = 0
    cumulative_loss = torch.zeros((), dtype=torch.float32, device=device)
    all_logits, all_labels, all_true_idx = [], [], []
    with torch.no_grad():
        for i, batch in enumerate(dataloader):
            all_true_idx.append(torch.as_tensor(batch[1][2][1]).reshape(-1))
            logits, _, label = _forward(model, mm, batch, device, single)
            batch_size = label.shape[0]
            cumulative_loss += regression_loss(logits, label) * batch_size
            all_logits.append(logits.float())
            all_labels.append(label)
            num_samples += batch_size
            if (i % 100) == 0:
                logging.info(f"Eval {setting}-{dinfo_idx} Epoch: {epoch} [{num_samples} / {samples_per_val}]")
    if num_samples == 0:
        raise ValueError("evaluate: the loader is empty")
    dev_logits, dev_labels = torch.cat(all_logits), torch.cat(all_labels)
    logits, labels = dev_logits.cpu().numpy(), dev_labels.cpu().numpy()
    metrics.update(column_metrics(logits, labels))
    if getattr(args, "bootstrap", None):
        metrics.update(bootstrap_column_metrics(dev_logits, dev_labels, metrics, args))
    metrics.update({"val_loss": float(cumulative_loss / num_samples), "epoch": epoch, "num_samples": num_samples})
    original_labels = labels.astype(np.float32) * label_std + label_mean
    original_logits = logits.astype(np.float32) * label_std + label_mean
    original_true_idx = torch.cat(all_true_idx).cpu().numpy()
    logging.info(f"Eval {setting}-{dinfo_idx} Epoch: {epoch} " + "\t".join(f"{k}: {round(v, 4):.4f}" for k, v in metrics.items()))
    if getattr(args, "save_logs", False):
        pre = ""
        if fold != -1:
            pre = {"val": f"val_fold_{fold}/", "test": f"test_dataset_{dinfo_idx}_fold_{fold}/",
                   "independent_test": f"independent_test_dataset_{dinfo_idx}_fold_{fold}/"}[setting]
        if tb_writer is not None:
            for key, val in metrics.items():
                tb_writer.add_scalar(f"{setting}-{dinfo_idx}/{pre}{key}", val, epoch)
        result_name = f"results-{setting}-{dinfo_idx}.jsonl" if fold == -1 else f"results-{setting}-{dinfo_idx}_fold_{fold}.jsonl"
        with open(os.path.join(args.checkpoint_path, result_name), "a+") as f:
            f.write(json.dumps(metrics))
            f.write("\n")
        cls_type = getattr(args, "cls_dataset_type", None)
        names, (lo, hi) = (PLOT_NAMES_GAGROWTH, PLOT_RANGES_GAGROWTH) if cls_type in GAGROWTH_TYPES else (PLOT_NAMES, PLOT_RANGES)
        if original_labels.shape[1] > len(names):
            raise ValueError(f"evaluate: {original_labels.shape[1]} target columns, cls_dataset_type {cls_type!r} names {len(names)}")
        folder = os.path.join(args.checkpoint_path, f"log_{setting}", f"{setting}_dataset_{dinfo_idx if setting != 'val' else 0}",
                              f"fold_{fold}", f"epoch_{epoch - 1}")
        os.makedirs(folder, exist_ok=True)
        for j in range(original_labels.shape[1]):
            yt, yp = original_labels[:, j].astype(np.float64), original_logits[:, j].astype(np.float64)
            poly = np.polyfit(yt, yp, 1).tolist() if yt.size >= 2 and np.ptp(yt) > 0 else [float("nan"), float("nan")]
            save = {"label": names[j], "min_val": int(lo[j]), "max_val": int(hi[j]), "epoch": epoch, "actual_epoch": epoch - 1, "fold": fold,
                    "cls_dataset_type": cls_type, "poly_coef": poly, "true_idx": original_true_idx.tolist(),
                    "y_true": original_labels[:, j].tolist(), "y_pred": original_logits[:, j].tolist()}
            with open(os.path.join(folder, f"{names[j]}.json"), "w") as f:
                json.dump(save, f, indent=2)
    if return_prediction:
        return metrics, {"original_labels": original_labels, "original_logits": original_logits, "original_true_idx": original_true_idx}
    return metrics
