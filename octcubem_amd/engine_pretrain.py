"""Pre-training inner loops with the reference's signatures: ``train_one_epoch`` (3-D volumes only) and
``train_one_epoch_joint`` (3-D volumes + 2-D/512 B-scans, per-frame loss feedback for self-paced sampling) plus the two
epoch schedules of the joint recipe, ``eval_one_epoch``, the validation pass with its reconstruction dumps (3-D, and the 2-D half of
the joint recipe), and ``eval_one_epoch_2d``, the validation pass of the 2-D MAE.

``train_one_epoch``: pre-training inner loop with the reference's signature and per-iteration order of operations
(OCTCube/engine_pretrain.py:31-91; Pre-training/engine_pretrain.py:29-204 is the same loop plus the 2-D branch):
per-iteration LR schedule -> H2D -> forward -> non-finite guard -> loss_scaler(backward / [all-reduce] / clip / step)
-> zero_grad -> logging.  The dead ``get_mask`` work of the 3-D engine (its result is dropped by forward) and the
per-iteration full-device synchronise are not reproduced; a single ``loss.item()`` per iteration remains (it is the
reference's non-finite guard).

Provenance, stated once: this file is a RESTATEMENT of the reference's host loop, written to be call-compatible with it -- same
function signatures, same order of operations per iteration, same ``MetricLogger`` keys -- because it is the caller SURVEY section 8
(R14 / N1, N3) requires and the reference's drivers import it by name.  It holds no kernel logic; everything it calls (models, scaler,
optimizer, schedules) is this package's own."""
from __future__ import annotations

import math
import os
import sys
from typing import Iterable

import torch

from . import lr_sched, misc


def train_one_epoch(model: torch.nn.Module, data_loader: Iterable, optimizer: torch.optim.Optimizer, device: torch.device,
                    epoch: int, loss_scaler, log_writer=None, args=None, noise_fn=None):
    model.train(True)
    metric_logger = misc.MetricLogger(delimiter="  ")
    metric_logger.add_meter("lr", misc.SmoothedValue(window_size=1, fmt="{value:.6f}"))
    header = "Epoch: [{}]".format(epoch)
    print_freq = 20
    accum_iter = args.accum_iter
    optimizer.zero_grad()
    n_iter = len(data_loader)
    for data_iter_step, batch in enumerate(metric_logger.log_every(misc.prefetched(data_loader, device, args), print_freq, header)):
        samples = batch[0] if isinstance(batch, (tuple, list)) else batch
        if data_iter_step % accum_iter == 0:
            lr_sched.adjust_learning_rate(optimizer, data_iter_step / n_iter + epoch, args)
        samples = samples.to(device, non_blocking=True)
        if samples.dim() == 6:
            b, r, c, t, h, w = samples.shape
            samples = samples.reshape(b * r, c, t, h, w)
        noise = noise_fn(samples) if noise_fn is not None else None
        loss, _, _ = model(samples, mask_ratio=args.mask_ratio, noise=noise) if noise is not None else \
            model(samples, mask_ratio=args.mask_ratio)
        loss_value = loss.item()
        if not math.isfinite(loss_value):
            print("Loss is {}, stopping training".format(loss_value))
            sys.exit(1)
        loss = loss / accum_iter
        loss_scaler(loss, optimizer, parameters=model.parameters(), update_grad=(data_iter_step + 1) % accum_iter == 0,
                    clip_grad=getattr(args, "clip_grad", None))
        if (data_iter_step + 1) % accum_iter == 0:
            optimizer.zero_grad()
        metric_logger.update(loss=loss_value)
        lr = optimizer.param_groups[0]["lr"]
        metric_logger.update(lr=lr)
        loss_value_reduce = misc.all_reduce_mean(loss_value)
        if log_writer is not None and (data_iter_step + 1) % accum_iter == 0:
            epoch_1000x = int((data_iter_step / n_iter + epoch) * 1000)
            log_writer.add_scalar("train_loss", loss_value_reduce, epoch_1000x)
            log_writer.add_scalar("lr", lr, epoch_1000x)
    metric_logger.synchronize_between_processes()
    print("Averaged stats:", metric_logger)
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


def K_scheduler(epoch, K_max=0.7, K_min=0.3, all_epoch=100, warmup_epochs=10, epoch_offset=0):
    """Self-paced-learning keep fraction K (main_pretrain_oph_joint_2d512_flash_attn.py:53-59): K_max through the warm-up, then
    linearly down to K_min at ``all_epoch``."""
    num_epochs = epoch - epoch_offset
    if num_epochs <= warmup_epochs:
        return K_max
    return K_max - (num_epochs - warmup_epochs) * (K_max - K_min) / (all_epoch - warmup_epochs - epoch_offset)


def mask_ratio_2d_scheduler(epoch, mask_ratio_max=0.85, mask_ratio_min=0.75, all_epoch=100, warmup_epochs=10, epoch_offset=0):
    """Mask ratio of the 2-D branch (:61-67): mask_ratio_min through the warm-up, then linearly up to mask_ratio_max."""
    num_epochs = epoch - epoch_offset
    if num_epochs <= warmup_epochs:
        return mask_ratio_min
    return mask_ratio_min + (num_epochs - warmup_epochs) * (mask_ratio_max - mask_ratio_min) / (all_epoch - warmup_epochs - epoch_offset)


def record_frame_losses(frame_loss, data_dict, dataset_2d_all_image_dict, cube_size=3):
    """Per-frame loss feedback of the joint loop (Pre-training/engine_pretrain.py:133-146): every temporal patch group's masked
    MSE is written to the ``mse_loss`` / ``hardness`` fields of the ``cube_size`` frames it covers (the 2-D dataset samples
    by hardness).  ``frame_loss``: [N, T / t_patch]; ``data_dict['frames'][nf][j]`` = name of frame nf of volume j.
    One device->host copy instead of one ``.item()`` per frame."""
    fl = frame_loss.detach().float().cpu().tolist()
    n_frames = len(data_dict["frames"])
    for j, vol in enumerate(fl):
        names = [data_dict["frames"][nf][j] for nf in range(n_frames)]
        for k, v in enumerate(vol):
            for fr in range(cube_size):
                e = dataset_2d_all_image_dict[names[k * cube_size + fr]]
                e["mse_loss"] = v
                e["hardness"] = v
        e = dataset_2d_all_image_dict[names[-1]]
        e["mse_loss"] = vol[-1]
        e["hardness"] = vol[-1]


def train_one_epoch_joint(model: torch.nn.Module, data_loader: Iterable, optimizer: torch.optim.Optimizer, device: torch.device,
                          epoch: int, loss_scaler, data_loader_2d, dataset_2d_all_image_dict, mask_ratio_2d, log_writer=None,
                          args=None, fp32=False, fp16=False, noise_fn=None):
    """Joint 3-D + 2-D/512 pre-training epoch (Pre-training/engine_pretrain.py:29-204): per iteration one volume batch
    (``frame_loss=True``) and one batch of ``(B, C, 3, 512, 512)`` B-scan triplets through ``high_res_patch_embed``, the two
    losses summed before a single backward; the 2-D loader restarts when exhausted.  ``data_loader`` yields
    ``(samples, (img_names, data_dict))``.  Same omissions as ``train_one_epoch`` (the dropped ``get_mask`` result, the
    per-iteration device synchronise); ``fp32`` / ``fp16`` are accepted and ignored (bf16 operands, fp32 everything else).
    Both forwards feed the same parameters, so a parameter reports its gradient once per use: the data-parallel reducer learns
    the number of reports per parameter in the first exchanged backward (run without overlap) and overlaps from then on."""
    model.train(True)
    net = getattr(model, "module", model)
    reducer = getattr(loss_scaler, "reducer", None)
    if reducer is not None:
        reducer.multi_use = True
    metric_logger = misc.MetricLogger(delimiter="  ")
    for name in ("lr", "mask_ratio", "mask_ratio_2d"):
        metric_logger.add_meter(name, misc.SmoothedValue(window_size=1, fmt="{value:.6f}"))
    metric_logger.add_meter("loss_2d", misc.SmoothedValue(window_size=1))
    metric_logger.add_meter("loss_all", misc.SmoothedValue(window_size=1))
    header = "Epoch: [{}]".format(epoch)
    print_freq = 20
    accum_iter = args.accum_iter
    optimizer.zero_grad()
    n_iter = len(data_loader)
    secondary_iter = iter(data_loader_2d)
    for data_iter_step, (samples, data_info) in enumerate(metric_logger.log_every(misc.prefetched(data_loader, device, args), print_freq, header)):
        if data_iter_step % accum_iter == 0:
            lr_sched.adjust_learning_rate(optimizer, data_iter_step / n_iter + epoch, args)
        data_dict = data_info[1]
        try:
            secondary_data = next(secondary_iter)
        except StopIteration:
            secondary_iter = iter(data_loader_2d)
            secondary_data = next(secondary_iter)
        sample_2d = secondary_data[0].to(device, non_blocking=True)
        samples = samples.to(device, non_blocking=True)
        if samples.dim() == 6:
            b, r, c, t, h, w = samples.shape
            samples = samples.reshape(b * r, c, t, h, w)
        kw3 = {"noise": noise_fn(samples)} if noise_fn is not None else {}
        (loss, frame_loss), _, _ = net(samples, mask_ratio=args.mask_ratio, frame_loss=True, **kw3)
        kw2 = {"noise": noise_fn(sample_2d)} if noise_fn is not None else {}
        loss_2d, _, _ = net(sample_2d, mask_ratio=mask_ratio_2d, **kw2)
        loss_value, loss_2d_value = loss.item(), loss_2d.item()
        record_frame_losses(frame_loss, data_dict, dataset_2d_all_image_dict)
        loss = loss + loss_2d
        loss_all_value = loss_value + loss_2d_value
        if not math.isfinite(loss_value):
            raise Exception("Loss is {}, stopping training".format(loss_value))
        loss = loss / accum_iter
        loss_scaler(loss, optimizer, parameters=net.parameters(), update_grad=(data_iter_step + 1) % accum_iter == 0,
                    clip_grad=getattr(args, "clip_grad", None))
        if (data_iter_step + 1) % accum_iter == 0:
            optimizer.zero_grad()
        metric_logger.update(loss=loss_value, mask_ratio=args.mask_ratio, loss_2d=loss_2d_value, loss_all=loss_all_value,
                             mask_ratio_2d=mask_ratio_2d)
        lr = optimizer.param_groups[0]["lr"]
        metric_logger.update(lr=lr)
        loss_value_reduce = misc.all_reduce_mean(loss_value)
        if log_writer is not None and (data_iter_step + 1) % accum_iter == 0:
            epoch_1000x = int((data_iter_step / n_iter + epoch) * 1000 * getattr(args, "repeat_aug", 1))
            log_writer.add_scalar("train_loss", loss_value_reduce, epoch_1000x)
            log_writer.add_scalar("lr", lr, epoch_1000x)
    metric_logger.synchronize_between_processes()
    print("Averaged stats:", metric_logger)
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


@torch.no_grad()
def eval_one_epoch(model: torch.nn.Module, data_loader: Iterable, device: torch.device, epoch: int, log_writer=None, args=None,
                   fp32=False, joint=False, mask_ratio_2d=None, data_loader_2d=None, visible_frame_freq=20, all_image_dict=None,
                   analysis=False, fp16=False, agg_data=False):
    """Validation pass (Pre-training/engine_pretrain.py:207-357) with the reference's signature and order of operations: eval mode,
    no grad, per batch ``loss, pred, mask = model(samples, mask_ratio=args.mask_ratio)`` -> non-finite guard -> on the main process,
    every ``print_freq * visible_frame_freq``-th step, the reconstruction dump of that batch into
    ``args.output_dir/val_images_<epoch>`` (misc.get_visible_images) -> ``loss`` / ``mask_ratio`` meters, ``val_loss`` to the writer.
    ``data_loader`` yields ``(samples, img_names)``.  Returns the averaged stats, or None on a non-finite loss (as engine_finetune).
    Not reproduced: the per-step device synchronise, ``forward_patch_embed`` / ``get_patch_embed_images`` (analysis output nothing
    reads) and the checkpoint deletion on a non-finite loss; ``all_image_dict``, ``analysis``, ``agg_data`` and ``fp32`` / ``fp16``
    (bf16 operands, fp32 everything else) are accepted and ignored.  ``joint`` picks ``img_names[0]`` as there.
    With ``joint`` and a ``data_loader_2d``, every dump step also does what :298-322 does: the next batch of the 2-D loader (which
    restarts when exhausted, as in ``train_one_epoch_joint``; the reference's bare ``next`` raises StopIteration there) goes to the
    device, its bright borders are blanked (misc.blank_white_borders: the reference's per-sample find_and_convert_large_white_region
    loop as two launches), the model runs on it with ``mask_ratio_2d`` and misc.get_visible_images_2d writes
    ``val_images_<epoch>/visible_2d/<name>`` under the names ``batch[1][-1]``.  The 2-D loss enters no meter: the returned stats are
    those of the 3-D loader alone, as in the reference.
    The pass leaves ``.grad`` as it found it: the parameter arena attaches its gradient views when a model's first forward creates it
    (octcubem_amd/arena.py), also under no_grad; parameters that came in without a gradient go out without one, and the next forward
    with grad enabled re-attaches the views (``arena.rebind_grads``).  Nothing computes a gradient inside the pass, so a parameter that
    came in with a gradient keeps it untouched, and a model without an arena is left exactly as it was."""
    no_grad_at_entry = [p for p in model.parameters() if p.grad is None]
    try:
        return _eval_one_epoch(model, data_loader, device, epoch, log_writer, args, joint, visible_frame_freq,
                               data_loader_2d if joint else None, mask_ratio_2d)
    finally:
        for p in no_grad_at_entry:
            p.grad = None


def _eval_one_epoch(model, data_loader, device, epoch, log_writer, args, joint, visible_frame_freq, data_loader_2d=None,
                    mask_ratio_2d=None):
    img_save_dir = os.path.join(args.output_dir, f"val_images_{epoch}")
    os.makedirs(img_save_dir, exist_ok=True)
    model.eval()
    metric_logger = misc.MetricLogger(delimiter="  ")
    metric_logger.add_meter("mask_ratio", misc.SmoothedValue(window_size=1, fmt="{value:.6f}"))
    header = "Epoch: [{}]".format(epoch)
    print_freq = 20
    accum_iter = args.accum_iter
    n_iter = len(data_loader)
    secondary_iter = iter(data_loader_2d) if data_loader_2d is not None else None
    for data_iter_step, (samples, img_names) in enumerate(metric_logger.log_every(data_loader, print_freq, header)):
        samples = samples.to(device, non_blocking=True)
        if samples.dim() == 6:
            b, r, c, t, h, w = samples.shape
            samples = samples.reshape(b * r, c, t, h, w)
        loss, pred, mask = model(samples, mask_ratio=args.mask_ratio)
        loss_value = loss.item()
        if not math.isfinite(loss_value):
            print("Loss is {}, stopping evaluation".format(loss_value))
            return None
        if data_iter_step % (print_freq * visible_frame_freq) == 0 and misc.is_main_process():
            if joint:
                img_names = img_names[0]
            vars_ = {"reconstruct_imgs": pred, "samples": samples, "mask": mask, "img_names": img_names}
            misc.get_visible_images(vars_, model, img_save_dir)
            if secondary_iter is not None:
                try:
                    secondary_data = next(secondary_iter)
                except StopIteration:
                    secondary_iter = iter(data_loader_2d)
                    secondary_data = next(secondary_iter)
                img_names_2d = secondary_data[1][-1]
                sample_2d, pre_mask = misc.blank_white_borders(secondary_data[0].to(device, non_blocking=True))
                _, pred_2d, mask_2d = model(sample_2d, mask_ratio=mask_ratio_2d)
                vars_2d_ = {"reconstruct_imgs": pred_2d, "samples": sample_2d, "mask": mask_2d, "img_names": img_names_2d,
                            "pre_mask": pre_mask}
                misc.get_visible_images_2d(vars_2d_, model, img_save_dir)
        metric_logger.update(loss=loss_value)
        metric_logger.update(mask_ratio=args.mask_ratio)
        loss_value_reduce = misc.all_reduce_mean(loss_value)
        if log_writer is not None and (data_iter_step + 1) % accum_iter == 0:
            epoch_1000x = int((data_iter_step / n_iter + epoch) * 1000 * getattr(args, "repeat_aug", 1))
            log_writer.add_scalar("val_loss", loss_value_reduce, epoch_1000x)
    metric_logger.synchronize_between_processes()
    print("Averaged stats:", metric_logger)
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


def cover_one_epoch(model: torch.nn.Module, data_loader: Iterable, device: torch.device, epoch: int, args=None, mask_ratio=None,
                    generator=None, save_volumes=0):
    """Full-coverage reconstruction over a validation loader (no counterpart in the reference): per batch, in the form
    ``eval_one_epoch`` takes them (``(samples, img_names)``, a 6-D batch folded into the batch axis, a bare tensor accepted),
    ``model.reconstruct_full(samples, mask_ratio, generator)`` -- every voxel predicted while hidden, and its squared error against
    the scan.  One row per volume is appended to ``args.output_dir/cover_scores_<epoch>.csv``: ``index,name,volume_score,
    max_frame_score,max_frame`` (the name is empty where the batch carries none).  ``mask_ratio=None`` means ``args.mask_ratio``.
    ``save_volumes = n`` also writes ``recon`` and ``error`` of the first n volumes to ``cover_volumes_<epoch>.npz``.  Returns
    ``{"volume_score": float64 [V], "frame_score": float64 [V, Tp], "max_frame": int64 [V], "names": [...], "loss": the mean of all
    passes' losses}`` as numpy arrays.  ``reconstruct_full`` leaves the training flag and ``.grad`` as found."""
    import numpy as np
    inner = getattr(model, "module", model)
    if mask_ratio is None:
        mask_ratio = args.mask_ratio
    os.makedirs(args.output_dir, exist_ok=True)
    path = os.path.join(args.output_dir, f"cover_scores_{epoch}.csv")
    vol, frm, names, losses, kept = [], [], [], [], {"recon": [], "error": []}
    new_file = not os.path.exists(path)
    with open(path, "a") as f:
        if new_file:
            f.write("index,name,volume_score,max_frame_score,max_frame\n")
        for batch in data_loader:
            samples, img_names = (batch[0], batch[1]) if isinstance(batch, (tuple, list)) else (batch, None)
            samples = samples.to(device, non_blocking=True)
            if samples.dim() == 6:
                b, r, c, t, h, w = samples.shape
                samples = samples.reshape(b * r, c, t, h, w)
            n = samples.shape[0]
            if img_names is None or isinstance(img_names, str) or len(img_names) != n:
                img_names = [""] * n
            out = inner.reconstruct_full(samples, mask_ratio=mask_ratio, generator=generator, error_volume=True)
            vs, fs = out["volume_score"].cpu().numpy(), out["frame_score"].cpu().numpy()
            losses += out["losses"]
            for i in range(n):
                k = int(fs[i].argmax())
                f.write(f"{len(vol)},{str(img_names[i]).replace(',', ';')},{float(vs[i])!r},{float(fs[i, k])!r},{k}\n")
                if len(vol) < save_volumes:
                    kept["recon"].append(out["recon"][i].cpu().numpy())
                    kept["error"].append(out["error"][i].cpu().numpy())
                vol.append(float(vs[i])); frm.append(fs[i]); names.append(str(img_names[i]))
    if save_volumes > 0 and kept["recon"]:
        np.savez_compressed(os.path.join(args.output_dir, f"cover_volumes_{epoch}.npz"), recon=np.stack(kept["recon"]),
                            error=np.stack(kept["error"]), names=np.array(names[:len(kept["recon"])]))
    frame = np.stack(frm) if frm else np.zeros((0, 0))
    return {"volume_score": np.asarray(vol, dtype=np.float64), "frame_score": frame,
            "max_frame": frame.argmax(axis=1) if frm else np.zeros((0,), dtype=np.int64), "names": names,
            "loss": float(np.mean(losses)) if losses else float("nan")}


IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@torch.no_grad()
def eval_one_epoch_2d(model: torch.nn.Module, data_loader: Iterable, device: torch.device, epoch: int, log_writer=None, args=None,
                      visible_frame_freq=20, inverse_imagenet_transform=None, **ignored):
    """Validation pass of the 2-D MAE (models_mae_2d): the primary path of OCTCube/engine_pretrain.py:172-330, that file's
    ``eval_one_epoch``, under a name of its own because this module's ``eval_one_epoch`` is the 3-D / joint one.  Per batch
    ``loss, pred, mask = model(samples, mask_ratio=args.mask_ratio)`` on [B, C, H, W] images -> non-finite guard (returns None, as
    ``eval_one_epoch``) -> on the main process, when ``(step + 1) % (20 * visible_frame_freq) == 0`` (this file's condition, one step
    later than the other one's), the panels of the WHOLE batch into ``args.output_dir/val_images_<epoch>/visible_2d/<name>``
    (misc.get_visible_images_2d) -> ``loss`` / ``mask_ratio`` meters, ``val_loss`` to the writer.  ``data_loader`` yields
    ``(samples, img_names)``.  Departures: the reference indexes ``img_names[0]`` and then takes the ``len`` of that string, so it
    draws as many images as the first name has characters; here every image of the batch is drawn under its own name.  With
    ``inverse_imagenet_transform`` (any value but None, as there) the levels are those of the inverse ImageNet Normalize
    (``v * std + mean``, in the kernel) instead of the raw ones.  The joint branch of that function (it can never run with a 2-D
    model) and ``fp32`` / ``fp16`` / ``analysis`` / ``all_image_dict`` are accepted through ``**ignored``.  ``.grad`` is left as
    ``eval_one_epoch`` leaves it."""
    no_grad_at_entry = [p for p in model.parameters() if p.grad is None]
    try:
        return _eval_one_epoch_2d(model, data_loader, device, epoch, log_writer, args, visible_frame_freq,
                                  inverse_imagenet_transform is not None)
    finally:
        for p in no_grad_at_entry:
            p.grad = None


def _eval_one_epoch_2d(model, data_loader, device, epoch, log_writer, args, visible_frame_freq, imagenet):
    img_save_dir = os.path.join(args.output_dir, f"val_images_{epoch}")
    os.makedirs(img_save_dir, exist_ok=True)
    model.eval()
    metric_logger = misc.MetricLogger(delimiter="  ")
    metric_logger.add_meter("mask_ratio", misc.SmoothedValue(window_size=1, fmt="{value:.6f}"))
    header = "Epoch: [{}]".format(epoch)
    print_freq = 20
    accum_iter = args.accum_iter
    n_iter = len(data_loader)
    for data_iter_step, (samples, img_names) in enumerate(metric_logger.log_every(data_loader, print_freq, header)):
        samples = samples.to(device, non_blocking=True)
        loss, pred, mask = model(samples, mask_ratio=args.mask_ratio)
        loss_value = loss.item()
        if not math.isfinite(loss_value):
            print("Loss is {}, stopping evaluation".format(loss_value))
            return None
        if (data_iter_step + 1) % (print_freq * visible_frame_freq) == 0 and misc.is_main_process():
            vars_ = {"reconstruct_imgs": pred, "samples": samples, "mask": mask, "img_names": img_names}
            if imagenet:
                vars_.update(mean=IMAGENET_MEAN, std=IMAGENET_STD)
            misc.get_visible_images_2d(vars_, model, img_save_dir)
        metric_logger.update(loss=loss_value)
        metric_logger.update(mask_ratio=args.mask_ratio)
        loss_value_reduce = misc.all_reduce_mean(loss_value)
        if log_writer is not None and (data_iter_step + 1) % accum_iter == 0:
            epoch_1000x = int((data_iter_step / n_iter + epoch) * 1000)
            log_writer.add_scalar("val_loss", loss_value_reduce, epoch_1000x)
    metric_logger.synchronize_between_processes()
    print("Averaged stats:", metric_logger)
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}
