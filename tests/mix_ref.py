"""Reference for the mixup / cutmix tests: timm's ``_mix_batch``, ``_mix_elem``, ``_mix_pair`` and ``mixup_target`` restated in plain torch
with the clone of the batch and the per-sample Python loop, on the CPU in float32.  The random decisions are ARGUMENTS (timm draws them
inside), so the same decisions can be handed to this file and to the kernel.  One departure, the package's own (octcubem_amd/mixup.py):
the box is cut over the last two dimensions, ``x[..., yl:yh, xl:xh]``, also for 5-D input.

``lam`` keeps the type the mode gives it -- a Python float in batch mode, numpy float32 values in elem and pair mode -- because
``1 - lam`` is a double subtraction for the one and a float32 subtraction for the other."""
import numpy as np
import torch


def mix_batch(x, lam, use_cutmix, box=None):
    """In place; one decision for the whole batch.  ``lam == 1``: untouched."""
    if lam == 1.0:
        return x
    if use_cutmix:
        yl, yh, xl, xh = box
        x[..., yl:yh, xl:xh] = x.flip(0)[..., yl:yh, xl:xh]
    else:
        x_flipped = x.flip(0).mul_(1.0 - lam)
        x.mul_(lam).add_(x_flipped)
    return x


def mix_elem(x, lam, use_cutmix, boxes):
    """In place; one decision per sample (``lam`` float32 [B], ``use_cutmix`` bool [B], ``boxes`` [B] of (yl, yh, xl, xh))."""
    B = len(x)
    x_orig = x.clone()
    for i in range(B):
        j = B - i - 1
        l = lam[i]
        if l != 1.0:
            if use_cutmix[i]:
                yl, yh, xl, xh = boxes[i]
                x[i][..., yl:yh, xl:xh] = x_orig[j][..., yl:yh, xl:xh]
            else:
                x[i] = x[i] * l + x_orig[j] * (1 - l)
    return x


def mix_pair(x, lam, use_cutmix, boxes):
    """In place; one decision per pair (i, B - 1 - i), ``lam`` / ``use_cutmix`` / ``boxes`` of length B / 2."""
    B = len(x)
    x_orig = x.clone()
    for i in range(B // 2):
        j = B - i - 1
        l = lam[i]
        if l != 1.0:
            if use_cutmix[i]:
                yl, yh, xl, xh = boxes[i]
                x[i][..., yl:yh, xl:xh] = x_orig[j][..., yl:yh, xl:xh]
                x[j][..., yl:yh, xl:xh] = x_orig[i][..., yl:yh, xl:xh]
            else:
                x[i] = x[i] * l + x_orig[j] * (1 - l)
                x[j] = x[j] * l + x_orig[i] * (1 - l)
    return x


def one_hot(t, num_classes, on_value=1.0, off_value=0.0):
    t = t.long().view(-1, 1)
    return torch.full((t.size(0), num_classes), off_value).scatter_(1, t, on_value)


def mixup_target(target, num_classes, lam=1.0, smoothing=0.0):
    """``lam``: a float, or per-sample values [B] (made a float32 [B, 1] column, as the elem and pair modes do)."""
    off_value = smoothing / num_classes
    on_value = 1.0 - smoothing + off_value
    y1 = one_hot(target, num_classes, on_value, off_value)
    y2 = one_hot(target.flip(0), num_classes, on_value, off_value)
    if not isinstance(lam, float):
        lam = torch.tensor(np.asarray(lam), dtype=torch.float32).unsqueeze(1)
    return y1 * lam + y2 * (1.0 - lam)


def apply_params(x, target, p, num_classes, smoothing):
    """Mix a CPU copy of ``x`` / ``target`` by the decisions ``p`` that ``Mixup.last_params`` recorded."""
    x = x.detach().cpu().clone()
    boxes = [tuple(int(v) for v in b) for b in p["box"]]
    if p["mode"] == "batch":
        mix_batch(x, p["lam_mix"], p["use_cutmix"], boxes[0])
    elif p["mode"] == "elem":
        mix_elem(x, p["lam_mix"], p["use_cutmix"], boxes)
    else:
        h = len(x) // 2
        mix_pair(x, p["lam_mix"][:h], p["use_cutmix"][:h], boxes[:h])
    return x, mixup_target(target.cpu(), num_classes, p["lam"], smoothing)
