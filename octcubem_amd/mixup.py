"""Mixup / cutmix for the fine-tune loop: the ``mixup_fn`` that ``engine_finetune.train_one_epoch`` calls on device tensors and whose soft
targets ``losses.SoftTargetCrossEntropy`` consumes.  The reference's drivers build it from ``timm.data.Mixup`` (for example
OCTCube/main_finetune_downstream_inhouse_singlefold.py:448-455); timm is not a dependency here, so this is the published rule written
out for this package: same constructor arguments, same ``__call__(x, target) -> (x, target)``, the same decisions in the same order of
draws from numpy's legacy random stream.  The decisions are made on the host and become four small tables; the volumes are mixed in
place by one launch of csrc/mixup.hip (ops.mix_batch), the ``[B, num_classes]`` targets by a few torch ops on the device.

Departure from timm, on purpose: for 5-D input ``[B, C, T, H, W]`` the box is cut over (H, W) in every channel and frame.  timm's
``x[:, :, yl:yh, xl:xh]`` would cut (T, H) there with a box it drew for (H, W).  For 4-D input there is no difference."""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from ._autocast import no_autocast

KIND_NONE, KIND_MIXUP, KIND_CUTMIX = 0, 1, 2


def one_hot(target: torch.Tensor, num_classes: int, on_value: float = 1.0, off_value: float = 0.0) -> torch.Tensor:
    t = target.long().view(-1, 1)
    return torch.full((t.shape[0], num_classes), off_value, device=t.device).scatter_(1, t, on_value)


def mixup_target(target: torch.Tensor, num_classes: int, lam=1.0, smoothing: float = 0.0) -> torch.Tensor:
    """``onehot(t) * lam + onehot(t.flip(0)) * (1 - lam)`` with the smoothed one-hot values off = smoothing / num_classes and
    on = 1 - smoothing + off; ``lam`` a float or a ``[B, 1]`` tensor."""
    off = smoothing / num_classes
    on = 1.0 - smoothing + off
    y1 = one_hot(target, num_classes, on, off)
    y2 = one_hot(target.flip(0), num_classes, on, off)
    return y1 * lam + y2 * (1.0 - lam)


class Mixup:
    """timm's ``Mixup``: per batch (``mode='batch'``), per sample (``'elem'``) or per pair of samples (``'pair'``) either blend sample i
    with sample B - 1 - i (lam ~ Beta(mixup_alpha, mixup_alpha)) or paste a box of it (lam ~ Beta(cutmix_alpha, cutmix_alpha), box of
    area ratio 1 - lam around a uniform centre, or of side ratios drawn from ``cutmix_minmax``), with probability ``prob``; where both
    alphas are positive, cutmix with probability ``switch_prob``.  ``correct_lam`` replaces a cutmix lam by 1 - area / (H W) of the box
    actually cut (always with ``cutmix_minmax``).  Targets become the lam-weighted smoothed one-hot vectors.

    ``x``: float32 GPU tensor ``[B, C, H, W]`` or ``[B, C, T, H, W]``, B even; anything else raises ValueError.  A contiguous ``x`` is
    modified in place and returned; any other is made contiguous first (the result is then a new tensor).  ``rng``: a
    ``numpy.random.RandomState``; None draws from numpy's global state, as timm does.  ``last_params`` holds the decisions of the
    last call (mode, kind / lam / oml / box tables as launched, ``use_cutmix``, ``lam_mix`` as drawn and ``lam`` as it weights the
    targets).  Autocast changes nothing."""

    def __init__(self, mixup_alpha=1.0, cutmix_alpha=0.0, cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode="batch", correct_lam=True,
                 label_smoothing=0.1, num_classes=1000, rng=None):
        if mode not in ("batch", "elem", "pair"):
            raise ValueError(f"Mixup: mode must be 'batch', 'elem' or 'pair', got {mode!r}")
        self.mixup_alpha = mixup_alpha
        self.cutmix_alpha = cutmix_alpha
        self.cutmix_minmax = cutmix_minmax
        if cutmix_minmax is not None:
            if len(cutmix_minmax) != 2:
                raise ValueError("Mixup: cutmix_minmax is a (min, max) pair of side ratios")
            self.cutmix_alpha = 1.0           # the box no longer depends on lam; cutmix must be switched on
        self.mix_prob = prob
        self.switch_prob = switch_prob
        self.mode = mode
        self.correct_lam = correct_lam
        self.label_smoothing = label_smoothing
        self.num_classes = num_classes
        self.mixup_enabled = True             # timm's drivers clear it to switch the augmentation off late in training
        self.rng = rng
        self.last_params = None

    # ---- decisions (host) ------------------------------------------------------------------------------
    def _rng(self):
        return np.random if self.rng is None else self.rng

    def _draw_lam(self, size=None):
        """(lam_mix, use_cutmix) for one decision (size None) or ``size`` of them: the switch first, then the beta draw(s)."""
        r = self._rng()
        if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
            use_cutmix = r.rand(*(() if size is None else (size,))) < self.switch_prob
            if size is None:
                lam_mix = r.beta(self.cutmix_alpha, self.cutmix_alpha) if use_cutmix else r.beta(self.mixup_alpha, self.mixup_alpha)
            else:
                lam_mix = np.where(use_cutmix, r.beta(self.cutmix_alpha, self.cutmix_alpha, size=size),
                                   r.beta(self.mixup_alpha, self.mixup_alpha, size=size))
        elif self.mixup_alpha > 0.0:
            use_cutmix = False if size is None else np.zeros(size, dtype=bool)
            lam_mix = r.beta(self.mixup_alpha, self.mixup_alpha, size=size)
        elif self.cutmix_alpha > 0.0:
            use_cutmix = True if size is None else np.ones(size, dtype=bool)
            lam_mix = r.beta(self.cutmix_alpha, self.cutmix_alpha, size=size)
        else:
            raise ValueError("Mixup: one of mixup_alpha > 0, cutmix_alpha > 0 or cutmix_minmax must be set")
        return lam_mix, use_cutmix

    def _params_per_batch(self):
        lam, use_cutmix = 1.0, False
        if self.mixup_enabled and self._rng().rand() < self.mix_prob:
            lam_mix, use_cutmix = self._draw_lam()
            lam, use_cutmix = float(lam_mix), bool(use_cutmix)
        return lam, use_cutmix

    def _params_per_elem(self, n):
        lam = np.ones(n, dtype=np.float32)
        use_cutmix = np.zeros(n, dtype=bool)
        if self.mixup_enabled:
            lam_mix, use_cutmix = self._draw_lam(n)
            lam = np.where(self._rng().rand(n) < self.mix_prob, lam_mix.astype(np.float32), lam)
        return lam, use_cutmix

    def _rand_bbox(self, H, W, lam):
        ratio = np.sqrt(1 - lam)
        cut_h, cut_w = int(H * ratio), int(W * ratio)
        r = self._rng()
        cy = r.randint(0, H)
        cx = r.randint(0, W)
        return (int(np.clip(cy - cut_h // 2, 0, H)), int(np.clip(cy + cut_h // 2, 0, H)),
                int(np.clip(cx - cut_w // 2, 0, W)), int(np.clip(cx + cut_w // 2, 0, W)))

    def _rand_bbox_minmax(self, H, W):
        lo, hi = self.cutmix_minmax
        r = self._rng()
        cut_h = r.randint(int(H * lo), int(H * hi))
        cut_w = r.randint(int(W * lo), int(W * hi))
        yl = r.randint(0, H - cut_h)
        xl = r.randint(0, W - cut_w)
        return int(yl), int(yl + cut_h), int(xl), int(xl + cut_w)

    def _cutmix_bbox_and_lam(self, H, W, lam):
        """The box (yl, yh, xl, xh) over (H, W) and the lam that goes with it."""
        if self.cutmix_minmax is not None:
            box = self._rand_bbox_minmax(H, W)
        else:
            box = self._rand_bbox(H, W, lam)
        if self.correct_lam or self.cutmix_minmax is not None:
            area = (box[1] - box[0]) * (box[3] - box[2])
            lam = 1.0 - area / float(H * W)
        return box, lam

    def decide(self, B: int, H: int, W: int) -> dict:
        """Draw the decisions for a batch of ``B`` samples with ``[H, W]`` planes; the tables ``ops.mix_batch`` takes and the lam of the
        targets.  ``__call__`` uses exactly this; it needs no GPU."""
        if B < 2 or B % 2:
            raise ValueError(f"Mixup: the batch size must be even, got {B}")
        kind = np.zeros(B, dtype=np.int32)
        lam32 = np.ones(B, dtype=np.float32)
        oml32 = np.zeros(B, dtype=np.float32)
        box = np.zeros((B, 4), dtype=np.int32)
        if self.mode == "batch":
            lam_mix, use_cutmix = self._params_per_batch()
            lam = lam_mix
            if lam_mix != 1.0:
                if use_cutmix:
                    bx, lam = self._cutmix_bbox_and_lam(H, W, lam_mix)
                    kind[:], box[:] = KIND_CUTMIX, bx
                else:
                    # torch multiplies a float32 tensor by float32(python float); 1 - lam is a Python (double) subtraction first
                    kind[:], lam32[:], oml32[:] = KIND_MIXUP, np.float32(lam_mix), np.float32(1.0 - lam_mix)
            target_lam = lam
        else:
            n = B if self.mode == "elem" else B // 2
            lam_mix, use_cutmix = self._params_per_elem(n)
            lam = lam_mix.copy()                                   # float32 [n], as timm keeps it
            for i in range(n):
                if lam_mix[i] == 1.0:
                    continue
                if use_cutmix[i]:
                    bx, l = self._cutmix_bbox_and_lam(H, W, lam_mix[i])
                    kind[i], box[i], lam[i] = KIND_CUTMIX, bx, l
                else:
                    # lam is a numpy float32 here, so is 1 - lam: a float32 subtraction
                    kind[i], lam32[i], oml32[i] = KIND_MIXUP, lam_mix[i], 1 - lam_mix[i]
            if self.mode == "pair":                                # both members of a pair share the decision
                for t in (kind, lam32, oml32, box):
                    t[B // 2:] = t[:B // 2][::-1]
                lam = np.concatenate((lam, lam[::-1]))
                lam_mix, use_cutmix = np.concatenate((lam_mix, lam_mix[::-1])), np.concatenate((use_cutmix, use_cutmix[::-1]))
            target_lam = lam
        return {"mode": self.mode, "kind": kind, "lam32": lam32, "oml32": oml32, "box": box, "use_cutmix": use_cutmix, "lam_mix": lam_mix,
                "lam": target_lam}

    # ---- the call ----------------------------------------------------------------------------------------
    @no_autocast
    def __call__(self, x: torch.Tensor, target: torch.Tensor):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda or x.dim() not in (4, 5):
            raise ValueError("Mixup: x must be a float32 GPU tensor [B, C, H, W] or [B, C, T, H, W], got "
                             + (f"{x.dtype} {tuple(x.shape)} on {x.device}" if isinstance(x, torch.Tensor) else type(x).__name__))
        B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
        if B < 2 or B % 2:
            raise ValueError(f"Mixup: the batch size must be even, got {B}")
        if x.numel() == 0:
            raise ValueError(f"Mixup: empty input {tuple(x.shape)}")
        if not x.is_contiguous():
            x = x.contiguous()
        p = self.decide(B, H, W)
        self.last_params = p
        ops.mix_batch(x, p["kind"], p["lam32"], p["oml32"], p["box"], H, W)
        lam = p["lam"]
        if not isinstance(lam, float):
            lam = torch.from_numpy(np.ascontiguousarray(lam, dtype=np.float32)).to(x.device, non_blocking=True).unsqueeze(1)
        return x, mixup_target(target, self.num_classes, lam, self.label_smoothing)
