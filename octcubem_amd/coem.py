"""COEM (contrastive OCT / en-face pre-training) step pieces -- SURVEY section 8f N4, counterparts of
``retinal-COEM/src/open_clip``: ``loss.gather_features`` / ``ClipLoss`` (loss.py:21-65, :148-230), ``model.CustomTextCLIP``
(model.py:635-682: two towers, ``logit_scale = log(1 / 0.07)``, L2-normalised features) and the per-step clamp of
``logit_scale`` to [0, log 100] (training/train_retclip.py).

The towers are the 3-D ST ViT (``models_vit_st``, OCT volume) and the 2-D ViT (``models_vit``, IR image) of this package; their
``head`` is the projection to the shared embedding.  The loss acts on ``[B, embed]`` features: a ``[B_global, B_global]``
logits matmul and two cross-entropies -- a few MFLOP next to the towers' TFLOPs, left to ATen on the device by default
(``fused=True``: ops.clip_pair_loss, csrc/cliploss.hip, which stores no ``[n, m]`` array).  The epoch loop with the reference's
cached-feature accumulation is ``train_one_epoch`` / ``train_one_epoch_3modalities`` below.  With
``world_size > 1`` the features of all ranks are exchanged by ONE all-gather per tower (RCCL over xGMI; gloo in the CPU tests),
differentiable when ``gather_with_grad`` (its backward is a reduce-scatter of the feature gradients)."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F
from ._autocast import autocast_invariant


def _native_comm(x: torch.Tensor):
    """The process's RCCL communicator behind the C ABI (comm.NativeComm), for GPU tensors when one has been created
    (misc.init_distributed_mode / bench.py do); None -> torch.distributed (gloo in the CPU tests)."""
    if not x.is_cuda:
        return None
    from . import comm as _comm
    c = _comm.get_default()
    return c if c is not None and c.world > 1 else None


def _all_gather_cat(x: torch.Tensor, group=None) -> torch.Tensor:
    """cat over ranks of x (no gradient), one collective."""
    x = x.contiguous()
    nc = _native_comm(x)
    if nc is not None:
        out = torch.empty((nc.world * x.shape[0],) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
        nc.all_gather_async(x, out)
        nc.wait()
        return out
    world = dist.get_world_size(group)
    out = torch.empty((world * x.shape[0],) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    dist.all_gather_into_tensor(out, x, group=group)
    return out


class _AllGatherWithGrad(torch.autograd.Function):
    """cat(all_gather(x)) whose backward returns this rank's slice of the SUM over ranks of the incoming gradient
    (what ``torch.distributed.nn.all_gather`` computes, as one reduce-scatter instead of world_size all-reduces)."""

    @staticmethod
    def forward(ctx, x, group):
        ctx.group = group
        return _all_gather_cat(x, group)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        nc = _native_comm(g)
        world = nc.world if nc is not None else dist.get_world_size(ctx.group)
        out = torch.empty((g.shape[0] // world,) + tuple(g.shape[1:]), dtype=g.dtype, device=g.device)
        if nc is not None:
            from . import comm as _comm
            nc.reduce_scatter_async(g, out, _comm.SUM)
            nc.wait()
        elif g.is_cuda:
            dist.reduce_scatter_tensor(out, g, op=dist.ReduceOp.SUM, group=ctx.group)
        else:                                   # gloo has no reduce_scatter: all-reduce and slice
            dist.all_reduce(g, op=dist.ReduceOp.SUM, group=ctx.group)
            r = dist.get_rank(ctx.group)
            out = g[r * out.shape[0]:(r + 1) * out.shape[0]].clone()
        return out, None


def gather_features(image_features, enface_features, local_loss=False, gather_with_grad=False, rank=0, world_size=1,
                    use_horovod=False, group=None):
    if use_horovod:
        raise NotImplementedError("horovod is not supported (one process per GPU under torch.distributed)")
    if gather_with_grad:
        return _AllGatherWithGrad.apply(image_features, group), _AllGatherWithGrad.apply(enface_features, group)
    gi = list(_all_gather_cat(image_features.detach(), group).chunk(world_size, dim=0))
    ge = list(_all_gather_cat(enface_features.detach(), group).chunk(world_size, dim=0))
    if not local_loss:          # keep the graph for the local rank's rows
        gi[rank] = image_features
        ge[rank] = enface_features
    return torch.cat(gi, dim=0), torch.cat(ge, dim=0)


def _rows(x):
    """a feature matrix as ops.clip_pair_loss takes it: unit column stride (a row-strided slice is passed as it is)"""
    return x if x.dim() != 2 or x.shape[1] == 1 or x.stride(1) == 1 else x.contiguous()


@autocast_invariant
class ClipLoss(nn.Module):
    """``fused=True``: the same gather and the same partners, with the logits / cross-entropy part and its autograd replaced by
    ops.clip_pair_loss (csrc/cliploss.hip: no [n, m] array, deterministic) -- one call for the single-process and the gathered
    non-local case, two rectangular calls under ``local_loss``.  ``correct_label`` (soft labels from duplicate reports) keeps the ATen
    path whatever ``fused`` says.  ``fused=False`` (default) is the ATen composition, unchanged."""

    def __init__(self, local_loss=False, gather_with_grad=False, cache_labels=False, rank=0, world_size=1, use_horovod=False,
                 correct_label=0, fused=False):
        super().__init__()
        self.local_loss = local_loss
        self.gather_with_grad = gather_with_grad
        self.cache_labels = cache_labels
        self.rank = rank
        self.world_size = world_size
        self.use_horovod = use_horovod
        self.correct_label = correct_label
        self.fused = fused
        self.prev_num_logits = 0
        self.labels = {}
        self._fused_w = {}

    def _forward_fused(self, image_features, enface_features, logit_scale):
        from . import ops
        if self.world_size > 1:
            all_image, all_enface = gather_features(image_features, enface_features, self.local_loss, self.gather_with_grad,
                                                    self.rank, self.world_size, self.use_horovod)
            if self.local_loss:
                n = image_features.shape[0]
                w = self._uniform(n, image_features.device)
                off = n * self.rank              # labels = arange(num_logits) + num_logits * rank
                return (ops.clip_pair_loss(_rows(image_features), _rows(all_enface), logit_scale, w, None, off)
                        + ops.clip_pair_loss(_rows(enface_features), _rows(all_image), logit_scale, w, None, off))
            image_features, enface_features = all_image, all_enface
        w = self._uniform(image_features.shape[0], image_features.device)
        return ops.clip_pair_loss(_rows(image_features), _rows(enface_features), logit_scale, w, w, 0)

    def _uniform(self, n, device):
        """1 / (2 n) per row: the mean of each cross entropy and the halving of their sum"""
        w = self._fused_w.get((n, device)) if self.cache_labels else None
        if w is None:
            w = torch.full((n,), 0.5 / n, dtype=torch.float32, device=device)
            if self.cache_labels:
                self._fused_w = {(n, device): w}
        return w

    def get_corrected_label(self, enface_features_i, enface_features_j, t=10 ** (-100)):
        """Soft labels that share the target mass among samples with IDENTICAL en-face features (same report)."""
        d = torch.cdist(enface_features_i.detach().float(), enface_features_j.detach().float())
        L = (d <= t).to(enface_features_i.dtype)
        return L / torch.sum(L, dim=1, keepdim=True)

    def forward(self, image_features, enface_features, logit_scale):
        if self.fused and not self.correct_label:
            return self._forward_fused(image_features, enface_features, logit_scale)
        device = image_features.device
        if self.world_size > 1:
            all_image, all_enface = gather_features(image_features, enface_features, self.local_loss, self.gather_with_grad,
                                                    self.rank, self.world_size, self.use_horovod)
            if self.local_loss:
                logits_per_image = logit_scale * image_features @ all_enface.T
                logits_per_enface = logit_scale * enface_features @ all_image.T
            else:
                logits_per_image = logit_scale * all_image @ all_enface.T
                logits_per_enface = logits_per_image.T
        else:
            all_enface = enface_features
            logits_per_image = logit_scale * image_features @ enface_features.T
            logits_per_enface = logit_scale * enface_features @ image_features.T
        if self.correct_label:
            src = enface_features if (self.world_size > 1 and self.local_loss) or self.world_size == 1 else all_enface
            labels = self.get_corrected_label(src, all_enface)
        else:
            num_logits = logits_per_image.shape[0]
            if self.prev_num_logits != num_logits or device not in self.labels:
                labels = torch.arange(num_logits, device=device, dtype=torch.long)
                if self.world_size > 1 and self.local_loss:
                    labels = labels + num_logits * self.rank
                if self.cache_labels:
                    self.labels[device] = labels
                    self.prev_num_logits = num_logits
            else:
                labels = self.labels[device]
        return (F.cross_entropy(logits_per_image, labels) + F.cross_entropy(logits_per_enface, labels)) / 2


def gather_features_3mod(image_features, enface1_features, enface2_features, t_weight1, t_weight2, local_loss=False,
                         gather_with_grad=False, rank=0, world_size=1, use_horovod=False, group=None):
    """open_clip/loss.py:68-146: the five per-sample tensors of the 3-modality loss (OCT, two en-face modalities, and the
    two presence weights) gathered over ranks -- with gradient, or detached with the local rank's rows spliced back in."""
    if use_horovod:
        raise NotImplementedError("horovod is not supported (one process per GPU under torch.distributed)")
    xs = (image_features, enface1_features, enface2_features, t_weight1, t_weight2)
    if gather_with_grad:
        return tuple(_AllGatherWithGrad.apply(x, group) for x in xs)
    out = []
    for x in xs:
        parts = list(_all_gather_cat(x.detach(), group).chunk(world_size, dim=0))
        if not local_loss:
            parts[rank] = x
        out.append(torch.cat(parts, dim=0))
    return tuple(out)


@autocast_invariant
class ThreeModalityClipLoss(nn.Module):
    """open_clip/loss.py:230-385: symmetric InfoNCE over the three pairs (OCT, en-face 1), (OCT, en-face 2), (en-face 1,
    en-face 2) with one temperature per pair; a sample whose modality is missing carries weight 0 in that modality's terms
    (t_weight1 / t_weight2, per sample), each term is a weighted mean over the samples present, 0 when none is; the total is
    the mean of the six directed terms.

    ``fused=True``: three ops.clip_pair_loss calls (six rectangular ones under ``local_loss``) with the weights w / (6 sum w) built on the
    device -- a modality absent from the whole batch contributes 0 without the host read of the ATen path.  The ``local_loss`` partners
    are taken as the ATen path forms them (the reference's GLOBAL-count offset); where that puts a partner out of range the fused path
    raises ValueError (``cross_entropy`` raises its own error there).  ``correct_label`` keeps the ATen path whatever ``fused`` says."""

    def __init__(self, local_loss=False, gather_with_grad=False, cache_labels=False, rank=0, world_size=1, use_horovod=False,
                 correct_label=0, fused=False):
        super().__init__()
        self.local_loss = local_loss
        self.gather_with_grad = gather_with_grad
        self.cache_labels = cache_labels
        self.rank = rank
        self.world_size = world_size
        self.use_horovod = use_horovod
        self.correct_label = correct_label
        self.fused = fused
        self.prev_num_logits = 0
        self.labels = {}

    def _forward_fused(self, image_features, enface1_features, enface2_features, logit_scale, logit_scale1, logit_scale2, t_weight1,
                       t_weight2):
        from . import ops
        if self.world_size > 1:
            all_i, all_e1, all_e2, all_w1, all_w2 = gather_features_3mod(
                image_features, enface1_features, enface2_features, t_weight1, t_weight2, self.local_loss, self.gather_with_grad,
                self.rank, self.world_size, self.use_horovod)
        else:
            all_i, all_e1, all_e2, all_w1, all_w2 = image_features, enface1_features, enface2_features, t_weight1, t_weight2

        def share(w):                  # w / (6 sum w), 0 where the modality is absent from the whole batch: no host read
            w = w.detach().to(torch.float32)
            tot = w.sum()
            return torch.where(tot > 0, w / (6.0 * tot), torch.zeros_like(w))
        f = _rows
        if self.local_loss:
            off = all_i.shape[0] * self.rank if self.world_size > 1 else 0      # the GLOBAL count, as the ATen path (and the reference)
            w1, w2 = share(t_weight1), share(t_weight2)
            w12 = share(t_weight1 * t_weight2)
            pairs = ((image_features, all_e1, logit_scale, w1), (enface1_features, all_i, logit_scale, w1),
                     (image_features, all_e2, logit_scale1, w2), (enface2_features, all_i, logit_scale1, w2),
                     (enface1_features, all_e2, logit_scale2, w12), (enface2_features, all_e1, logit_scale2, w12))
            return sum(ops.clip_pair_loss(f(a), f(b), sc, w, None, off) for a, b, sc, w in pairs)
        w1, w2, w12 = share(all_w1), share(all_w2), share(all_w1 * all_w2)
        return (ops.clip_pair_loss(f(all_i), f(all_e1), logit_scale, w1, w1, 0) + ops.clip_pair_loss(f(all_i), f(all_e2), logit_scale1, w2, w2, 0)
                + ops.clip_pair_loss(f(all_e1), f(all_e2), logit_scale2, w12, w12, 0))

    @staticmethod
    def get_corrected_label(features_i, features_j, t=1e-10):
        d = torch.sqrt(((features_i.detach().unsqueeze(1) - features_j.detach().unsqueeze(0)) ** 2).sum(dim=-1))
        L = (d <= t).to(torch.float32)
        return L / torch.sum(L, dim=1, keepdim=True)

    @staticmethod
    def _weighted(loss_vec, w):
        tot = w.sum()
        return loss_vec.new_zeros(()) if float(tot) == 0.0 else (loss_vec * w).sum() / tot

    def forward(self, image_features, enface1_features, enface2_features, logit_scale, logit_scale1, logit_scale2, t_weight1,
                t_weight2):
        if self.fused and not self.correct_label:
            return self._forward_fused(image_features, enface1_features, enface2_features, logit_scale, logit_scale1, logit_scale2,
                                       t_weight1, t_weight2)
        device = image_features.device
        if self.world_size > 1:
            all_i, all_e1, all_e2, all_w1, all_w2 = gather_features_3mod(
                image_features, enface1_features, enface2_features, t_weight1, t_weight2, self.local_loss, self.gather_with_grad,
                self.rank, self.world_size, self.use_horovod)
        else:
            all_i, all_e1, all_e2, all_w1, all_w2 = image_features, enface1_features, enface2_features, t_weight1, t_weight2
        if self.local_loss:
            l_i_e1 = logit_scale * image_features @ all_e1.T; l_e1_i = logit_scale * enface1_features @ all_i.T
            l_i_e2 = logit_scale1 * image_features @ all_e2.T; l_e2_i = logit_scale1 * enface2_features @ all_i.T
            l_e1_e2 = logit_scale2 * enface1_features @ all_e2.T; l_e2_e1 = logit_scale2 * enface2_features @ all_e1.T
            w1, w2 = t_weight1, t_weight2
        else:
            l_i_e1 = logit_scale * all_i @ all_e1.T; l_e1_i = l_i_e1.T
            l_i_e2 = logit_scale1 * all_i @ all_e2.T; l_e2_i = l_i_e2.T
            l_e1_e2 = logit_scale2 * all_e1 @ all_e2.T; l_e2_e1 = l_e1_e2.T
            w1, w2 = all_w1, all_w2
        if self.correct_label:
            labels = self.get_corrected_label(enface1_features, all_e1).to(device)
        else:
            num_logits = all_i.shape[0]           # as the reference: the GLOBAL count, also under local_loss
            if self.prev_num_logits != num_logits or device not in self.labels:
                labels = torch.arange(num_logits, device=device, dtype=torch.long)
                if self.world_size > 1 and self.local_loss:
                    labels = labels + num_logits * self.rank
                if self.cache_labels:
                    self.labels[device] = labels
                    self.prev_num_logits = num_logits
            else:
                labels = self.labels[device]
        ce = lambda lg: F.cross_entropy(lg, labels, reduction="none")
        w12 = w1 * w2
        terms = (self._weighted(ce(l_i_e1), w1), self._weighted(ce(l_e1_i), w1), self._weighted(ce(l_i_e2), w2),
                 self._weighted(ce(l_e2_i), w2), self._weighted(ce(l_e1_e2), w12), self._weighted(ce(l_e2_e1), w12))
        return sum(terms) / 6


@autocast_invariant
class CustomTextCLIP(nn.Module):
    """Two towers + a learned temperature.  ``visual`` / ``text`` are modules mapping their input to ``[B, embed_dim]`` (here:
    models_vit_st / models_vit with ``num_classes = embed_dim``); the reference builds them from config objects
    (model.py:125-578), this class takes them ready-made."""

    def __init__(self, visual: nn.Module, text: nn.Module):
        super().__init__()
        self.visual = visual
        self.text = text
        self.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))

    def lock_image_tower(self, unlocked_groups=0, freeze_bn_stats=False):
        """model.py:649-651 (``--lock-image --lock-image-unlocked-groups N``): lock the OCT tower as per LiT."""
        self.visual.lock(unlocked_groups=unlocked_groups, freeze_bn_stats=freeze_bn_stats)

    def lock_text_tower(self, unlocked_layers: int = 0, freeze_layer_norm: bool = True):
        """model.py:653-654: the en-face tower's ``lock``, the two arguments passed by position as the reference passes them (a ViT
        tower reads them as ``unlocked_groups, freeze_bn_stats``)."""
        self.text.lock(unlocked_layers, freeze_layer_norm)

    @torch.jit.ignore
    def set_grad_checkpointing(self, enable=True, mode="full"):
        """model.py:656-659 (``--grad-checkpointing``) on both towers; ``mode`` as in video_vit.set_recompute."""
        self.visual.set_grad_checkpointing(enable, mode)
        self.text.set_grad_checkpointing(enable, mode)

    def encode_image(self, image, normalize: bool = False):
        features = self.visual(image).float()
        return F.normalize(features, dim=-1) if normalize else features

    def encode_text(self, text, normalize: bool = False):
        features = self.text(text).float()
        return F.normalize(features, dim=-1) if normalize else features

    def forward(self, image, text, single_modality=None):
        if single_modality is not None:
            assert single_modality in ["image", "text"], f"single_modality should be either 'image' or 'text', got {single_modality}"
            if single_modality == "image":
                return self.encode_image(image, normalize=True), None, self.logit_scale.exp()
            return None, self.encode_text(text, normalize=True), self.logit_scale.exp()
        return self.encode_image(image, normalize=True), self.encode_text(text, normalize=True), self.logit_scale.exp()


@autocast_invariant
class CustomTextCLIP3Mod(CustomTextCLIP):
    """open_clip/model.py:685-720: one OCT tower, ONE en-face tower with a head per modality (models_vit_2mod: IR = modality 0, FAF =
    modality 1) and a temperature per pair -- ``logit_scale`` (OCT, IR), ``logit_scale1`` (OCT, FAF), ``logit_scale2`` (IR, FAF).
    ``forward`` returns the reference's 6-tuple (L2-normalised features, None for a modality ``single_modality`` leaves out, and the
    three exponentiated temperatures).  With both en-face images present the tower runs them in one trunk pass (``forward_pair``;
    ``pair=False``: two passes, as the reference).  Deliberate departure: the 'text2' branch returns ``logit_scale2.exp()`` -- the
    reference returns the unbound method there (model.py:715, a missing call)."""

    def __init__(self, visual: nn.Module, text: nn.Module, pair: bool = True):
        super().__init__(visual, text)
        self.logit_scale1 = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))
        self.logit_scale2 = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))
        self.pair = bool(pair)

    def encode_text(self, text, normalize: bool = False, modality=0):
        features = self.text(text, modality=modality).float()
        return F.normalize(features, dim=-1) if normalize else features

    def _scales(self):
        return self.logit_scale.exp(), self.logit_scale1.exp(), self.logit_scale2.exp()

    def _raw_features(self, image, text1, text2, single_modality=None):
        """the RAW tower outputs (image, text1, text2), None for what ``single_modality`` leaves out"""
        if single_modality not in ("image", "text1", "text2", None):
            raise ValueError(f"single_modality should be either 'image', 'text1', 'text2' or None, got {single_modality}")
        if single_modality == "image":
            return self.encode_image(image), None, None
        if single_modality == "text1":
            return None, self.encode_text(text1, modality=0), None
        if single_modality == "text2":
            return None, None, self.encode_text(text2, modality=1)
        fi = self.encode_image(image)
        if self.pair and hasattr(self.text, "forward_pair"):
            f1, f2 = self.text.forward_pair(text1, text2)
            return fi, f1.float(), f2.float()
        return fi, self.encode_text(text1, modality=0), self.encode_text(text2, modality=1)

    def forward(self, image, text1, text2, single_modality=None):
        feats = self._raw_features(image, text1, text2, single_modality)
        return tuple(None if f is None else F.normalize(f, dim=-1) for f in feats) + self._scales()


@autocast_invariant
class ClassificationHead(nn.Module):
    """open_clip/model.py:723-739: ``input_norm`` (LayerNorm, eps 1e-5) -> ``fc1`` -> GELU -> ``fc2`` with the reference's keys and
    initialisation (``fc1.weight`` ~ N(0, 0.02), everything else nn.Linear's / nn.LayerNorm's own).  A module with a parameter arena of
    its own, as each tower is (``prepare()`` / ``invalidate_lp()``; one FusedAdamW / FlatGradReducer per arena).

    ``forward(x)`` on an already-joined fp32 ``x`` is the plain form: the LayerNorm kernel, then fc1 + GELU -> fc2 on the MLP path
    (ops.MlpFn).  ``forward_joined(features, present_mask)`` takes the RAW tower outputs and runs ops.JoinFn (csrc/join.hip: normalise,
    zero-fill, concatenate, LayerNorm in one kernel each way) in front of the same MLP; it returns ``(logits, normalised features)``.
    ``num_classes % 8 != 0`` (the reference's 2 and 5): fc2 takes the ``torch.nn.functional.linear`` route models_vit takes for odd class
    counts, behind fc1 as ops.LinearFn and ATen's GELU."""

    def __init__(self, input_dim, hidden_dim, num_classes, initialization=True):
        super().__init__()
        self.fc1 = nn.Linear(input_dim, hidden_dim)
        self.gelu = nn.GELU()
        self.fc2 = nn.Linear(hidden_dim, num_classes)
        self.input_norm = nn.LayerNorm(input_dim)
        if initialization:
            torch.nn.init.normal_(self.fc1.weight, std=0.02)

    def prepare(self):
        from .arena import get_arena
        arena = get_arena(self, full_check=True)
        if torch.is_grad_enabled():
            arena.rebind_grads()
        arena.refresh_lp()
        return arena

    @property
    def arena(self):
        from .arena import get_arena
        return get_arena(self, full_check=True)

    def invalidate_lp(self):
        self.arena.invalidate_lp()

    def _mlp(self, arena, y):
        from . import ops
        f1, f2 = self.fc1, self.fc2
        if f2.out_features % 8 == 0:
            ps = (f1.weight, f1.bias, f2.weight, f2.bias)
            return ops.MlpFn.apply(y, None, arena.lp_view(f1.weight), arena.f32_view(f1.bias), arena.lp_view(f2.weight),
                                   arena.f32_view(f2.bias), lambda: tuple(arena.grad_view(p) for p in ps), *ps).float()
        h = ops.LinearFn.apply(y, arena.lp_view(f1.weight), arena.f32_view(f1.bias), lambda: arena.grad_view(f1.weight),
                               lambda: arena.grad_view(f1.bias), True, f1.weight, f1.bias)
        return F.linear(F.gelu(h), f2.weight, f2.bias)

    def forward(self, x):
        from .video_vit import layer_norm
        arena = self.prepare()
        return self._mlp(arena, layer_norm(self.input_norm, x.float().contiguous()))

    def forward_joined(self, features, present_mask):
        from . import ops
        arena = self.prepare()
        feats = tuple(None if f is None else f.float() for f in features)
        y, *n = ops.JoinFn.apply(self.input_norm.weight, self.input_norm.bias, self.input_norm.eps, int(present_mask), *feats)
        return self._mlp(arena, y), tuple(n)


def _tower_out_dim(tower):
    d = getattr(tower, "out_dim", None)
    return int(d) if d else int(tower.head.out_features)


@autocast_invariant
class CustomTextCLIPClassification(CustomTextCLIP):
    """open_clip/model.py:741-769: the two towers and a ClassificationHead over ``2 * embed_dim``; ``forward`` returns
    ``(logits, logit_scale.exp())``.  ``single_modality`` ('image' | 'text') puts zeros into the absent slot, as the reference does.
    The normalisation, the zero-filling, the concatenation and the head's LayerNorm are one kernel (ClassificationHead.forward_joined)."""

    def __init__(self, visual: nn.Module, text: nn.Module, num_classes: int, embed_dim: int = None):
        super().__init__(visual, text)
        embed_dim = _tower_out_dim(visual) if embed_dim is None else int(embed_dim)
        self.classification_head = ClassificationHead(2 * embed_dim, hidden_dim=embed_dim, num_classes=num_classes)

    def forward(self, image, text, single_modality=None):
        if single_modality not in ("image", "text", None):
            raise ValueError(f"single_modality should be either 'image' or 'text', got {single_modality}")
        fi = None if single_modality == "text" else self.encode_image(image)
        ft = None if single_modality == "image" else self.encode_text(text)
        mask = (1 if fi is not None else 0) | (2 if ft is not None else 0)
        logits, _ = self.classification_head.forward_joined((fi, ft), mask)
        return logits, self.logit_scale.exp()


@autocast_invariant
class CustomTextCLIP3ModClassification(CustomTextCLIP3Mod):
    """open_clip/model.py:772-809: CustomTextCLIP3Mod and a ClassificationHead over ``3 * embed_dim``; ``forward`` returns ``(logits,
    logit_scale.exp(), logit_scale1.exp(), logit_scale2.exp())``; ``single_modality`` ('image' | 'text1' | 'text2') puts zeros into
    the two absent slots."""

    def __init__(self, visual: nn.Module, text: nn.Module, num_classes: int, embed_dim: int = None, pair: bool = True):
        super().__init__(visual, text, pair=pair)
        embed_dim = _tower_out_dim(visual) if embed_dim is None else int(embed_dim)
        self.classification_head = ClassificationHead(3 * embed_dim, hidden_dim=embed_dim, num_classes=num_classes)

    def forward_with_features(self, image, text1, text2, single_modality=None):
        """-> (logits, (n_image, n_text1, n_text2)): the normalised features the join kernel wrote, zeros in absent slots"""
        feats = self._raw_features(image, text1, text2, single_modality)
        mask = sum(1 << k for k, f in enumerate(feats) if f is not None)
        return self.classification_head.forward_joined(feats, mask)

    def forward(self, image, text1, text2, single_modality=None):
        logits, _ = self.forward_with_features(image, text1, text2, single_modality)
        return (logits,) + self._scales()


def build_towers_from_config(cfg: dict, flash_semantics: bool = True):
    """Config-driven construction of the two towers, for the model configs the reference ships for this path
    (retinal-COEM/src/open_clip/model_configs/vit_large_patch16_retFound-vit_large_patch16_OCTCube.json through
    open_clip/model.py ``_build_vision_tower`` :190-290 and ``_build_text_tower`` :462-509):

      vision_cfg.model_name  "ViT_ST" | "ViT_ST_nodrop"   -> the 3-D spatio-temporal ViT (models_vit_st), ``out_dim = embed_dim`` head,
                             sep_pos_embed / cls_embed on, dropout before the head only for "ViT_ST"
      text_cfg.vit_model_name "ViT_flash_attn"             -> the 2-D ViT (models_vit) on the en-face image
                              "ViT_flash_attn_2mod"        -> the two-modality en-face tower (models_vit_2mod: one trunk, a head per
                                                              modality), ``flash_compat`` from its own ``use_flash_attn`` and ``flash_semantics``

    ``use_flash_attn: true`` in the config selects, in the reference, flash-attn blocks whose final residual is dropped
    (SURVEY section 0 fact 3); ``flash_semantics`` reproduces that through ``flash_compat`` (native key layout).  The rest of
    open_clip's tower zoo (timm / HIPT / LongNet / Perceiver / HF text) is out of scope.  Checkpoints named by ``model_ckpt``
    are loaded with checkpoint.load_pretrained when the file exists (the reference raises when it does not; here the tower
    stays randomly initialised and says so)."""
    import os
    from functools import partial
    from . import checkpoint as _ck, models_vit, models_vit_st
    embed_dim = int(cfg["embed_dim"])
    v, t = dict(cfg["vision_cfg"]), dict(cfg["text_cfg"])
    name = v.get("model_name") or ""
    if name not in ("ViT_ST", "ViT_ST_nodrop"):
        raise NotImplementedError(f"vision tower {name!r}: only the ViT_ST / ViT_ST_nodrop towers of the OCTCube configs are built")
    nf = int(v.get("num_frames", -1))
    visual = models_vit_st.VisionTransformer(
        num_frames=nf if nf > 0 else 60, t_patch_size=int(v.get("t_patch_size", 3)), img_size=int(v["image_size"]),
        patch_size=int(v["patch_size"]), in_chans=int(v.get("in_chans", 1)), num_classes=embed_dim, embed_dim=int(v["width"]),
        depth=int(v["layers"]), num_heads=int(v["num_heads"]), mlp_ratio=float(v.get("mlp_ratio", 4)),
        norm_layer=partial(nn.LayerNorm, eps=float(v.get("norm_layer_eps", 1e-6))), drop_path_rate=float(v.get("drop_path_rate", 0.0)),
        dropout=float(v.get("dropout", 0.0)) if name == "ViT_ST" else 0.0, sep_pos_embed=True, cls_embed=True,
        global_pool=bool(v.get("global_pool", True)) if name == "ViT_ST_nodrop" else True,
        flash_compat=bool(v.get("use_flash_attn", False)) and flash_semantics)
    tname = t.get("vit_model_name") or ""
    if "ViT_flash_attn_2mod" in tname:          # open_clip/model.py:510-534: one trunk, a head per en-face modality
        from . import models_vit_2mod
        text = models_vit_2mod.VisionTransformer(
            image_size=int(t["image_size"]), out_dim=embed_dim, embed_dim=int(t["width"]), depth=int(t["layers"]),
            patch_size=int(t["patch_size"]), in_chans=int(t.get("in_chans", 3)), global_pool=bool(t.get("global_pool", True)),
            num_heads=int(t["num_heads"]), mlp_ratio=float(t.get("mlp_ratio", 4)), drop_path_rate=float(t.get("drop_path_rate", 0.0)),
            norm_layer=partial(nn.LayerNorm, eps=float(t.get("norm_layer_eps", 1e-6))), dropout=float(t.get("dropout", 0.5)),
            cls_embed=True, num_mod_head=2, flash_compat=bool(t.get("use_flash_attn", False)) and flash_semantics)
    elif "ViT_flash_attn" not in tname or "mod" in tname:
        raise NotImplementedError(f"en-face tower {tname!r}: only ViT_flash_attn and ViT_flash_attn_2mod are built")
    else:
        text = models_vit.VisionTransformer(
            img_size=int(t["image_size"]), patch_size=int(t["patch_size"]), in_chans=int(t.get("in_chans", 3)), num_classes=embed_dim,
            embed_dim=int(t["width"]), depth=int(t["layers"]), num_heads=int(t["num_heads"]), mlp_ratio=float(t.get("mlp_ratio", 4)),
            qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=float(t.get("norm_layer_eps", 1e-6))),
            drop_path_rate=float(t.get("drop_path_rate", 0.0)), global_pool=bool(t.get("global_pool", True)))
    for tower, c in ((visual, v), (text, t)):
        path = c.get("model_ckpt")
        if path and os.path.exists(path):
            ck = torch.load(path, map_location="cpu")
            _ck.load_pretrained(tower, ck, filter_keys=())
        elif path:
            print(f"Warnings! No such checkpoint {path}: randomizing the model!")
    return visual, text


def create_model_from_config(cfg: dict, three: bool = False, num_classes: int = None, **kw) -> "CustomTextCLIP":
    """The model open_clip/factory.py:299-309 picks for the configs above: ``three`` is its ``args.enable_3mod_training``, a
    ``num_classes`` its ``args.cls_dataset`` (with ``args.num_classes``) --
        neither: CustomTextCLIP          three: CustomTextCLIP3Mod
        num_classes: CustomTextCLIPClassification          both: CustomTextCLIP3ModClassification"""
    visual, text = build_towers_from_config(cfg, **kw)
    if num_classes is not None:
        cls = CustomTextCLIP3ModClassification if three else CustomTextCLIPClassification
        return cls(visual, text, int(num_classes), embed_dim=int(cfg["embed_dim"]))
    return CustomTextCLIP3Mod(visual, text) if three else CustomTextCLIP(visual, text)


def make_reducers(model, comm=None, **kw):
    """One FlatGradReducer per tower (each tower is a model with its own flat gradient arena), and one for the classification head of a
    model that has one."""
    from .parallel import FlatGradReducer
    m = getattr(model, "module", model)
    reds = [FlatGradReducer(m.visual, comm=comm, **kw), FlatGradReducer(m.text, comm=comm, **kw)]
    if getattr(m, "classification_head", None) is not None:
        reds.append(FlatGradReducer(m.classification_head, comm=comm, **kw))
    return reds


def clamp_logit_scale(model):
    """After every optimizer step (train_retclip.py): logit_scale stays within [0, ln 100]."""
    with torch.no_grad():
        getattr(model, "module", model).logit_scale.clamp_(0, math.log(100))


def train_step(model, loss_fn, images, texts, optimizers, loss_scalers=None, clip_grad=None, reducers=None):
    """One accum_freq == 1 iteration of train_retclip.train_one_epoch: forward both towers, ClipLoss, backward, optional clip,
    optimizer step(s), clamp.  ``optimizers``: one per parameter set (each tower owns its own flat arena / FusedAdamW; the
    temperature uses a plain torch optimizer).  Returns the loss (detached).

    Data parallel (the reference wraps the whole model in DistributedDataParallel, training/main_retclip.py:206): pass
    ``reducers`` = one parallel.FlatGradReducer per tower (``make_reducers``); they exchange the towers' weight gradients
    during backward, and the temperature's scalar gradient is averaged here -- without them every rank would step on its local
    gradient only and the replicas would drift apart."""
    for o in optimizers:
        o.zero_grad()
    image_features, text_features, logit_scale = model(images, texts)
    loss = loss_fn(image_features, text_features, logit_scale)
    if reducers:
        for r in reducers:
            r.begin_backward(sync=True)
    loss.backward()
    if reducers:
        for r in reducers:
            r.finish()
        g = getattr(model, "module", model).logit_scale.grad
        if g is not None and reducers[0].world > 1:
            nc = _native_comm(g)
            if nc is not None:
                from . import comm as _comm
                nc.all_reduce_async(g, _comm.AVG)
                nc.wait()
            else:
                dist.all_reduce(g)
                g.div_(reducers[0].world)
    if clip_grad is not None:
        torch.nn.utils.clip_grad_norm_([p for p in model.parameters() if p.grad is not None], clip_grad)
    for o in optimizers:
        o.step()
    clamp_logit_scale(model)
    return loss.detach()


# ---------------------------------------------------------------------------------------------------------------------------------
# the epoch loop (training/train_retclip.py:64-240, train_retclip_3modalities.py:74-276) and its schedule (training/scheduler.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def _optimizer_list(optimizers):
    return list(optimizers) if isinstance(optimizers, (list, tuple)) else [optimizers]


def assign_learning_rate(optimizer, new_lr):
    """scheduler.assign_learning_rate; ``optimizer`` may be a list (one optimizer per tower arena and one for the temperature)."""
    for o in _optimizer_list(optimizer):
        for param_group in o.param_groups:
            param_group["lr"] = new_lr


def _warmup_lr(base_lr, warmup_length, step):
    return base_lr * (step + 1) / warmup_length


def cosine_lr(optimizer, base_lr, warmup_length, steps):
    """scheduler.cosine_lr: linear warm-up over ``warmup_length`` steps, then half a cosine down to 0 at ``steps``."""
    def _lr_adjuster(step):
        if step < warmup_length:
            lr = _warmup_lr(base_lr, warmup_length, step)
        else:
            e = step - warmup_length
            es = steps - warmup_length
            lr = 0.5 * (1 + np.cos(np.pi * e / es)) * base_lr
        assign_learning_rate(optimizer, lr)
        return lr
    return _lr_adjuster


# The loop's default for ``fused``: the path profiles/cliploss_bench.txt shows faster at the shipped local-loss shape (32 local rows
# against 256 gathered columns, two calls, forward + backward, d = 512): the ATen composition at 387 us per call against 819 us for the
# fused path on an MI355X -- so False.  (The fused path is the faster one only at n = m = 64, and holds 33 x less memory at n = 8192.)
FUSED_DEFAULT = False


class AverageMeter:
    """train_retclip.AverageMeter"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = 0
        self.avg = 0
        self.sum = 0
        self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def stack_weight_modalities(weight_modalities):
    """train_retclip_3modalities.stack_weight_modalities: [accum step][modality] -> [modality], concatenated over the steps."""
    return [torch.cat([step[i] for step in weight_modalities], dim=0) for i in range(len(weight_modalities[0]))]


def convert_modalities_idx_to_flag(modalities):
    """The per-sample presence weights of one modality as a float32 tensor.  (The reference imports this helper from open_clip/misc.py,
    a module it does not ship; its loss uses the result as a 0 / 1 weight per sample, which is what the loader's flags are.)"""
    return torch.as_tensor(modalities).to(torch.float32)


def _refuse_unsupported(name, scaler, args):
    if scaler is not None:
        raise NotImplementedError(f"{name}: a GradScaler is not run by this package (the kernels keep fp32 gradients on bfloat16 operands; "
                                  "pass scaler=None)")
    if getattr(args, "horovod", False):
        raise NotImplementedError(f"{name}: horovod is not supported (one process per GPU under torch.distributed)")
    if getattr(args, "wandb", False):
        raise NotImplementedError(f"{name}: wandb logging is not part of this package (pass a tb_writer)")
    precision = getattr(args, "precision", None)
    if precision not in (None, "fp32", "amp", "amp_bf16", "amp_bfloat16"):
        raise NotImplementedError(f"{name}: precision {precision!r} casts the inputs to a 16-bit type, which this package does not run "
                                  "(the kernels choose their own operand precision; use 'amp', 'amp_bf16' or 'fp32')")


def _average_temperature_grads(model, reducers):
    """the scalar temperature gradients are averaged over ranks once per optimizer step (DistributedDataParallel's job in the reference)"""
    if not reducers or reducers[0].world <= 1:
        return
    m = getattr(model, "module", model)
    for name in ("logit_scale", "logit_scale1", "logit_scale2"):
        g = getattr(getattr(m, name, None), "grad", None)
        if g is None:
            continue
        nc = _native_comm(g)
        if nc is not None:
            from . import comm as _comm
            nc.all_reduce_async(g, _comm.AVG)
            nc.wait()
        else:
            dist.all_reduce(g)
            g.div_(reducers[0].world)


def _run_epoch(name, three, model, data, epoch, optimizers, scaler, scheduler, args, tb_writer, reducers, loss, fused):
    import logging
    import time
    _refuse_unsupported(name, scaler, args)
    mm = getattr(args, "multimodal_type", "default") or "default"
    allowed = ("oct_faf_ir",) if three else ("default", "oct_ir", "oct_faf_only")
    if mm not in allowed:
        raise NotImplementedError(f"{name}: multimodal_type {mm!r} is not supported (only {', '.join(repr(a) for a in allowed)})")
    optimizers = _optimizer_list(optimizers)
    device = torch.device(args.device)
    accum_freq = int(getattr(args, "accum_freq", 1))
    rank, world_size = getattr(args, "rank", 0), getattr(args, "world_size", 1)
    is_master = rank == 0
    clip = getattr(args, "grad_clip_norm", None)
    model.train()
    if loss is None:
        cls = ThreeModalityClipLoss if three else ClipLoss
        loss = cls(local_loss=getattr(args, "local_loss", False), gather_with_grad=getattr(args, "gather_with_grad", False),
                   cache_labels=True, rank=rank, world_size=world_size, use_horovod=False,
                   correct_label=getattr(args, "correct_label", 0), fused=FUSED_DEFAULT if fused is None else bool(fused))

    data["train"].set_epoch(epoch)
    dataloader = data["train"].dataloader
    num_batches_per_epoch = dataloader.num_batches // accum_freq
    sample_digits = math.ceil(math.log(dataloader.num_samples + 1, 10))
    total_train_batch_size = accum_freq * args.batch_size * world_size
    log_every = getattr(args, "log_every_n_steps", 100)
    unwrapped = getattr(model, "module", model)
    accum_inputs, accum_features, accum_weights = [], [], []
    record = {"losses": [], "micro_losses": [], "steps": 0}

    def unpack(batch):
        """-> (model inputs on the device, per-sample weights [oct, ir, faf] or None)"""
        if mm == "default":
            images, texts = batch
            inputs, weights = (images, texts), None
        else:
            images, texts_ir, texts_f2_faf = batch[0]["oct"], batch[0]["ir"], batch[0]["f2_faf"]
            modalities = batch[1][2]
            if mm == "oct_ir":
                inputs, weights = (images, texts_ir), None
            elif mm == "oct_faf_only":
                assert sum(modalities[2]) == len(modalities[2]), "Only f2_faf is allowed in this setting"
                inputs, weights = (images, texts_f2_faf), None
            else:
                inputs = (images, texts_ir, texts_f2_faf)
                weights = [convert_modalities_idx_to_flag(mod) for mod in modalities[:3]]
        return tuple(x.to(device=device, non_blocking=True) for x in inputs), weights

    def micro_loss(inputs, j, weights):
        """forward with a graph; the fresh features spliced at position j among the cached ones (all of them fresh when nothing is cached)"""
        out = model(*inputs)
        nf = len(inputs)
        feats, scales = out[:nf], out[nf:]
        if accum_features:
            feats = [torch.cat(accum_features[k][:j] + [feats[k]] + accum_features[k][j + 1:]) for k in range(nf)]
        if three:
            return loss(*feats, *scales, t_weight1=weights[1], t_weight2=weights[2]), scales[0]
        return loss(*feats, *scales), scales[0]

    loss_m, batch_time_m, data_time_m = AverageMeter(), AverageMeter(), AverageMeter()
    end = time.time()
    for i, batch in enumerate(dataloader):
        i_accum = i // accum_freq
        step = num_batches_per_epoch * epoch + i_accum
        inputs, weights = unpack(batch)
        if not getattr(args, "skip_scheduler", False):
            scheduler(step)
        data_time_m.update(time.time() - end)

        if accum_freq == 1 and not three:
            logit_scale = unwrapped.logit_scale.detach().exp()
            total_loss = train_step(model, loss, inputs[0], inputs[1], optimizers, clip_grad=clip, reducers=reducers)
            micro = [total_loss]
        else:
            if accum_freq > 1:
                # first, the features of this batch without a graph
                with torch.no_grad():
                    out = model(*inputs)
                if not accum_features:
                    accum_features = [[] for _ in inputs]
                for k in range(len(inputs)):
                    accum_features[k].append(out[k])
                accum_inputs.append(inputs)
                accum_weights.append(weights)
                if ((i + 1) % accum_freq) > 0:
                    continue
            else:
                accum_inputs, accum_weights = [inputs], [weights]
            for o in optimizers:
                o.zero_grad()
            stacked = None
            if three:
                stacked = [w.to(device=device, non_blocking=True) for w in stack_weight_modalities(accum_weights)]
            micro = []
            for j in range(accum_freq):
                total_loss, logit_scale = micro_loss(accum_inputs[j], j, stacked)
                if reducers:
                    for r in reducers:
                        r.begin_backward(sync=(j == accum_freq - 1))
                total_loss.backward()
                micro.append(total_loss.detach())
            if reducers:
                for r in reducers:
                    r.finish()
                _average_temperature_grads(model, reducers)
            if clip is not None:
                torch.nn.utils.clip_grad_norm_([p for p in model.parameters() if p.grad is not None], clip, norm_type=2.0)
            for o in optimizers:
                o.step()
            accum_inputs, accum_features, accum_weights = [], [], []
            clamp_logit_scale(model)
            total_loss, logit_scale = micro[-1], logit_scale.detach()
        record["losses"].append(total_loss)
        record["micro_losses"].append(micro)
        record["steps"] += 1

        batch_time_m.update(time.time() - end)
        end = time.time()
        batch_count = i_accum + 1
        if is_master and (i_accum % log_every or batch_count == num_batches_per_epoch):
            batch_size = len(inputs[0])
            num_samples = batch_count * batch_size * world_size * accum_freq
            samples_per_epoch = dataloader.num_samples
            percent_complete = 100.0 * batch_count / num_batches_per_epoch
            # NOTE loss is coarsely sampled, just master node and per log update
            loss_m.update(total_loss.item(), batch_size)
            logit_scale_scalar = logit_scale.item()
            lr = optimizers[0].param_groups[0]["lr"]
            logging.info(
                f"Train Epoch: {epoch} [{num_samples:>{sample_digits}}/{samples_per_epoch} ({percent_complete:.0f}%)] "
                f"Loss: {loss_m.val:#.5g} ({loss_m.avg:#.4g}) "
                f"Data (t): {data_time_m.avg:.3f} "
                f"Batch (t): {batch_time_m.avg:.3f}, {total_train_batch_size / batch_time_m.val:#g}/s "
                f"LR: {lr:5f} "
                f"Logit Scale: {logit_scale_scalar:.3f}")
            log_data = {"loss": loss_m.val, "data_time": data_time_m.val, "batch_time": batch_time_m.val,
                        "samples_per_second": total_train_batch_size / batch_time_m.val, "scale": logit_scale_scalar, "lr": lr}
            for key, val in log_data.items():
                if tb_writer is not None:
                    tb_writer.add_scalar("train/" + key, val, step)
            batch_time_m.reset()
            data_time_m.reset()
    return record


def train_one_epoch(model, data, epoch, optimizers, scaler, scheduler, args, tb_writer=None, reducers=None, loss=None, fused=None):
    """training/train_retclip.py:64-240 in its order of operations: ``data['train'].set_epoch(epoch)``, ``dataloader.num_batches //
    args.accum_freq`` optimizer steps, ``scheduler(step)`` unless ``args.skip_scheduler``, ``args.grad_clip_norm``, the ``logit_scale``
    clamp, the reference's log line and ``tb_writer`` scalars (``train/loss``, ``data_time``, ``batch_time``, ``samples_per_second``,
    ``scale``, ``lr``).  ``args.multimodal_type``: 'default' (batch = (images, texts)), 'oct_ir', 'oct_faf_only' (batch =
    ({'oct', 'ir', 'f2_faf'}, (names, dataset index, modalities, h))); anything else raises NotImplementedError.

    ``accum_freq == 1`` is ``train_step``.  ``accum_freq > 1`` is open_clip's cached-feature accumulation, what every training script
    of the reference runs (``--accum-freq 4`` / ``8``): the features of ``accum_freq`` batches are cached under ``torch.no_grad()``;
    then every batch is run again with a graph, its fresh features spliced at its own position among the cached ones, so the loss sees
    the whole contrastive batch; one backward each, ONE optimizer step, the caches cleared.  A trailing incomplete group is dropped.
    Every micro-step's loss is the full-batch loss, so the tower gradients add up to the full-batch gradient while ``logit_scale.grad``
    ends up ``accum_freq`` times the full-batch derivative -- as in the reference, kept.

    ``optimizers``: one optimizer or a list (one per tower arena and one for the temperature); ``scheduler`` as ``cosine_lr`` builds it.
    ``reducers`` (``make_reducers``): ``begin_backward(sync=False)`` on every micro-step but the last, ``sync=True`` on the last and
    ``finish()`` once -- the result of the reference's exchange on every micro-step at 1 / accum_freq of the traffic (parallel.py); the
    temperature's gradient is averaged once, after the last micro-step.  Refused by name: a ``scaler`` (no GradScaler is run here),
    ``args.horovod``, ``args.wandb``, and the pure 16-bit ``args.precision`` values ('fp16', 'bf16'); under 'amp*' nothing is cast, the
    package is autocast-invariant.  The loss is built once per epoch as the reference builds it (``cache_labels=True``, rank / world size
    from ``args``); ``loss=`` replaces it by any callable of the same signature (tests), ``fused=`` chooses ``ClipLoss(fused=...)``,
    default ``FUSED_DEFAULT`` = False: at the shipped local-loss shape (32 x 256, two calls) the ATen composition measured 387 us per
    forward + backward on an MI355X and the fused path 819 us (profiles/cliploss_bench.txt).  Returns ``{"losses": [the last micro-step's loss of every optimizer step], "micro_losses": [[...]],
    "steps": n}`` (detached device tensors; the reference returns nothing)."""
    return _run_epoch("train_one_epoch", False, model, data, epoch, optimizers, scaler, scheduler, args, tb_writer, reducers, loss, fused)


def train_one_epoch_3modalities(model, data, epoch, optimizers, scaler, scheduler, args, tb_writer=None, reducers=None, loss=None,
                                fused=None):
    """training/train_retclip_3modalities.py:74-276: the same loop for ``args.multimodal_type == 'oct_faf_ir'`` -- ``model(oct, ir, faf)``
    returns three feature matrices and three temperatures, the loss is ``ThreeModalityClipLoss`` with the per-sample presence weights
    of the IR and FAF modalities (``batch[1][2]``: one flag vector per modality), which the accumulation caches per batch and
    concatenates over the group (``stack_weight_modalities``) beside the features.  Everything else as ``train_one_epoch``."""
    return _run_epoch("train_one_epoch_3modalities", True, model, data, epoch, optimizers, scaler, scheduler, args, tb_writer, reducers,
                      loss, fused)


# ---------------------------------------------------------------------------------------------------------------------------------
# validation: retrieval ranks (training/train_retclip.py:243-469, train_retclip_3modalities.py:542-604)
# ---------------------------------------------------------------------------------------------------------------------------------
# The reference moves the features to the CPU, forms the [N, N] logits there and argsorts every row twice (its own FIXME: "this does not
# scale past small eval datasets").  Everything it reports follows from one integer per sample and direction -- the number of candidates
# ranked before the true partner -- which ops.retrieval_ranks counts off f32 MFMA tiles of the feature product without storing it
# (csrc/retrieval.hip).  The host finishes in float64 with the reference's own expressions.  ``ranks=`` replaces the kernel by any
# function of the same signature (tests/retrieval_ref.py: numpy), as metrics.misc_measures_multi_label takes ``rank_counts=``.
def _device_ranks(a, b, **kw):
    if not (isinstance(a, torch.Tensor) and a.is_cuda):
        raise RuntimeError("retrieval metrics: the ranks come from the HIP kernel (ops.retrieval_ranks), which has no CPU fallback: pass "
                           "features on the device, or a ranks function")
    from . import ops
    return ops.retrieval_ranks(a, b, **kw)


def _feat(x):
    x = x.detach()
    return x if x.dtype == torch.float32 else x.float()


def _check_scale(name, logit_scale):
    v = float(logit_scale)
    if not (math.isfinite(v) and v > 0):
        raise ValueError(f"{name} must be finite and > 0, got {v}")
    return v


def _positions(ranks, pairs):
    """[(a, b), ...] -> one int64 numpy array per pair: the place of sample i's partner (column i) among the rows of b under a stable
    descending sort of the UNSCALED scores.  One device-to-host copy for all pairs together."""
    cols = [torch.as_tensor(ranks(a, b))[:, :2].sum(dim=1) for a, b in pairs]
    flat = torch.cat(cols).cpu().numpy().astype(np.int64)
    return np.split(flat, np.cumsum([c.shape[0] for c in cols])[:-1])


def _device_pair_ranks(pairs):
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for p in pairs for t in p):
        raise RuntimeError("retrieval metrics: the ranks come from the HIP kernel (ops.retrieval_pair_ranks), which has no CPU fallback: "
                           "pass features on the device, or a pair_ranks function")
    from . import ops
    return ops.retrieval_pair_ranks(pairs)


def _one_ranks_source(name, ranks, pair_ranks):
    if ranks is not None and pair_ranks is not None:
        raise ValueError(f"{name}: pass ranks= or pair_ranks=, not both")


def _pair_positions(pair_ranks, pairs):
    """[(a, b), ...] -> two int64 numpy arrays per pair, in order: the place of sample i's partner among the rows of b (the rows of the
    product), then among the rows of a (its columns).  One call, one device-to-host copy."""
    out = torch.as_tensor(pair_ranks(list(pairs)))
    n = pairs[0][0].shape[0]
    if tuple(out.shape) != (len(pairs), 2, n, 2):
        raise ValueError(f"pair_ranks returned {tuple(out.shape)}, expected {(len(pairs), 2, n, 2)}")
    pos = out.sum(dim=-1).cpu().numpy().astype(np.int64)
    return [pos[p, k] for p in range(len(pairs)) for k in (0, 1)]


def _rank_summary(metrics, name, preds):
    metrics[f"{name}_mean_rank"] = preds.mean() + 1
    metrics[f"{name}_median_rank"] = np.floor(np.median(preds)) + 1
    for k in [1, 5, 10]:
        metrics[f"{name}_R@{k}"] = np.mean(preds < k)


def get_metrics(image_features, text_features, logit_scale, ranks=None, pair_ranks=None):
    """train_retclip.get_metrics: ``{image_to_text, text_to_image}_{mean_rank, median_rank, R@1, R@5, R@10}``.  ``logit_scale`` is
    checked (finite, > 0) and does not enter the ranking: a positive factor changes no order.  Ties resolve by column index.
    ``pair_ranks=`` (a function of ``ops.retrieval_pair_ranks``' signature; not together with ``ranks=``): both directions from one
    walk over the product."""
    _check_scale("logit_scale", logit_scale)
    _one_ranks_source("get_metrics", ranks, pair_ranks)
    ranks = ranks or _device_ranks
    img, txt = _feat(image_features), _feat(text_features)
    if img.dim() != 2 or img.shape != txt.shape:
        raise ValueError(f"get_metrics: expected two [N, D] feature matrices, got {tuple(img.shape)} and {tuple(txt.shape)}")
    metrics = {}
    preds_all = _positions(ranks, [(img, txt), (txt, img)]) if pair_ranks is None else _pair_positions(pair_ranks, [(img, txt)])
    for name, preds in zip(("image_to_text", "text_to_image"), preds_all):
        _rank_summary(metrics, name, preds)
    return metrics


def get_metrics_3modalities(image_features, text1_features, text2_features, logit_scale, logit_scale1, logit_scale2, t_weight1,
                            t_weight2, ranks=None, pair_ranks=None):
    """train_retclip_3modalities.get_metrics_3modalities: the six directions among (image, text1, text2); every sample is ranked against
    ALL candidates and the summary is taken over the samples whose modality is present (``t_weight > 0``; ``t_weight1 * t_weight2``
    for the text1 / text2 pair).  A direction with no sample left raises ValueError.  ``pair_ranks=`` (a function of
    ``ops.retrieval_pair_ranks``' signature; not together with ``ranks=``): the six directions from one launch over the three products
    instead of six launches."""
    for nm, s in (("logit_scale", logit_scale), ("logit_scale1", logit_scale1), ("logit_scale2", logit_scale2)):
        _check_scale(nm, s)
    _one_ranks_source("get_metrics_3modalities", ranks, pair_ranks)
    ranks = ranks or _device_ranks
    img, t1, t2 = _feat(image_features), _feat(text1_features), _feat(text2_features)
    if img.dim() != 2 or img.shape != t1.shape or img.shape != t2.shape:
        raise ValueError(f"get_metrics_3modalities: expected three [N, D] feature matrices, got {tuple(img.shape)}, {tuple(t1.shape)}, "
                         f"{tuple(t2.shape)}")
    w1 = torch.as_tensor(t_weight1).detach().cpu().numpy().reshape(-1)
    w2 = torch.as_tensor(t_weight2).detach().cpu().numpy().reshape(-1)
    if w1.shape[0] != img.shape[0] or w2.shape[0] != img.shape[0]:
        raise ValueError(f"get_metrics_3modalities: t_weight1 / t_weight2 need {img.shape[0]} entries, got {w1.shape[0]} and {w2.shape[0]}")
    directions = (("image_to_text1", img, t1, w1), ("text1_to_image", t1, img, w1), ("image_to_text2", img, t2, w2),
                  ("text2_to_image", t2, img, w2), ("text1_to_text2", t1, t2, w1 * w2), ("text2_to_text1", t2, t1, w1 * w2))
    for name, _, _, w in directions:
        if not (w > 0).any():
            raise ValueError(f"get_metrics_3modalities: no sample with t_weight > 0 is left for {name}")
    metrics = {}
    if pair_ranks is None:
        preds_all = _positions(ranks, [(a, b) for _, a, b, _ in directions])
    else:                               # the rows and columns of three products, in the order of `directions`
        preds_all = _pair_positions(pair_ranks, [(img, t1), (img, t2), (t1, t2)])
    for (name, _, _, w), preds in zip(directions, preds_all):
        _rank_summary(metrics, name, preds[w > 0])
    return metrics


def _label_ids(labels):
    """labels of any hashable type -> (int ids in order of first occurrence [N], index of the LAST occurrence of each sample's label [N])."""
    if isinstance(labels, (torch.Tensor, np.ndarray)):
        labels = labels.tolist()
    ids, last, out = {}, {}, []
    for i, l in enumerate(labels):
        k = ids.setdefault(l, len(ids))
        last[k] = i
        out.append(k)
    ids_np = np.asarray(out, dtype=np.int32)
    return ids_np, np.asarray([last[k] for k in out], dtype=np.int32)


def get_corrected_metrics(image_features, text_features, logit_scale, labels, ranks=None):
    """train_retclip.get_corrected_metrics for evaluation sets in which one report (``labels[i]``) belongs to several images.
    Image-to-text: the sample's report ranked among the DISTINCT reports, each represented by its last occurrence (make_correct_labels).
    Text-to-image: micro and macro recall of ``logit >= 0`` against "same label" (the reference thresholds f32 sigmoid(logit) at 0.5)."""
    _check_scale("logit_scale", logit_scale)
    ranks = ranks or _device_ranks
    img, txt = _feat(image_features), _feat(text_features)
    ids, target = _label_ids(labels)
    if img.dim() != 2 or img.shape != txt.shape or ids.shape[0] != img.shape[0]:
        raise ValueError(f"get_corrected_metrics: expected two [N, D] feature matrices and N labels, got {tuple(img.shape)}, "
                         f"{tuple(txt.shape)} and {ids.shape[0]} labels")
    keep = np.zeros(ids.shape[0], dtype=np.uint8)
    keep[target] = 1
    dev = img.device
    group = torch.from_numpy(ids).to(dev)
    out = torch.as_tensor(ranks(img, txt, target=torch.from_numpy(target).to(dev), keep=torch.from_numpy(keep).to(dev), row_group=group,
                                col_group=group)).cpu().numpy().astype(np.int64)
    metrics = {}
    _rank_summary(metrics, "corrected_image_to_text", out[:, 0] + out[:, 1])
    metrics["corrected_text_to_image_micro_recall"] = out[:, 2].sum() / out[:, 3].sum()
    metrics["corrected_text_to_image_macro_recall"] = np.mean(out[:, 2] / out[:, 3])
    return metrics


# ---- which candidates come back: top-k retrieval (retDisease_eval/evaluate_results_test_train_visualize_all_models_top3_col_aireadi_
# laterality.py:186-270).  The script rebuilds the [N, N] logits from the features ``evaluate`` saved, overwrites the columns of the
# query's own patient with -1e5 and takes torch.topk for k = 1, 3, 5, 10; ops.retrieval_topk keeps the k best candidates per query
# while it walks the tiles of the ranks kernel (csrc/retrieval_topk.hip) and excludes the group instead of masking it.  ``topk=``
# replaces the kernel by any function of its signature (tests/retrieval_topk_ref.py: numpy), as ``ranks=`` does above.
def _device_topk(a, b, k, **kw):
    if not (isinstance(a, torch.Tensor) and a.is_cuda):
        raise RuntimeError("retrieve_topk: the lists come from the HIP kernel (ops.retrieval_topk), which has no CPU fallback: pass "
                           "features on the device, or a topk function")
    from . import ops
    return ops.retrieval_topk(a, b, k, **kw)


def _as_list(labels):
    return labels.tolist() if isinstance(labels, (torch.Tensor, np.ndarray)) else list(labels)


def retrieve_topk(query_features, gallery_features, k, query_groups=None, gallery_groups=None, keep=None, topk=None):
    """``(indices int64 [N, k], scores float32 [N, k])`` as numpy arrays: for every row of ``query_features`` [N, D] the k best rows of
    ``gallery_features`` [M, D] by the UNSCALED f32 score, equal scores by ascending index.  ``query_groups`` [N] / ``gallery_groups``
    [M] (both or neither; any hashable labels, e.g. patient ids, mapped to int32 ids through ONE dictionary for the two sides): a
    gallery row of the query's own group is no candidate.  ``keep`` [M]: != 0 marks the gallery rows that take part.  A query with
    fewer than k candidates has ``-1`` / ``-inf`` in the open slots.  ``topk=``: see above; without it the features must be on the GPU."""
    topk = topk or _device_topk
    q, g = _feat(torch.as_tensor(query_features)), _feat(torch.as_tensor(gallery_features))
    if q.dim() != 2 or g.dim() != 2 or q.shape[1] != g.shape[1]:
        raise ValueError(f"retrieve_topk: expected [N, D] queries and an [M, D] gallery, got {tuple(q.shape)} and {tuple(g.shape)}")
    if (query_groups is None) != (gallery_groups is None):
        raise ValueError("retrieve_topk: query_groups and gallery_groups are given together or not at all")
    kw = {}
    if query_groups is not None:
        ql, gl = _as_list(query_groups), _as_list(gallery_groups)
        if len(ql) != q.shape[0] or len(gl) != g.shape[0]:
            raise ValueError(f"retrieve_topk: {len(ql)} query groups and {len(gl)} gallery groups for {q.shape[0]} queries and "
                             f"{g.shape[0]} gallery rows")
        ids = {}
        kw["row_group"] = torch.tensor([ids.setdefault(l, len(ids)) for l in ql], dtype=torch.int32, device=q.device)
        kw["col_group"] = torch.tensor([ids.setdefault(l, len(ids)) for l in gl], dtype=torch.int32, device=q.device)
    if keep is not None:
        kept = torch.as_tensor(keep).reshape(-1)
        if kept.shape[0] != g.shape[0]:
            raise ValueError(f"retrieve_topk: keep needs {g.shape[0]} entries, got {kept.shape[0]}")
        kw["keep"] = (kept != 0).to(device=q.device, dtype=torch.uint8)
    idx, score = topk(q, g, int(k), **kw)
    idx = torch.as_tensor(idx).cpu().numpy().astype(np.int64)
    score = torch.as_tensor(score).cpu().numpy().astype(np.float32)
    if idx.shape != (q.shape[0], int(k)) or score.shape != idx.shape:
        raise ValueError(f"retrieve_topk: the topk function returned {idx.shape} / {score.shape} for {q.shape[0]} queries and k = {k}")
    return idx, score


def topk_match_accuracy(indices, query_attr, gallery_attr, topk_list=(1, 3, 5, 10)):
    """``{k: {"Micro Accuracy": ..., "Macro Accuracy": ...}}``: how often a retrieved row carries the query's attribute (the script's
    laterality score, for any attribute), in float64.  Micro: matches over filled slots among the first k of all rows; macro: the mean,
    over the rows with a filled slot, of matches over filled slots.  With every slot filled these are the script's
    ``sum(matched) / (N k)`` and ``mean(sum(matched, 1) / k)``; a ``-1`` slot counts neither as a match nor as a slot (NaN when
    no slot is filled at all).  A k beyond ``indices.shape[1]`` raises ValueError."""
    idx = np.asarray(indices)
    qa, ga = np.asarray(_as_list(query_attr)), np.asarray(_as_list(gallery_attr))
    if idx.ndim != 2 or qa.shape != (idx.shape[0],) or ga.ndim != 1:
        raise ValueError(f"topk_match_accuracy: expected indices [N, K], N query and M gallery attributes, got {idx.shape}, {qa.shape}, "
                         f"{ga.shape}")
    if idx.size and (idx.max() >= ga.shape[0] or idx.min() < -1):
        raise ValueError(f"topk_match_accuracy: an index lies outside [-1, {ga.shape[0]})")
    out = {}
    for k in topk_list:
        if not 1 <= k <= idx.shape[1]:
            raise ValueError(f"topk_match_accuracy: k = {k} with lists of {idx.shape[1]}")
        sub = idx[:, :k]
        filled = sub >= 0
        matched = filled & (ga[np.where(filled, sub, 0)] == qa[:, None]) if ga.shape[0] else np.zeros_like(filled)
        slots, hits = filled.sum(axis=1).astype(np.float64), matched.sum(axis=1).astype(np.float64)
        some = slots > 0
        micro = hits.sum() / slots.sum() if some.any() else float("nan")
        macro = float(np.mean(hits[some] / slots[some])) if some.any() else float("nan")
        out[k] = {"Micro Accuracy": float(micro), "Macro Accuracy": macro}
    return out


def retrieval_report(results, attribute, groups, output_dir, model_name, topk_list=(1, 3, 5, 10), ir_oct=False,
                     attribute_name="laterality", topk=None):
    """The script's retrieval table from what ``evaluate(..., save_retrieval_results=True)`` wrote.  ``results``: the path of a
    ``retrieval_results_{epoch}.npz`` or the dict of its arrays; the queries are ``image_features`` and the gallery ``text_features``
    (``ir_oct=True``: the other way round, the script's swap).  ``attribute`` [N] (e.g. 1 for a right eye) and ``groups`` [N] (e.g.
    patient ids) describe sample i on both sides; gallery rows of the query's group are excluded.  Writes
    ``<output_dir>/<model_name>_<attribute_name>[_ir].csv`` as pandas writes the script's ``DataFrame(results).to_csv(index=False)``:
    the k values, the micro row, the macro row (float64 values).  Returns ``{"accuracy", "indices", "scores"}`` with lists of
    ``max(topk_list)``.  Features loaded from a file go to the GPU when there is one and no ``topk=`` is given."""
    import csv
    import os
    if isinstance(results, (str, os.PathLike)):
        with np.load(results) as z:
            results = {key: z[key] for key in ("image_features", "text_features")}
    img, txt = torch.as_tensor(results["image_features"]), torch.as_tensor(results["text_features"])
    if topk is None and not img.is_cuda and torch.cuda.is_available():
        img, txt = img.cuda(), txt.cuda()
    query, gallery = (txt, img) if ir_oct else (img, txt)
    topk_list = [int(k) for k in topk_list]
    if not topk_list or min(topk_list) < 1:
        raise ValueError(f"retrieval_report: topk_list must hold positive ints, got {topk_list}")
    indices, scores = retrieve_topk(query, gallery, max(topk_list), query_groups=groups, gallery_groups=groups, topk=topk)
    accuracy = topk_match_accuracy(indices, attribute, attribute, topk_list)
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(output_dir, f"{model_name}_{attribute_name}{'_ir' if ir_oct else ''}.csv")
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(list(accuracy))
        for row in ("Micro Accuracy", "Macro Accuracy"):
            w.writerow([accuracy[k][row] for k in accuracy])
    return {"accuracy": accuracy, "indices": indices, "scores": scores}


def _eval_corrected_label(text_features, t=10 ** (-8)):
    """evaluate's own get_corrected_label (train_retclip.py:257-263): 1 where two reports of the batch have the same features."""
    f = text_features.detach()
    d = torch.sqrt(((f.unsqueeze(1) - f.unsqueeze(0)) ** 2).sum(dim=-1))
    return (d <= t).to(text_features.dtype)


def evaluate(model, data, epoch, args, tb_writer=None):
    """The validation half of train_retclip.evaluate: features of ``data['val'].dataloader`` stay ON THE DEVICE, the per-batch loss
    (symmetric cross entropy, or BCE against the duplicate-report targets with ``args.correct_label``) is weighted by batch size and
    summed on the device with one synchronisation at the end, and the retrieval metrics come from ``get_metrics``.  Returns ``{}``
    off the main process or when validation is not due; otherwise the ten metrics plus ``val_loss``, ``epoch``, ``num_samples``.
    With ``args.save_retrieval_results`` the features go to ``retrieval_results_{epoch}.npz``; a positive int ``args.retrieval_topk``
    adds the k best partners of every sample in both directions (``topk_image_to_text``, ``topk_text_to_image``, int32 [N, k], and
    their ``*_scores``; nothing excluded -- ``retrieval_report`` excludes by group).
    Zero-shot evaluation and wandb are not part of this package."""
    import json
    import logging
    import os
    from . import misc
    metrics = {}
    if not misc.is_main_process():
        return metrics
    mm = getattr(args, "multimodal_type", "default")
    if mm not in (None, "default"):
        raise NotImplementedError(f"evaluate: multimodal_type {mm!r} is not supported (only 'default')")
    val_frequency = getattr(args, "val_frequency", 0)
    if not ("val" in data and (val_frequency and ((epoch % val_frequency) == 0 or epoch == getattr(args, "epochs", None)))):
        return metrics
    device = torch.device(getattr(args, "device", "cuda"))
    model.eval()
    dataloader = data["val"].dataloader
    samples_per_val = getattr(dataloader, "num_samples", None)
    correct_label = bool(getattr(args, "correct_label", 0))
    return_metainfo = bool(getattr(args, "return_metainfo", False))
    num_samples = 0
    cumulative_loss = torch.zeros((), dtype=torch.float32, device=device)
    all_image, all_text, all_scale, all_labels = [], [], [], []
    logit_scale = None
    with torch.no_grad():
        for i, batch in enumerate(dataloader):
            if return_metainfo:
                images, texts, labels = batch
                all_labels.extend(labels.tolist() if isinstance(labels, (torch.Tensor, np.ndarray)) else list(labels))
            else:
                images, texts = batch
            images = images.to(device=device, non_blocking=True)
            texts = texts.to(device=device, non_blocking=True)
            image_features, text_features, logit_scale = model(images, texts)
            with torch.autocast(device_type=device.type, enabled=False):
                image_features, text_features = image_features.float(), text_features.float()
                logit_scale = logit_scale.float().mean()
                logits_per_image = logit_scale * image_features @ text_features.t()
                logits_per_text = logits_per_image.t()
                batch_size = images.shape[0]
                if correct_label:
                    targets = _eval_corrected_label(text_features)
                    total_loss = (F.binary_cross_entropy_with_logits(logits_per_image, targets)
                                  + F.binary_cross_entropy_with_logits(logits_per_text, targets)) / 2
                else:
                    targets = torch.arange(batch_size, device=device).long()
                    total_loss = (F.cross_entropy(logits_per_image, targets) + F.cross_entropy(logits_per_text, targets)) / 2
                cumulative_loss += total_loss * batch_size
            all_image.append(image_features)
            all_text.append(text_features)
            all_scale.append(logit_scale)
            num_samples += batch_size
            if (i % 100) == 0:
                logging.info(f"Eval Epoch: {epoch} [{num_samples} / {samples_per_val}]")
        if num_samples == 0:
            raise ValueError("evaluate: the validation loader is empty")
        image_all, text_all = torch.cat(all_image), torch.cat(all_text)
        val_metrics = get_metrics(image_features=image_all, text_features=text_all, logit_scale=logit_scale)
        loss = cumulative_loss / num_samples
        metrics.update({**{k: float(v) for k, v in val_metrics.items()}, "val_loss": loss.item(), "epoch": epoch,
                        "num_samples": num_samples})
    logging.info(f"Eval Epoch: {epoch} " + "\t".join([f"{k}: {round(v, 4):.4f}" for k, v in metrics.items()]))
    if getattr(args, "save_logs", False):
        for name, val in metrics.items():
            if tb_writer is not None:
                tb_writer.add_scalar(f"val/{name}", val, epoch)
        with open(os.path.join(args.checkpoint_path, "results.jsonl"), "a+") as f:
            f.write(json.dumps(metrics))
            f.write("\n")
        if getattr(args, "save_retrieval_results", False):
            arrays = {"image_features": image_all.cpu().numpy(), "text_features": text_all.cpu().numpy(),
                      "logit_scale": torch.stack(all_scale).cpu().numpy()}
            if all_labels:
                arrays["labels"] = np.asarray(all_labels)
            k = getattr(args, "retrieval_topk", 0) or 0
            if isinstance(k, int) and k > 0:
                # the k best partners of every sample in both directions, nothing excluded (retrieval_report excludes by group)
                from . import ops
                for name, a, b in (("topk_image_to_text", image_all, text_all), ("topk_text_to_image", text_all, image_all)):
                    idx, score = ops.retrieval_topk(a, b, k)
                    arrays[name], arrays[name + "_scores"] = idx.cpu().numpy(), score.cpu().numpy()
            np.savez(os.path.join(args.checkpoint_path, f"retrieval_results_{epoch}.npz"), **arrays)
    return metrics


# ---- validation of the other recipes (train_retclip.py:290-300 for 'oct_ir' / 'oct_faf_only', train_retclip_3modalities.py:279-538 for
# 'oct_faf_ir').  ``evaluate`` above stays the 'default' loop, untouched; the loops below take dict batches as ``_run_epoch`` does and
# may draw every direction's ranks from one launch of ops.retrieval_pair_ranks (csrc/retrieval_pair.hip).  Whether they do without being
# asked is PAIR_RANKS_DEFAULT, True only if the one launch is not slower than the launches it replaces at N = 3000: measured on an
# MI355X at D = 512 (tools/bench_pair_ranks.py, profiles/pair_ranks_bench.txt; DESIGN.md section 4 holds the table, as for
# FUSED_DEFAULT), one P = 3 launch takes 1.63 ms against 4.65 ms for the six launches.
PAIR_RANKS_DEFAULT = True


def _pair_ranks_arg(pair_ranks):
    """None: PAIR_RANKS_DEFAULT; True / False: the pair kernel / the per-direction kernel; a function: that function."""
    if pair_ranks is None:
        pair_ranks = PAIR_RANKS_DEFAULT
    if pair_ranks is True:
        return _device_pair_ranks
    return None if pair_ranks is False else pair_ranks


def _masked_pair_term(loss_rows, w):
    """sum(loss * w) / sum(w), 0 where sum(w) == 0 -- chosen on the device, without a division by that zero and without a read-back"""
    den = w.sum()
    return torch.where(den == 0, torch.zeros_like(den), (loss_rows * w).sum() / torch.where(den == 0, torch.ones_like(den), den))


def three_way_val_loss(image_features, text1_features, text2_features, logit_scale, logit_scale1, logit_scale2, w1, w2, correct_label=False):
    """The per-batch validation loss of train_retclip_3modalities.evaluate (:407-467): six ``cross_entropy(reduction='none')`` terms on
    the three in-batch logit matrices and their transposes; image / text1 weighted by ``w1`` over ``w1.sum()``, image / text2 by ``w2``
    over ``w2.sum()`` and text1 / text2 by ``w1`` ALONE over ``w1.sum()`` (:451-463 -- not the ``w1 * w2`` of ThreeModalityClipLoss),
    a zero weight sum giving 0 for its two terms; the sum over 6.  ``correct_label``: the targets are the 0 / 1 same-feature matrix of
    text1, which ``cross_entropy`` takes as class probabilities (the reference builds a BCE criterion there and never uses it)."""
    l0 = logit_scale * image_features @ text1_features.t()
    l1 = logit_scale1 * image_features @ text2_features.t()
    l2 = logit_scale2 * text1_features @ text2_features.t()
    if correct_label:
        targets = _eval_corrected_label(text1_features)
    else:
        targets = torch.arange(image_features.shape[0], device=image_features.device).long()
    total = 0.0
    for logits, w in ((l0, w1), (l1, w2), (l2, w1)):
        total = total + _masked_pair_term(F.cross_entropy(logits, targets, reduction="none"), w)
        total = total + _masked_pair_term(F.cross_entropy(logits.t(), targets, reduction="none"), w)
    return total / 6


def _evaluate_dict_batches(name, mm, model, data, epoch, args, tb_writer, pair_ranks):
    """The loop behind ``evaluate_3modalities`` (mm == 'oct_faf_ir') and the two-tower dict-batch types of ``evaluate_multimodal``:
    ``evaluate``'s gates, device-side accumulation, log line and files around the batch format of ``_run_epoch``."""
    import json
    import logging
    import os
    from . import misc
    metrics = {}
    if not misc.is_main_process():
        return metrics
    val_frequency = getattr(args, "val_frequency", 0)
    if not ("val" in data and (val_frequency and ((epoch % val_frequency) == 0 or epoch == getattr(args, "epochs", None)))):
        return metrics
    three = mm == "oct_faf_ir"
    device = torch.device(getattr(args, "device", "cuda"))
    model.eval()
    dataloader = data["val"].dataloader
    samples_per_val = getattr(dataloader, "num_samples", None)
    correct_label = bool(getattr(args, "correct_label", 0))
    pair_ranks = _pair_ranks_arg(pair_ranks)
    num_samples = 0
    cumulative_loss = torch.zeros((), dtype=torch.float32, device=device)
    all_feats, all_scales, all_weights = [], [], []
    scales = None
    with torch.no_grad():
        for i, batch in enumerate(dataloader):
            images, texts_ir, texts_f2_faf = batch[0]["oct"], batch[0]["ir"], batch[0]["f2_faf"]
            modalities = batch[1][2]
            if mm == "oct_ir":
                inputs = (images, texts_ir)
            elif mm == "oct_faf_only":
                assert sum(modalities[2]) == len(modalities[2]), "Only f2_faf is allowed in this setting"
                inputs = (images, texts_f2_faf)
            else:
                inputs = (images, texts_ir, texts_f2_faf)
                weights = [convert_modalities_idx_to_flag(mod) for mod in modalities[:3]]
                all_weights.append(weights)
            inputs = tuple(x.to(device=device, non_blocking=True) for x in inputs)
            out = model(*inputs)
            nf = len(inputs)
            with torch.autocast(device_type=device.type, enabled=False):
                feats = [f.float() for f in out[:nf]]
                scales = [s.float().mean() for s in out[nf:]]
                batch_size = inputs[0].shape[0]
                if three:
                    w1, w2 = (w.to(device=device, dtype=torch.float32, non_blocking=True) for w in weights[1:3])
                    total_loss = three_way_val_loss(*feats, *scales, w1, w2, correct_label)
                else:
                    logits_per_image = scales[0] * feats[0] @ feats[1].t()
                    logits_per_text = logits_per_image.t()
                    if correct_label:
                        targets = _eval_corrected_label(feats[1])
                        total_loss = (F.binary_cross_entropy_with_logits(logits_per_image, targets)
                                      + F.binary_cross_entropy_with_logits(logits_per_text, targets)) / 2
                    else:
                        targets = torch.arange(batch_size, device=device).long()
                        total_loss = (F.cross_entropy(logits_per_image, targets) + F.cross_entropy(logits_per_text, targets)) / 2
                cumulative_loss += total_loss * batch_size
            all_feats.append(feats)
            all_scales.append(torch.stack(scales))
            num_samples += batch_size
            if (i % 100) == 0:
                logging.info(f"Eval Epoch: {epoch} [{num_samples} / {samples_per_val}]")
        if num_samples == 0:
            raise ValueError(f"{name}: the validation loader is empty")
        feats_all = [torch.cat([f[k] for f in all_feats]) for k in range(len(all_feats[0]))]
        if three:
            weights_all = stack_weight_modalities(all_weights)
            val_metrics = get_metrics_3modalities(*feats_all, *scales, t_weight1=weights_all[1], t_weight2=weights_all[2],
                                                  pair_ranks=pair_ranks)
        else:
            val_metrics = get_metrics(image_features=feats_all[0], text_features=feats_all[1], logit_scale=scales[0], pair_ranks=pair_ranks)
        loss = cumulative_loss / num_samples
        metrics.update({**{k: float(v) for k, v in val_metrics.items()}, "val_loss": loss.item(), "epoch": epoch,
                        "num_samples": num_samples})
    logging.info(f"Eval Epoch: {epoch} " + "\t".join([f"{k}: {round(v, 4):.4f}" for k, v in metrics.items()]))
    if getattr(args, "save_logs", False):
        for key, val in metrics.items():
            if tb_writer is not None:
                tb_writer.add_scalar(f"val/{key}", val, epoch)
        with open(os.path.join(args.checkpoint_path, "results.jsonl"), "a+") as f:
            f.write(json.dumps(metrics))
            f.write("\n")
        if getattr(args, "save_retrieval_results", False):
            stacked = torch.stack(all_scales).cpu().numpy()                    # [batches, towers - 1 .. 3]
            if three:
                arrays = {"image_features": feats_all[0].cpu().numpy(), "text1_features": feats_all[1].cpu().numpy(),
                          "text2_features": feats_all[2].cpu().numpy(), "t_weight1": weights_all[1].cpu().numpy(),
                          "t_weight2": weights_all[2].cpu().numpy(), "logit_scale": stacked}
            else:
                arrays = {"image_features": feats_all[0].cpu().numpy(), "text_features": feats_all[1].cpu().numpy(),
                          "logit_scale": stacked[:, 0]}
            np.savez(os.path.join(args.checkpoint_path, f"retrieval_results_{epoch}.npz"), **arrays)
    return metrics


def evaluate_3modalities(model, data, epoch, args, tb_writer=None, pair_ranks=None):
    """train_retclip_3modalities.evaluate for ``args.multimodal_type == 'oct_faf_ir'``: ``model(oct, ir, faf)`` on dict batches
    (``batch[0]['oct' / 'ir' / 'f2_faf']``, presence flags ``batch[1][2]``, as ``train_one_epoch_3modalities`` takes them), the
    per-batch ``three_way_val_loss`` in f32 outside any autocast, weighted by batch size and summed on the device with one
    synchronisation at the end, and ``get_metrics_3modalities`` on the concatenated device features with the LAST batch's three
    temperatures and the concatenated weights.  Gates, log line, ``results.jsonl`` and ``tb_writer`` scalars as ``evaluate``; returns
    ``{}`` off the main process or when validation is not due, otherwise the 30 metrics plus ``val_loss``, ``epoch``, ``num_samples``.
    ``pair_ranks``: None = ``PAIR_RANKS_DEFAULT``, True / False = the six directions from one launch of ``ops.retrieval_pair_ranks`` /
    from six of ``ops.retrieval_ranks`` (the same integers), or a function of the former's signature.
    With ``args.save_retrieval_results``: ``retrieval_results_{epoch}.npz`` with ``image_features``, ``text1_features``,
    ``text2_features``, ``t_weight1``, ``t_weight2`` and ``logit_scale`` [batches, 3].  Departures: the reference's own saving block
    names variables it never defines (it cannot run); zero-shot evaluation and wandb are not part of this package; a direction with no
    present sample raises ValueError (``get_metrics_3modalities``) where the reference reports the mean of an empty selection."""
    return _evaluate_dict_batches("evaluate_3modalities", "oct_faf_ir", model, data, epoch, args, tb_writer, pair_ranks)


def evaluate_multimodal(model, data, epoch, args, tb_writer=None, pair_ranks=None):
    """What a driver binds as ``evaluate``: dispatch on ``args.multimodal_type``.  None / 'default': ``evaluate``, unchanged (tuple
    batches; ``pair_ranks`` plays no part).  'oct_ir' / 'oct_faf_only': the two-tower loop of train_retclip.py:292-300 on
    ``batch[0]['oct']`` and ``batch[0]['ir']`` / ``batch[0]['f2_faf']`` (the latter with the reference's assertion that every FAF flag
    is set), with ``evaluate``'s loss, ``correct_label`` BCE included, and the ``get_metrics`` keys; the saved file holds
    ``image_features``, ``text_features`` and ``logit_scale`` (no labels, no top-k lists).  'oct_faf_ir': ``evaluate_3modalities``.
    Anything else ('oct_f2_faf_inplace' included, which the reference leaves unfinished) raises NotImplementedError."""
    from . import misc
    if not misc.is_main_process():
        return {}
    mm = getattr(args, "multimodal_type", "default")
    if mm in (None, "default"):
        return evaluate(model, data, epoch, args, tb_writer)
    if mm == "oct_faf_ir":
        return evaluate_3modalities(model, data, epoch, args, tb_writer, pair_ranks)
    if mm in ("oct_ir", "oct_faf_only"):
        return _evaluate_dict_batches("evaluate_multimodal", mm, model, data, epoch, args, tb_writer, pair_ranks)
    raise NotImplementedError(f"evaluate_multimodal: multimodal_type {mm!r} is not supported (only 'default', 'oct_ir', 'oct_faf_only', "
                              "'oct_faf_ir')")
