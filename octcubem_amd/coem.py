"""COEM (contrastive OCT / en-face pre-training) step pieces -- SURVEY section 8f N4, counterparts of
``retinal-COEM/src/open_clip``: ``loss.gather_features`` / ``ClipLoss`` (loss.py:21-65, :148-230), ``model.CustomTextCLIP``
(model.py:635-682: two towers, ``logit_scale = log(1 / 0.07)``, L2-normalised features) and the per-step clamp of
``logit_scale`` to [0, log 100] (training/train_retclip.py).

The towers are the 3-D ST ViT (``models_vit_st``, OCT volume) and the 2-D ViT (``models_vit``, IR image) of this package; their
``head`` is the projection to the shared embedding.  The loss acts on ``[B, embed]`` features: a ``[B_global, B_global]``
logits matmul and two cross-entropies -- a few MFLOP next to the towers' TFLOPs, left to ATen on the device.  With
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


@autocast_invariant
class ClipLoss(nn.Module):
    def __init__(self, local_loss=False, gather_with_grad=False, cache_labels=False, rank=0, world_size=1, use_horovod=False,
                 correct_label=0):
        super().__init__()
        self.local_loss = local_loss
        self.gather_with_grad = gather_with_grad
        self.cache_labels = cache_labels
        self.rank = rank
        self.world_size = world_size
        self.use_horovod = use_horovod
        self.correct_label = correct_label
        self.prev_num_logits = 0
        self.labels = {}

    def get_corrected_label(self, enface_features_i, enface_features_j, t=10 ** (-100)):
        """Soft labels that share the target mass among samples with IDENTICAL en-face features (same report)."""
        d = torch.cdist(enface_features_i.detach().float(), enface_features_j.detach().float())
        L = (d <= t).to(enface_features_i.dtype)
        return L / torch.sum(L, dim=1, keepdim=True)

    def forward(self, image_features, enface_features, logit_scale):
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
    the mean of the six directed terms."""

    def __init__(self, local_loss=False, gather_with_grad=False, cache_labels=False, rank=0, world_size=1, use_horovod=False,
                 correct_label=0):
        super().__init__()
        self.local_loss = local_loss
        self.gather_with_grad = gather_with_grad
        self.cache_labels = cache_labels
        self.rank = rank
        self.world_size = world_size
        self.use_horovod = use_horovod
        self.correct_label = correct_label
        self.prev_num_logits = 0
        self.labels = {}

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


def build_towers_from_config(cfg: dict, flash_semantics: bool = True):
    """Config-driven construction of the two towers, for the model configs the reference ships for this path
    (retinal-COEM/src/open_clip/model_configs/vit_large_patch16_retFound-vit_large_patch16_OCTCube.json through
    open_clip/model.py ``_build_vision_tower`` :190-290 and ``_build_text_tower`` :462-509):

      vision_cfg.model_name  "ViT_ST" | "ViT_ST_nodrop"   -> the 3-D spatio-temporal ViT (models_vit_st), ``out_dim = embed_dim`` head,
                             sep_pos_embed / cls_embed on, dropout before the head only for "ViT_ST"
      text_cfg.vit_model_name "ViT_flash_attn"             -> the 2-D ViT (models_vit) on the en-face image

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
    if "ViT_flash_attn" not in tname or "mod" in tname:
        raise NotImplementedError(f"en-face tower {tname!r}: only ViT_flash_attn is built")
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


def create_model_from_config(cfg: dict, **kw) -> "CustomTextCLIP":
    """CustomTextCLIP(embed_dim, vision_cfg, text_cfg) of open_clip/model.py:635-646 for the configs above."""
    visual, text = build_towers_from_config(cfg, **kw)
    return CustomTextCLIP(visual, text)


def make_reducers(model, comm=None, **kw):
    """One FlatGradReducer per tower (each tower is a model with its own flat gradient arena)."""
    from .parallel import FlatGradReducer
    m = getattr(model, "module", model)
    return [FlatGradReducer(m.visual, comm=comm, **kw), FlatGradReducer(m.text, comm=comm, **kw)]


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


def _rank_summary(metrics, name, preds):
    metrics[f"{name}_mean_rank"] = preds.mean() + 1
    metrics[f"{name}_median_rank"] = np.floor(np.median(preds)) + 1
    for k in [1, 5, 10]:
        metrics[f"{name}_R@{k}"] = np.mean(preds < k)


def get_metrics(image_features, text_features, logit_scale, ranks=None):
    """train_retclip.get_metrics: ``{image_to_text, text_to_image}_{mean_rank, median_rank, R@1, R@5, R@10}``.  ``logit_scale`` is
    checked (finite, > 0) and does not enter the ranking: a positive factor changes no order.  Ties resolve by column index."""
    _check_scale("logit_scale", logit_scale)
    ranks = ranks or _device_ranks
    img, txt = _feat(image_features), _feat(text_features)
    if img.dim() != 2 or img.shape != txt.shape:
        raise ValueError(f"get_metrics: expected two [N, D] feature matrices, got {tuple(img.shape)} and {tuple(txt.shape)}")
    metrics = {}
    for name, preds in zip(("image_to_text", "text_to_image"), _positions(ranks, [(img, txt), (txt, img)])):
        _rank_summary(metrics, name, preds)
    return metrics


def get_metrics_3modalities(image_features, text1_features, text2_features, logit_scale, logit_scale1, logit_scale2, t_weight1,
                            t_weight2, ranks=None):
    """train_retclip_3modalities.get_metrics_3modalities: the six directions among (image, text1, text2); every sample is ranked against
    ALL candidates and the summary is taken over the samples whose modality is present (``t_weight > 0``; ``t_weight1 * t_weight2``
    for the text1 / text2 pair).  A direction with no sample left raises ValueError."""
    for nm, s in (("logit_scale", logit_scale), ("logit_scale1", logit_scale1), ("logit_scale2", logit_scale2)):
        _check_scale(nm, s)
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
    for (name, _, _, w), preds in zip(directions, _positions(ranks, [(a, b) for _, a, b, _ in directions])):
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
            np.savez(os.path.join(args.checkpoint_path, f"retrieval_results_{epoch}.npz"), **arrays)
    return metrics
