"""2-D flash-attention ViT (RETFound-center, ``patient_dataset_type`` ``Center2D_flash_attn``): drop-in for the reference's
``OCTCube/models_vit_flash_attn.py`` ``VisionTransformer`` (constructor :50-115, ``forward_features`` :118-151, ``forward`` :153-158,
``load_state_dict_to_backbone`` :160-183) and its factory ``flash_attn_vit_large_patch16``.

The blocks, patch embedding and assembly are models_vit's (timm layout: ``blocks.i.attn.qkv``; GPU only).  What the flash model
adds on top of models_vit.VisionTransformer:
  * ``flash_compat`` (default: ``use_flash_attn``): flash-attn's prenorm Block hands back its MLP branch without the residual
    stream, and the reference pools / norms what the LAST block returned -- the last block runs with ``final_residual=False``
    (the convention of models_vit_st / models_mae);
  * ``hidden_states=True``: the list of per-block outputs instead of the features;
  * ``fused_pool=True`` (opt-in): the pooling and ``fc_norm`` / ``norm`` of the cls row go through ops.SlicePoolFn (one HIP
    kernel chain) instead of ATen's mean and the LayerNorm kernel;
  * the reference's extra keyword arguments (``qkv_bias``, ``use_flash_attn``, ``dropout``, ``drop_rate=0``) are accepted;
    ``self.dropout`` is built and, as in the reference, never applied.
Parameter names are the timm layout of the non-flash model; ``load_state_dict_to_backbone`` takes timm (RETFound) or flash
(``mixer.Wqkv`` / ``mixer.out_proj``) checkpoints and reports missing / unexpected keys in the reference's flash names."""
from __future__ import annotations

import re
from collections import OrderedDict
from functools import partial

import torch
import torch.nn as nn

from . import models_vit, ops, video_vit
from .arena import get_arena
from .video_vit import layer_norm
from ._autocast import autocast_invariant


def to_timm_layout(state_dict):
    """flash (``mixer.Wqkv`` / ``mixer.out_proj``) or split (``attn.q/k/v``) block keys -> timm ``attn.qkv`` / ``attn.proj``."""
    out = OrderedDict()
    for k, v in state_dict.items():
        k = re.sub(r"(blocks\.\d+)\.mixer\.out_proj\.", r"\1.attn.proj.", k)
        k = re.sub(r"(blocks\.\d+)\.mixer\.Wqkv\.", r"\1.attn.qkv.", k)
        m = re.match(r"(.*blocks\.\d+)\.attn\.([qkv])\.(weight|bias)$", k)
        if m:
            if m.group(2) == "q":
                pre, kind = m.group(1), m.group(3)
                parts = [state_dict.get(f"{pre}.attn.{n}.{kind}") for n in "qkv"]
                if all(p is not None for p in parts):
                    out[f"{pre}.attn.qkv.{kind}"] = torch.cat(parts, dim=0)
            continue
        out[k] = v
    return out


def _flash_name(k):
    """timm block key -> the name the reference's flash model gives the same parameter."""
    k = re.sub(r"(blocks\.\d+)\.attn\.proj\.", r"\1.mixer.out_proj.", k)
    return re.sub(r"(blocks\.\d+)\.attn\.qkv\.", r"\1.mixer.Wqkv.", k)


@autocast_invariant
class VisionTransformer(models_vit.VisionTransformer):
    """Vision Transformer with support for global average pooling (flash-attn semantics by default)"""

    def __init__(self, img_size=256, num_classes=400, embed_dim=768, depth=12, patch_size=16, in_chans=3, global_pool=False,
                 use_flash_attn=True, num_heads=12, mlp_ratio=4.0, no_qkv_bias=False, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0,
                 drop_path_rate=0.0, norm_layer=nn.LayerNorm, dropout=0.5, cls_embed=True, flash_compat=None, fused_pool=False,
                 **kwargs):
        if not cls_embed:
            raise NotImplementedError("built for cls_embed=True (how every reference script calls it)")
        kwargs.pop("qkv_bias", None)        # the factories pass qkv_bias=True; the flash blocks take ``not no_qkv_bias``
        kwargs.pop("drop_date", None)
        super().__init__(img_size=img_size, patch_size=patch_size, in_chans=in_chans, num_classes=num_classes, embed_dim=embed_dim,
                         depth=depth, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=not no_qkv_bias, qk_scale=qk_scale,
                         drop_rate=drop_rate, attn_drop_rate=attn_drop_rate, drop_path_rate=drop_path_rate, norm_layer=norm_layer,
                         global_pool=global_pool)
        self.use_flash_attn = bool(use_flash_attn)
        self.flash_compat = self.use_flash_attn if flash_compat is None else bool(flash_compat)
        self.fused_pool = bool(fused_pool)
        self.cls_embed = cls_embed
        self.depth = depth
        self.dropout = nn.Dropout(dropout)      # built, never applied (models_vit_flash_attn.py:111, forward :153-158)
        self.head = nn.Linear(embed_dim, num_classes)
        torch.nn.init.normal_(self.head.weight, std=0.02)

    def _tokens(self, x, hidden_states=False):
        """[N, C, H, W] -> the token stream after the last block, fp32 [N, 1 + L, D] (or the list of per-block outputs)."""
        self.prepare()
        x = x.float().contiguous()
        N, L = x.shape[0], self.patch_embed.num_patches
        tok = self.patch_embed.embed_tokens(x)
        if self._ids is None or self._ids.shape[0] != N or self._ids.device != x.device:
            object.__setattr__(self, "_ids", torch.arange(L, device=x.device, dtype=torch.int64).expand(N, L).contiguous())
        pe = self.pos_embed[0]
        x = ops.EncAssembleFn.apply(tok, pe[1:], self.cls_token, pe[:1].view(1, 1, -1), self._ids, self._ids)
        hs = []
        last = len(self.blocks) - 1
        for i, blk in enumerate(self.blocks):
            x = blk(x, final_residual=not (self.flash_compat and i == last))
            hs.append(x)
        return hs if hidden_states else x

    def _pool(self, x, S=1, fused=None):
        """fp32 [N, 1 + L, D] -> fp32 [N / S, D]: mean over the S slices of (fc_norm(mean of the patch tokens) | norm(x)[:, 0])."""
        norm = self.fc_norm if self.global_pool else self.norm
        if self.fused_pool if fused is None else fused:
            return ops.SlicePoolFn.apply(x, norm.weight, norm.bias, norm.eps, S, not self.global_pool)
        if self.global_pool:
            f = layer_norm(norm, x[:, 1:, :].mean(dim=1).contiguous()).float()
        else:
            f = layer_norm(norm, x[:, :1, :].contiguous())[:, 0].float()
        return f if S == 1 else f.view(-1, S, f.shape[-1]).mean(dim=1)

    def forward_features(self, x, hidden_states=False):
        x = self._tokens(x, hidden_states)
        if hidden_states:
            return x
        return self._pool(x)

    def _head(self, x):
        if self.head.out_features % 8 == 0:
            arena = get_arena(self)
            return ops.LinearFn.apply(x, arena.lp_view(self.head.weight), arena.f32_view(self.head.bias),
                                      lambda: arena.grad_view(self.head.weight), lambda: arena.grad_view(self.head.bias), True,
                                      self.head.weight, self.head.bias)
        return torch.nn.functional.linear(x.float(), self.head.weight, self.head.bias)     # odd class counts: see models_vit_st

    def forward(self, x, hidden_states=False):
        x = self.forward_features(x, hidden_states=hidden_states)
        if hidden_states:
            return x
        return self._head(x)

    def lock(self, unlocked_groups=0, freeze_bn_stats=False):
        """retinal-COEM/src/open_clip/models_vit_flash_attn.py:202-232: freeze everything, then unfreeze the last ``unlocked_groups``
        of [embeddings (patch_embed, cls_token, pos_embed), block 0, ..., block n-2, (block n-1, fc_norm / norm), head].  There are no
        batch-norm statistics to freeze."""
        groups = [[self.patch_embed, self.cls_token, self.pos_embed], *self.blocks[:-1],
                  [self.blocks[-1], self.fc_norm if hasattr(self, "fc_norm") else self.norm], self.head]
        video_vit.lock_groups(self, groups, unlocked_groups)

    def load_state_dict_to_backbone(self, state_dict, strict=False, filter_keys=()):
        """Load a timm-layout (RETFound: ``attn.qkv``, ``norm.*``) or flash-layout checkpoint; missing / unexpected block keys are
        reported under the names the reference's flash model gives them (``mixer.Wqkv`` / ``mixer.out_proj``)."""
        sd = to_timm_layout(state_dict)
        sd = {k: v for k, v in sd.items() if not any(f in k for f in filter_keys)}
        res = nn.Module.load_state_dict(self, sd, strict=strict)
        if not self.use_flash_attn:
            return res
        return torch.nn.modules.module._IncompatibleKeys([_flash_name(k) for k in res.missing_keys],
                                                         [_flash_name(k) for k in res.unexpected_keys])


def flash_attn_vit_large_patch16(**kwargs):
    return VisionTransformer(patch_size=16, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4, qkv_bias=True,
                             norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)
