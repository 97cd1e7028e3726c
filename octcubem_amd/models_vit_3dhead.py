"""RETFound-all: the slice-pooled 2-D ViT (``patient_dataset_type`` ``3D_flash_attn`` / ``3D``).  Drop-in for the reference's
``OCTCube/models_vit_3dhead_flash_attn.py`` ``VisionTransformerWith3DPoolingHead`` (:35-101, factory
``flash_attn_vit_large_patch16_3DSliceHead``) and ``OCTCube/models_vit_3dhead.py`` (the timm-semantics model, factory
``vit_large_patch16_3DSliceHead``).

Input [B, S, C, H, W]: every B-scan is its own image through the 2-D ViT ([B*S, C, H, W], models_vit_flash_attn), its patch tokens
are mean-pooled (or its cls token taken) and normalised by ``fc_norm`` (``norm``), the rows are averaged over the S slices, then
``fc_aggregate_cls`` (Linear D -> D), ``aggregate_cls_norm`` (LayerNorm) and ``head``.  The pooling, fc_norm and slice mean are one
HIP kernel chain (ops.SlicePoolFn, csrc/pool.hip) in both directions.  Parameter names are those of the reference's non-flash
model (timm layout); flash checkpoints load through ``load_state_dict_to_backbone`` or checkpoint.to_native_layout's rules."""
from __future__ import annotations

from functools import partial

import torch
import torch.nn as nn

from . import ops, video_vit
from .arena import get_arena
from .models_vit_flash_attn import VisionTransformer as VisionTransformer2DCenterHead
from .video_vit import layer_norm
from ._autocast import autocast_invariant


@autocast_invariant
class VisionTransformerWith3DPoolingHead(VisionTransformer2DCenterHead):
    def __init__(self, img_size=256, num_classes=400, embed_dim=768, depth=12, patch_size=16, in_chans=3, global_pool=False,
                 use_flash_attn=True, num_heads=12, mlp_ratio=4.0, no_qkv_bias=False, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0,
                 drop_path_rate=0.0, norm_layer=nn.LayerNorm, dropout=0.5, cls_embed=True, **kwargs):
        kwargs.pop("fused_pool", None)      # the slice pooling is always the fused kernel chain here
        super().__init__(img_size=img_size, num_classes=num_classes, embed_dim=embed_dim, depth=depth, patch_size=patch_size,
                         in_chans=in_chans, global_pool=global_pool, use_flash_attn=use_flash_attn, num_heads=num_heads,
                         mlp_ratio=mlp_ratio, no_qkv_bias=no_qkv_bias, qk_scale=qk_scale, drop_rate=drop_rate,
                         attn_drop_rate=attn_drop_rate, drop_path_rate=drop_path_rate, norm_layer=norm_layer, dropout=dropout,
                         cls_embed=cls_embed, fused_pool=True, **kwargs)
        # Fully connected layer for the aggregated CLS tokens, and the normalisation after it
        self.fc_aggregate_cls = nn.Linear(embed_dim, embed_dim)
        self.aggregate_cls_norm = norm_layer(embed_dim)

    def forward_features(self, x, hidden_states=False):
        B, S, C, H, W = x.shape
        t = self._tokens(x.reshape(B * S, C, H, W), hidden_states)
        if hidden_states:
            return t
        x = self._pool(t, S=S, fused=True)                                   # fp32 [B, D]: fc_norm per slice, mean over slices
        arena = get_arena(self)
        fc = self.fc_aggregate_cls
        x = ops.LinearFn.apply(x, arena.lp_view(fc.weight), arena.f32_view(fc.bias), lambda: arena.grad_view(fc.weight),
                               lambda: arena.grad_view(fc.bias), True, fc.weight, fc.bias)
        return layer_norm(self.aggregate_cls_norm, x.contiguous()).float()

    def lock(self, unlocked_groups=0, freeze_bn_stats=False):
        """Freeze everything, then unfreeze the last ``unlocked_groups`` of: embeddings, blocks[0 .. -2], (last block + fc_norm /
        norm), (fc_aggregate_cls + aggregate_cls_norm + head) -- models_vit_3dhead_flash_attn.py:67-101."""
        groups = [
            [self.patch_embed, self.cls_token, self.pos_embed],
            *self.blocks[:-1],
            [self.blocks[-1], self.fc_norm if hasattr(self, "fc_norm") else self.norm],
            [self.fc_aggregate_cls, self.aggregate_cls_norm, self.head],
        ]
        video_vit.lock_groups(self, groups, unlocked_groups)


def flash_attn_vit_large_patch16_3DSliceHead(**kwargs):
    """RETFound-all with flash-attn semantics (the last block hands its MLP branch alone to the pooling)."""
    return VisionTransformerWith3DPoolingHead(patch_size=16, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4, qkv_bias=True,
                                              norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)


def vit_large_patch16_3DSliceHead(**kwargs):
    """RETFound-all with timm semantics (OCTCube/models_vit_3dhead.py: standard residual, global pool by default)."""
    kwargs.setdefault("global_pool", True)
    kwargs.setdefault("use_flash_attn", False)
    return VisionTransformerWith3DPoolingHead(patch_size=16, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4, qkv_bias=True,
                                              norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)
