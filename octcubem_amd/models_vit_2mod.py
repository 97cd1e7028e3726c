"""Two-modality en-face tower of the three-modality COEM configs (``text_cfg.vit_model_name = "ViT_flash_attn_2mod"``): drop-in for the
reference's ``retinal-COEM/src/open_clip/models_vit_flash_attn_2mod.py`` ``VisionTransformer`` (constructor :53-128, ``forward``
:171-185, ``lock`` :221-251).  ONE trunk shared by the IR and the FAF image, ending in ``head -> GELU -> mod_head_{0,1}``:

  * the trunk, arena, ``prepare()`` / ``invalidate_lp()``, ``forward_features`` and ``load_state_dict_to_backbone`` are
    models_vit_flash_attn's (timm key layout for the blocks); the keys this class adds are the reference's: ``head.{weight,bias}``
    is ``embed_dim -> embed_dim`` and ``mod_head_{i}.{weight,bias}`` is ``embed_dim -> out_dim``;
  * ``forward(x, modality=k)`` runs ``mod_head_k(GELU(head(features)))`` as ops.MlpFn (GELU in the fc1 GEMM's epilogue) with ``head``
    as fc1 and ``mod_head_k`` as fc2.  The reference's ``assert torch.abs(...).sum() == 0`` self-checks are not reproduced: each one
    is a device synchronisation.  ``self.dropout`` is built and, as in the reference, never applied;
  * ``forward_pair(x0, x1)`` is both modalities in one trunk pass at 2 B rows (the reference runs the trunk twice at B): the COEM
    fine-tune runs at a handful of samples per GPU, where the GEMMs leave CUs idle, and one backward at 2 B accumulates the shared
    trunk's gradient once.
``out_dim`` must be a multiple of 8 (the rows of a GEMM operand); the reference's configs use 512."""
from __future__ import annotations

import operator
from functools import partial

import torch
import torch.nn as nn

from . import models_vit_flash_attn, ops, video_vit
from .arena import get_arena
from ._autocast import autocast_invariant


@autocast_invariant
class VisionTransformer(models_vit_flash_attn.VisionTransformer):
    """Vision Transformer with one ``head`` and ``num_mod_head`` modality heads behind a shared trunk"""

    def __init__(self, image_size=256, out_dim=400, embed_dim=1024, depth=24, patch_size=16, in_chans=3, global_pool=True,
                 use_flash_attn=True, num_heads=16, mlp_ratio=4.0, no_qkv_bias=False, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0,
                 drop_path_rate=0.0, norm_layer=nn.LayerNorm, dropout=0.5, cls_embed=True, num_mod_head=2, flash_compat=None, **kwargs):
        if out_dim % 8 != 0:
            raise ValueError(f"out_dim = {out_dim}: the modality heads are GEMM operands, whose rows come in multiples of 8")
        if num_mod_head < 1:
            raise ValueError(f"num_mod_head = {num_mod_head}")
        kwargs.pop("num_mod_heads", None)       # the reference's factory passes this name, which its constructor swallows in **kwargs
        for k in ("layer_decay", "weight_decay"):
            kwargs.pop(k, None)
        super().__init__(img_size=image_size, num_classes=embed_dim, embed_dim=embed_dim, depth=depth, patch_size=patch_size,
                         in_chans=in_chans, global_pool=global_pool, use_flash_attn=use_flash_attn, num_heads=num_heads,
                         mlp_ratio=mlp_ratio, no_qkv_bias=no_qkv_bias, qk_scale=qk_scale, drop_rate=drop_rate,
                         attn_drop_rate=attn_drop_rate, drop_path_rate=drop_path_rate, norm_layer=norm_layer, dropout=dropout,
                         cls_embed=cls_embed, flash_compat=flash_compat, **kwargs)
        self.image_size = image_size
        self.out_dim = out_dim
        self.num_mod_head = num_mod_head
        for i in range(num_mod_head):           # nn.Linear's own initialisation, as in the reference (created after the base's init pass)
            setattr(self, f"mod_head_{i}", nn.Linear(embed_dim, out_dim))

    def _check_modality(self, modality):
        try:
            k = -1 if isinstance(modality, bool) else operator.index(modality)      # Python and numpy integers alike
        except TypeError:
            k = -1
        if k not in range(self.num_mod_head):
            raise ValueError(f"modality should be in [0, {self.num_mod_head}), got {modality!r}")
        return k

    def _grads(self, arena, heads):
        ps = [self.head.weight, self.head.bias] + [p for h in heads for p in (h.weight, h.bias)]
        return (lambda: tuple(arena.grad_view(p) for p in ps)), ps

    def forward(self, x, hidden_states=False, modality=0):
        modality = self._check_modality(modality)
        x = self.forward_features(x, hidden_states=hidden_states)
        if hidden_states:
            return x
        arena = get_arena(self)
        mh = getattr(self, f"mod_head_{modality}")
        grads, ps = self._grads(arena, (mh,))
        return ops.MlpFn.apply(x, None, arena.lp_view(self.head.weight), arena.f32_view(self.head.bias), arena.lp_view(mh.weight),
                               arena.f32_view(mh.bias), grads, *ps).float()

    def forward_pair(self, x0, x1):
        """(mod_head_0(GELU(head(features(x0)))), mod_head_1(GELU(head(features(x1))))) from ONE trunk pass over cat(x0, x1)."""
        if self.num_mod_head < 2:
            raise ValueError("forward_pair needs two modality heads")
        if x0.shape != x1.shape:
            raise ValueError(f"forward_pair: two batches of one shape, got {tuple(x0.shape)} and {tuple(x1.shape)}")
        f = self.forward_features(torch.cat((x0, x1), dim=0))
        arena = get_arena(self)
        h0, h1 = self.mod_head_0, self.mod_head_1
        grads, ps = self._grads(arena, (h0, h1))
        y0, y1 = ops.MlpPairFn.apply(f, arena.lp_view(self.head.weight), arena.f32_view(self.head.bias), arena.lp_view(h0.weight),
                                     arena.f32_view(h0.bias), arena.lp_view(h1.weight), arena.f32_view(h1.bias), grads, *ps)
        return y0.float(), y1.float()

    def lock(self, unlocked_groups=0, freeze_bn_stats=False):
        """models_vit_flash_attn_2mod.py:221-251: freeze everything, then unfreeze the last ``unlocked_groups`` of [embedding, block 0,
        ..., block n-2, (block n-1, final norm), head]; the modality heads stay frozen, as in the reference."""
        groups = [[self.patch_embed, self.cls_token, self.pos_embed], *self.blocks[:-1],
                  [self.blocks[-1], self.fc_norm if hasattr(self, "fc_norm") else self.norm], self.head]
        video_vit.lock_groups(self, groups, unlocked_groups)


def flash_attn_vit_large_patch16(**kwargs):
    return VisionTransformer(patch_size=16, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4, qkv_bias=True,
                             norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)
