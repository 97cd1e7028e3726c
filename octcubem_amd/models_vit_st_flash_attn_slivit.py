"""OCTCube with the SLIViT slice head (``--patient_dataset_type 3D_st_flash_attn_slivit``): drop-in for the reference's
``OCTCube/models_vit_st_flash_attn_slivit.py`` ``VisionTransformer`` (constructor :53-166, forward :179-261) -- the spatio-temporal trunk
of ``models_vit_st`` whose final token stream is handed, slice by slice, to ``models_slivit_head.SLIViT``; the reference's regression and
cross-modality runs select it (main_finetune_downstream_inhouse_singlefold_diffmodal.py:1083-1094).

State dict: the trunk's keys, ``norm.*`` (the reference builds it and never applies it: present, no gradient) and ``SLIViT_head.*``; no
``head.*``.  The head's fixed sizes are the reference's (:92-94): width 256, 20 heads of 64, MLP 512, ``slivit_depth_num`` layers, one
"patch" per temporal slice of ``embed_dim x (h w)`` values.

Forward: trunk -> ``ops.SliceEmbedFn`` on the final stream (``n_prefix = 1``: the cls token takes no part) -> the head's 256-wide
LayerNorm -> cls / pos -> transformer -> ``mlp_head``.  With ``use_flash_attn=True`` the last block hands on its MLP branch alone, as the
reference's ``x, residual`` loop does (:228-232); with ``False`` the standard residual.  ``return_embeddings`` returns the ``[N, T, C, L]``
strided view of the stream the reference returns (:246-254); no copy is made.

The ATen composition of the same embedding (a materialised fp32 transpose, ``F.layer_norm``, a cast, the same GEMMs) is what
``model.SLIViT_head.forward_head(embedding)`` computes; it is slower at every size measured (tools/bench_slice_embed.py), so the model
has no switch for it.

Everything else is the base class's: ``set_grad_checkpointing``, ``prepare``, ``invalidate_lp``, ``load_state_dict_to_backbone``, autocast
invariance.  GPU only."""
from __future__ import annotations

from functools import partial

import torch.nn as nn

from . import models_vit_st, video_vit
from ._autocast import autocast_invariant
from .models_slivit_head import SLIViT


@autocast_invariant
class VisionTransformer(models_vit_st.VisionTransformer):
    """Vision Transformer with the SLIViT head over its temporal slices"""

    def __init__(self, num_frames, t_patch_size, img_size=256, patch_size=16, in_chans=1, num_classes=400, embed_dim=768, depth=12,
                 num_heads=12, mlp_ratio=4.0, no_qkv_bias=False, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0,
                 drop_path_rate=0.0, norm_layer=nn.LayerNorm, dropout=0.5, sep_pos_embed=False, cls_embed=False,
                 global_pool=False, use_flash_attn=False, slivit_depth_num=5, **kwargs):
        super().__init__(num_frames, t_patch_size, img_size=img_size, patch_size=patch_size, in_chans=in_chans, num_classes=num_classes,
                         embed_dim=embed_dim, depth=depth, num_heads=num_heads, mlp_ratio=mlp_ratio, no_qkv_bias=no_qkv_bias,
                         qk_scale=qk_scale, drop_rate=drop_rate, attn_drop_rate=attn_drop_rate, drop_path_rate=drop_path_rate,
                         norm_layer=norm_layer, dropout=dropout, sep_pos_embed=sep_pos_embed, cls_embed=cls_embed,
                         global_pool=global_pool, use_flash_attn=use_flash_attn, **kwargs)
        del self.head, self.dropout            # the reference has neither (:166 is its last module)
        T, h, w = self.input_size
        self.SLIViT_head = SLIViT(num_of_patches=T, vit_dim=256, vit_depth=slivit_depth_num, heads=20, mlp_dim=512, dropout=0.,
                                  emb_dropout=0., patch_height=embed_dim, patch_width=h * w, rnd_pos_emb=False,
                                  num_classes=num_classes, dim_head=64)

    def forward(self, x, hidden_states=False, return_embeddings=False):
        if not hidden_states and not self.global_pool:
            raise ValueError("Class token can not be implemented for Slivit head")
        hs = super().forward(x, hidden_states=True)            # prepares the arena; every block's output
        if hidden_states:
            return hs
        x = hs[-1]                                              # fp32 [N, 1 + T L, C]
        N, _, C = x.shape
        T, h, w = self.input_size
        embedding = x[:, 1:, :].view(N, T, h * w, C).transpose(2, 3)       # [N, T, C, L]: a view of the stream
        out = self.SLIViT_head.forward_stream(x, 1)
        if return_embeddings:
            return out, embedding
        return out

    def lock(self, unlocked_groups=0, freeze_bn_stats=False):
        """As the base class's, with ``SLIViT_head`` as the head group."""
        first_group = [self.patch_embed, self.pos_embed_spatial, self.pos_embed_temporal, self.pos_embed_class, self.cls_token]
        video_vit.lock_groups(self, [first_group, *self.blocks[:-1], [self.blocks[-1], self.norm], [self.SLIViT_head]], unlocked_groups)


def vit_base_patch16(**kwargs):
    return VisionTransformer(patch_size=16, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4,
                             norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)


def vit_large_patch16(**kwargs):
    return VisionTransformer(patch_size=16, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4,
                             norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)


def flash_attn_vit_large_patch16(**kwargs):
    kwargs.setdefault("use_flash_attn", True)
    return vit_large_patch16(**kwargs)


def vit_huge_patch14(**kwargs):
    """The reference's huge model is cut into 16-pixel patches despite its name (:339-348)."""
    return VisionTransformer(patch_size=16, embed_dim=1280, depth=32, num_heads=16, mlp_ratio=4,
                             norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)
