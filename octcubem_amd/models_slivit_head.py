"""The SLIViT slice head: drop-in for the reference's ``OCTCube/models_slivit_head.py`` ``SLIViT`` (:15-43), vit-pytorch's ``ViT`` with one
"patch" per slice, as ``models_vit_st_flash_attn_slivit.VisionTransformer`` puts it on top of the spatio-temporal trunk.

Same name, keyword signature and state-dict keys (``to_patch_embedding.{1,2,3}.*``, ``pos_embedding``, ``cls_token``, ``transformer.*``,
``mlp_head.*``).  Everything behind the patch projection is ``model_slivit_baseline.SLIViT.forward_embedded`` -- the restated ViT this
package already ships.  In front of it the reference rearranges its input ``[N, T, patch_height, patch_width]`` into rows of
``patch_height * patch_width`` and runs LayerNorm -> Linear over them.  Two ways in:

* ``forward_stream(x, n_prefix)``: the trunk's token stream fp32 ``[N, n_prefix + T * L, C]`` as it lies in memory (``patch_height = C``,
  ``patch_width = L``).  ``ops.SliceEmbedFn``: the HIP slab LayerNorm writes the GEMM's 16-bit operand in the reference's element order
  straight from the stream; no transposed fp32 copy exists, forward or backward.
* ``forward(x)`` / ``forward_head(x)``: any fp32 ``[N, T, patch_height, patch_width]`` tensor or view, the reference's own call.  The ATen
  composition (a materialised reshape, ``F.layer_norm``, the same GEMMs), as the baseline model runs it.

Dropout other than 0 is refused, as in the baseline.  GPU only."""
from __future__ import annotations

import torch

from . import ops
from .arena import get_arena
from . import model_slivit_baseline as _base
from ._autocast import autocast_invariant


@autocast_invariant
class SLIViT(_base.SLIViT):
    def __init__(self, *, num_of_patches=20, vit_dim=256, vit_depth=5, heads=20, mlp_dim=512, dropout=0., emb_dropout=0., patch_height=1024,
                 patch_width=256, rnd_pos_emb=False, num_classes=1, dim_head=64):
        if patch_height % 8:
            raise ValueError(f"SLIViT head: patch_height = {patch_height} (the trunk's width) is not a multiple of 8")
        super().__init__(feature_extractor=None, vit_dim=vit_dim, vit_depth=vit_depth, heads=heads, mlp_dim=mlp_dim,
                         num_of_patches=num_of_patches, dropout=dropout, emb_dropout=emb_dropout, patch_height=patch_height,
                         patch_width=patch_width, rnd_pos_emb=rnd_pos_emb, num_classes=num_classes, dim_head=dim_head)

    def forward_stream(self, x: torch.Tensor, n_prefix: int = 1) -> torch.Tensor:
        """fp32 token stream [N, n_prefix + num_patches * patch_width, patch_height] -> logits [N, num_classes].  The caller has prepared
        the arena (the model that owns this head)."""
        a = get_arena(self)
        ln1, proj = self.to_patch_embedding[1], self.to_patch_embedding[2]
        y = ops.SliceEmbedFn.apply(x, ln1.weight, ln1.bias, ln1.eps, self.num_patches, self.patch_width, int(n_prefix),
                                   a.lp_view(proj.weight), a.f32_view(proj.bias), lambda: a.grad_view(proj.weight),
                                   lambda: a.grad_view(proj.bias), proj.weight, proj.bias)
        return self.forward_embedded(y)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """The reference's call: fp32 [N, num_patches, patch_height, patch_width] (a view will do) -> logits."""
        self.prepare()
        assert x.dim() == 4 and tuple(x.shape[1:]) == (self.num_patches, self.patch_height, self.patch_width), \
            f"SLIViT head: expected [N, {self.num_patches}, {self.patch_height}, {self.patch_width}], got {tuple(x.shape)}"
        return self.forward_head(x.float())
