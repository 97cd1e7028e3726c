#!/usr/bin/env python
"""Writes tests/golden/stslivit_small.npz: OCTCube with the SLIViT slice head at tests/stslivit_ref.SMALL in fp32 on the CPU, from the
reference's OWN model class.

What runs from the reference's source files (its OCTCube directory, given with --reference): ``models_vit_st_flash_attn_slivit.
VisionTransformer`` (non-flash blocks: util/video_vit.PatchEmbed / Block / Attention), its slicing and ``transpose(2, 3)`` of the token
stream, and ``models_slivit_head.SLIViT`` with its einops ``Rearrange`` (einops is installed and runs for real).  vit-pytorch is not
installed: ``vit_pytorch.vit.ViT`` is a stand-in with vit-pytorch 1.x's module tree (so the reference's state-dict keys are the real
ones) whose forward applies ``to_patch_embedding[0]`` -- the reference's Rearrange -- and then tests/slivit_ref.head_forward, the
restated head the SLIViT baseline's golden already rests on.  timm, flash_attn and the rest: oracle.gen_golden.install_shims().

Stored, all fp32: the embedding the reference returns, the logits, the MSE loss against the seeded target, the gradient norm of every
parameter (0 for ``norm.*``, which has none), sub-sampled gradients of SAMPLE_KEYS, the state-dict key list -- and
``rounding_err/<dtype>/...``: the relative error of tests/stslivit_ref's ROUNDING-MODEL run (operands rounded to bfloat16 / float16
where the library rounds) against its fp32 run, per stored quantity, as tests/golden/slivit_small.npz stores them.
tests/test_gpu_stslivit.py takes its tolerances from these: the reference's own error under operand rounding, never the library's.

    python tools/gen_golden_stslivit.py --reference <reference>/OCTCube      (tests/test_cpu_stslivit.py checks the file without it)
"""
import argparse
import os
import sys
import types
from functools import partial

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import slivit_ref as R  # noqa: E402
from tests import stslivit_ref as S  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "stslivit_small.npz")
SAMPLE_KEYS = ["patch_embed.proj.weight", "patch_embed.proj.bias", "cls_token", "pos_embed_spatial", "pos_embed_temporal", "pos_embed_class",
               "blocks.0.norm1.weight", "blocks.0.attn.q.weight", "blocks.0.attn.v.bias", "blocks.1.attn.proj.weight", "blocks.1.mlp.fc1.weight",
               "blocks.1.mlp.fc2.bias", S.HP + "to_patch_embedding.1.weight", S.HP + "to_patch_embedding.1.bias",
               S.HP + "to_patch_embedding.2.weight", S.HP + "to_patch_embedding.2.bias", S.HP + "to_patch_embedding.3.weight",
               S.HP + "pos_embedding", S.HP + "cls_token", S.HP + "transformer.layers.0.0.to_qkv.weight",
               S.HP + "transformer.layers.1.1.net.4.weight", S.HP + "transformer.norm.weight", S.HP + "mlp_head.weight"]


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def install_vit_pytorch_stand_in():
    """``vit_pytorch.vit.ViT`` with vit-pytorch 1.x's constructor and module tree; the arithmetic is tests/slivit_ref.head_forward."""
    from octcubem_amd.model_slivit_baseline import _Transformer            # the module tree only: its forwards are never called here

    class ViT(nn.Module):
        def __init__(self, *, image_size, patch_size, num_classes, dim, depth, heads, mlp_dim, pool="cls", channels=3, dim_head=64,
                     dropout=0., emb_dropout=0.):
            super().__init__()
            (ih, iw), (ph, pw) = image_size, patch_size
            assert ih % ph == 0 and iw % pw == 0 and dropout == 0 and emb_dropout == 0 and pool == "cls"
            n, patch_dim = (ih // ph) * (iw // pw), channels * ph * pw
            self.to_patch_embedding = nn.Sequential(nn.Identity(), nn.LayerNorm(patch_dim), nn.Linear(patch_dim, dim), nn.LayerNorm(dim))
            self.pos_embedding = nn.Parameter(torch.randn(1, n + 1, dim))
            self.cls_token = nn.Parameter(torch.randn(1, 1, dim))
            self.transformer = _Transformer(dim, depth, heads, dim_head, mlp_dim)
            self.mlp_head = nn.Linear(dim, num_classes)
            self._cfg = dict(num_patches=n, vit_dim=dim, heads=heads, dim_head=dim_head, vit_depth=depth, mlp_dim=mlp_dim, patch_height=ph,
                             patch_width=pw)

        def forward(self, img):
            rows = self.to_patch_embedding[0](img)                          # the reference's Rearrange
            return R.head_forward(dict(self.named_parameters()), rows, self._cfg, None)

    vp, vv = types.ModuleType("vit_pytorch"), types.ModuleType("vit_pytorch.vit")
    vv.ViT = ViT
    vp.vit = vv
    sys.modules.update({"vit_pytorch": vp, "vit_pytorch.vit": vv})


def reference_forward_backward(P, x, target, cfg, ref_dir):
    from oracle.gen_golden import install_shims
    install_shims()
    install_vit_pytorch_stand_in()
    sys.path.insert(0, ref_dir)
    os.chdir(ref_dir)
    import models_vit_st_flash_attn_slivit as ref
    m = ref.VisionTransformer(num_frames=cfg["num_frames"], t_patch_size=cfg["t_patch_size"], img_size=cfg["img_size"],
                              patch_size=cfg["patch_size"], in_chans=cfg["in_chans"], num_classes=cfg["num_classes"],
                              embed_dim=cfg["embed_dim"], depth=cfg["depth"], num_heads=cfg["num_heads"], mlp_ratio=4,
                              norm_layer=partial(nn.LayerNorm, eps=1e-6), sep_pos_embed=True, cls_embed=True, global_pool=True,
                              drop_path_rate=0.0, use_flash_attn=False, slivit_depth_num=cfg["slivit_depth_num"])
    keys = list(m.state_dict().keys())
    res = m.load_state_dict(P, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    m.eval()
    logits, emb = m(x, return_embeddings=True)
    loss = torch.nn.functional.mse_loss(logits, target)
    loss.backward()
    G = {k: p.grad for k, p in m.named_parameters()}
    return emb.detach(), logits.detach(), loss.detach(), G, keys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's OCTCube directory")
    a = ap.parse_args()
    torch.manual_seed(0)
    torch.set_num_threads(1)                 # one summation order whatever the machine
    cfg = S.SMALL
    P = S.init_params(cfg)
    x, target = S.make_inputs(cfg)
    emb, logits, loss, G, ref_keys = reference_forward_backward(P, x, target, cfg, os.path.abspath(a.reference))
    assert sorted(ref_keys) == sorted(P.keys())
    assert all(G[k] is None for k in S.NO_GRAD) and all(G[k] is not None for k in P if k not in S.NO_GRAD)
    out = {"embedding": emb.contiguous().numpy(), "logits": logits.numpy(), "loss": np.float32(loss), "keys": np.array(ref_keys),
           "sample_keys": np.array(SAMPLE_KEYS),
           "grad_norm": np.array([0.0 if G[k] is None else float(G[k].double().norm()) for k in ref_keys], dtype=np.float32)}
    for k in SAMPLE_KEYS:
        out["grad_sample/" + k] = S.subsample(G[k]).numpy()
    e0, l0, s0, G0 = S.forward_backward(P, x, target, cfg, None)
    for name, dt in (("bfloat16", torch.bfloat16), ("float16", torch.float16)):
        e1, l1, s1, G1 = S.forward_backward(P, x, target, cfg, dt)
        pre = f"rounding_err/{name}/"
        out[pre + "embedding"] = np.float32(rel(e1, e0))
        out[pre + "logits"] = np.float32(rel(l1, l0))
        out[pre + "loss"] = np.float32(abs(float(s1) - float(s0)) / abs(float(s0)))
        out[pre + "grad"] = np.array([0.0 if G0[k] is None else rel(G1[k], G0[k]) for k in ref_keys], dtype=np.float32)
        for k in SAMPLE_KEYS:
            out[pre + "sample/" + k] = np.float32(rel(S.subsample(G1[k]), S.subsample(G0[k])))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes; loss {float(loss):.6f}; restatement vs reference: embedding {rel(e0, emb):.2e} "
          f"logits {rel(l0, logits):.2e} loss {abs(float(s0) - float(loss)) / abs(float(loss)):.2e}; rounding_err logits bf16 "
          f"{float(out['rounding_err/bfloat16/logits']):.2e} f16 {float(out['rounding_err/float16/logits']):.2e}")


if __name__ == "__main__":
    main()
