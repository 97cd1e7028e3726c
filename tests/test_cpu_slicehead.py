"""CPU: construction-side contract of the RETFound-all model (octcubem_amd.models_vit_3dhead) and the 2-D flash ViT
(octcubem_amd.models_vit_flash_attn) against what the reference's OCTCube/models_vit_3dhead.py reported in
tests/golden/slicehead_small.npz: state_dict keys, the missing keys of a RETFound checkpoint, layer-decay groups, ``lock``,
the module-name lookups of the reference's drivers, and the 224 -> 256 positional-table interpolation.  No GPU needed."""
import json
import os
from functools import partial

import numpy as np
import pytest
import torch

from octcubem_amd import checkpoint, lr_decay, models_vit_3dhead, models_vit_3dhead_flash_attn, models_vit_flash_attn, pos_embed
from oracle import vit_ref as V
from tests import slicehead_ref as R


def small(factory_flash=True, gp=True, **kw):
    cls = models_vit_3dhead.VisionTransformerWith3DPoolingHead
    return cls(img_size=64, patch_size=16, in_chans=3, num_classes=3, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True,
               norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), global_pool=gp, use_flash_attn=factory_flash, **kw)


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "slicehead_small.npz"))


@pytest.mark.parametrize("gp", [True, False])
@pytest.mark.parametrize("flash", [True, False])
def test_state_dict_keys_match_reference(z, gp, flash):
    ref = json.loads(str(z[f"gp{int(gp)}/keys"]))
    m = small(flash, gp)
    assert sorted(m.state_dict()) == sorted(ref)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == R.param_shapes(R.config(gp))


def test_factories_give_the_reference_key_list():
    cfg = V.ViT2DConfig(img_size=224, num_classes=5, embed_dim=1024, depth=24, num_heads=16, global_pool=True)
    want = set(R.param_shapes(cfg))
    for fac in (models_vit_3dhead.flash_attn_vit_large_patch16_3DSliceHead, models_vit_3dhead.vit_large_patch16_3DSliceHead):
        m = fac(img_size=224, num_classes=5, drop_path_rate=0.2, global_pool=True)
        assert set(m.state_dict()) == want
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == R.param_shapes(cfg)
    assert models_vit_3dhead.flash_attn_vit_large_patch16_3DSliceHead(img_size=224, num_classes=5).flash_compat
    assert not models_vit_3dhead.vit_large_patch16_3DSliceHead(img_size=224, num_classes=5).flash_compat


def test_reference_module_lookups_resolve():
    fac = models_vit_3dhead_flash_attn.__dict__["flash_attn_vit_large_patch16_3DSliceHead"]
    assert fac is models_vit_3dhead.flash_attn_vit_large_patch16_3DSliceHead
    assert callable(models_vit_flash_attn.__dict__["flash_attn_vit_large_patch16"])


@pytest.mark.parametrize("gp", [True, False])
def test_retfound_checkpoint_missing_keys(z, gp):
    """The reference's drivers assert this set after loading RETFound weights (main_finetune_downstream_*.py:516-518)."""
    want_missing = set(json.loads(str(z[f"gp{int(gp)}/ckpt_missing"])))
    want_unexpected = set(json.loads(str(z[f"gp{int(gp)}/ckpt_unexpected"])))
    ck = {k: torch.zeros(s) for k, s in V.vit2d_param_shapes(R.config(False)).items() if not k.startswith("head.")}
    for flash in (True, False):
        msg = small(flash, gp).load_state_dict_to_backbone(dict(ck))
        assert set(msg.missing_keys) == want_missing and set(msg.unexpected_keys) == want_unexpected
    if gp:
        assert want_missing == {"fc_aggregate_cls.weight", "fc_aggregate_cls.bias", "aggregate_cls_norm.weight", "aggregate_cls_norm.bias",
                                "head.weight", "head.bias", "fc_norm.weight", "fc_norm.bias"}


def test_backbone_loader_takes_flash_layout_and_reports_flash_names():
    P = R.init(R.config(True))
    m = small(True, True)
    flash = models_vit_flash_attn.to_timm_layout(P)
    assert flash.keys() == P.keys()
    fl = checkpoint.to_flash_layout(checkpoint.to_native_layout(P))
    assert any(".mixer.Wqkv." in k for k in fl)
    msg = m.load_state_dict_to_backbone(fl, strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    for k, v in m.state_dict().items():
        assert torch.equal(v, P[k]), k
    fl.pop("blocks.1.mixer.Wqkv.bias")
    msg = m.load_state_dict_to_backbone(fl)
    assert msg.missing_keys == ["blocks.1.mixer.Wqkv.bias"]
    msg = m.load_state_dict_to_backbone(P, filter_keys=("pos_embed", "patch_embed"))
    assert set(msg.missing_keys) == {"pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias"}


def test_layer_decay_puts_aggregation_head_in_top_group():
    m = small(True, True)
    groups = lr_decay.param_groups_lrd(m, 0.05, no_weight_decay_list=m.no_weight_decay(), layer_decay=0.65)
    name = {id(p): n for n, p in m.named_parameters()}
    scale = {name[id(p)]: g["lr_scale"] for g in groups for p in g["params"]}
    wd = {name[id(p)]: g["weight_decay"] for g in groups for p in g["params"]}
    for n in ("fc_aggregate_cls.weight", "fc_aggregate_cls.bias", "aggregate_cls_norm.weight", "aggregate_cls_norm.bias",
              "head.weight", "fc_norm.weight"):
        assert scale[n] == 1.0, n
        assert lr_decay.get_layer_id_for_vit(n, len(m.blocks) + 1) == len(m.blocks) + 1
    assert scale["blocks.1.mlp.fc1.weight"] == 0.65 and scale["blocks.0.norm1.weight"] == 0.65 ** 2 and scale["pos_embed"] == 0.65 ** 3
    assert wd["fc_aggregate_cls.weight"] == 0.05 and wd["fc_aggregate_cls.bias"] == 0.0 and wd["pos_embed"] == 0.0
    assert m.no_weight_decay() == {"pos_embed", "cls_token"}


@pytest.mark.parametrize("gp", [True, False])
def test_lock_unfreezes_the_reference_groups(gp):
    m = small(True, gp)
    nm = "fc_norm" if gp else "norm"
    top = {"fc_aggregate_cls.weight", "fc_aggregate_cls.bias", "aggregate_cls_norm.weight", "aggregate_cls_norm.bias", "head.weight",
           "head.bias"}
    last = {n for n, _ in m.named_parameters() if n.startswith("blocks.1.") or n.startswith(nm + ".")}
    first = {n for n, _ in m.named_parameters() if n.startswith("blocks.0.")}
    embed = {"cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias"}
    allp = {n for n, _ in m.named_parameters()}
    assert allp == top | last | first | embed
    for n_groups, want in ((0, set()), (1, top), (2, top | last), (3, top | last | first), (4, allp)):
        m.lock(n_groups)
        assert {n for n, p in m.named_parameters() if p.requires_grad} == want, n_groups


def test_center2d_flash_model_contract():
    m = models_vit_flash_attn.flash_attn_vit_large_patch16(img_size=224, num_classes=4, drop_path_rate=0.1, global_pool=True,
                                                           dropout=0.3, drop_rate=0.0)
    assert m.flash_compat and isinstance(m.dropout, torch.nn.Dropout) and not m.fused_pool
    cfg = V.ViT2DConfig(img_size=224, num_classes=4, embed_dim=1024, depth=24, num_heads=16, global_pool=True)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == dict(V.vit2d_param_shapes(cfg))
    with pytest.raises(NotImplementedError):
        models_vit_flash_attn.flash_attn_vit_large_patch16(img_size=224, num_classes=4, cls_embed=False)
    msg = m.load_state_dict_to_backbone({k: torch.zeros(s) for k, s in V.vit2d_param_shapes(
        V.ViT2DConfig(img_size=224, embed_dim=1024, depth=24, num_heads=16, global_pool=False)).items() if not k.startswith("head.")})
    assert set(msg.missing_keys) == {"head.weight", "head.bias", "fc_norm.weight", "fc_norm.bias"}   # main_finetune_downstream_*.py:525


def test_pos_embed_interpolation_224_to_256():
    """finetune_ct3d.sh runs the RETFound-all model at 256 from 224-trained weights: 14 x 14 -> 16 x 16, cls entry kept."""
    m = models_vit_3dhead.flash_attn_vit_large_patch16_3DSliceHead(img_size=256, num_classes=3, global_pool=True)
    src = V.ViT2DConfig(img_size=224, embed_dim=1024, depth=24, num_heads=16, global_pool=False)
    ck = V.init_from_shapes({k: s for k, s in V.vit2d_param_shapes(src).items() if not k.startswith("head.")}, seed=3)
    pe224 = ck["pos_embed"].clone()
    pos_embed.interpolate_pos_embed(m, ck)
    assert tuple(ck["pos_embed"].shape) == (1, 257, 1024) == tuple(m.pos_embed.shape)
    assert torch.equal(ck["pos_embed"][:, :1], pe224[:, :1])
    grid = pe224[:, 1:].reshape(1, 14, 14, 1024).permute(0, 3, 1, 2)
    want = torch.nn.functional.interpolate(grid, size=(16, 16), mode="bicubic", align_corners=False).permute(0, 2, 3, 1).flatten(1, 2)
    assert torch.allclose(ck["pos_embed"][:, 1:], want)
    msg = m.load_state_dict_to_backbone(ck)
    assert set(msg.missing_keys) == {"fc_aggregate_cls.weight", "fc_aggregate_cls.bias", "aggregate_cls_norm.weight",
                                     "aggregate_cls_norm.bias", "head.weight", "head.bias", "fc_norm.weight", "fc_norm.bias"}
    assert torch.equal(m.pos_embed.detach(), ck["pos_embed"])
