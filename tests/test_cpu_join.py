"""CPU tests of the join in front of the COEM classification head and of the three-modality model family: the f32 restatement of
csrc/join.hip inside the derived bounds of tests/join_ref.py and five planted faults outside them, the ABI of the new entry points, the
regression loss and per-column metrics of coem_finetune against by-hand numpy, the state-dict keys of the new classes and the class
``create_model_from_config`` picks."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import join_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("octmae_join_ws_floats", "octmae_join_fwd", "octmae_join_bwd")
ALL_KEYS = R.FWD_KEYS + R.BWD_KEYS
# (B, D, M, present_mask): one float4 per row; a ragged last lane group; the shipped size with every and with one modality; the largest row
CASES = ((5, 4, 2, 3), (7, 68, 3, 5), (65, 512, 3, 7), (9, 512, 3, 2), (6, 1364, 3, 7), (5, 1024, 2, 1))


@pytest.mark.parametrize("lp_is_f16", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_f32_restatement_is_inside_the_bounds(case, lp_is_f16):
    B, D, M, mask = case
    feats, gamma, beta, dy, extra = R.make_problem(B, D, M, seed=21)
    for ex in (extra, None):
        ref, bound = R.reference(feats, mask, gamma, beta, dy, ex, lp_is_f16=lp_is_f16)
        got = R.emulate(feats, mask, gamma, beta, dy, ex, lp_is_f16=lp_is_f16)
        for key in ALL_KEYS:
            w = R.worst(got[key], ref[key], bound[key])
            print(case, "f16" if lp_is_f16 else "bf16", key, "worst |err| / bound =", w)
            assert w <= 1.0, (key, w)


def test_reference_equals_autograd():
    """the float64 reference against torch's own normalize / cat / layer_norm and their autograd, the clamped rows included"""
    B, D, M, mask = 6, 12, 3, 5
    feats, gamma, beta, dy, extra = R.make_problem(B, D, M, seed=4)
    ref, _ = R.reference(feats, mask, gamma, beta, dy, extra)
    fs = [torch.from_numpy(f).double().requires_grad_(True) for f in feats]
    g, b = torch.from_numpy(gamma).double().requires_grad_(True), torch.from_numpy(beta).double().requires_grad_(True)
    ns = [torch.nn.functional.normalize(f, dim=-1) if (mask >> k) & 1 else torch.zeros_like(f) for k, f in enumerate(fs)]
    y = torch.nn.functional.layer_norm(torch.cat(ns, dim=-1), (M * D,), g, b, float(np.float32(R.LN_EPS)))
    loss = (y * torch.from_numpy(dy).double()).sum() + sum((n * torch.from_numpy(extra[k]).double()).sum() for k, n in enumerate(ns)
                                                           if (mask >> k) & 1)
    loss.backward()
    assert float((y.detach() - torch.from_numpy(ref["y"])).abs().max()) <= 1e-12
    for k in range(M):
        if (mask >> k) & 1:
            assert float((ns[k].detach() - torch.from_numpy(ref["n"][k])).abs().max()) <= 1e-13
            want = torch.from_numpy(ref["df"][k])
            assert float((fs[k].grad - want).abs().max()) <= 1e-11 * float(want.abs().max()), k
        else:
            assert np.isnan(ref["df"][k]).all() and (ref["n"][k] == 0).all()
    assert float((g.grad - torch.from_numpy(ref["dgamma"])).abs().max()) <= 1e-11
    assert float((b.grad - torch.from_numpy(ref["dbeta"])).abs().max()) <= 1e-11
    assert abs(ref["rstd"][1] - float(np.float32(R.LN_EPS)) ** -0.5) <= 1e-9            # the all-zero row: variance 0


@pytest.mark.parametrize("fault,mask,keys", [("slot", 7, ("n", "y", "df")), ("stale_inv", 7, ("df",)), ("stats_D", 7, ("mean", "rstd", "y", "df")),
                                             ("dgamma_row", 7, ("dgamma", "dbeta")), ("mask", 5, ("n", "y"))])
def test_planted_faults_leave_the_bounds(fault, mask, keys):
    feats, gamma, beta, dy, extra = R.make_problem(9, 512, 3, seed=22)
    ref, bound = R.reference(feats, mask, gamma, beta, dy, extra)
    got = R.emulate(feats, mask, gamma, beta, dy, extra, fault=fault)
    over = {key: R.worst(got[key], ref[key], bound[key]) for key in ALL_KEYS}
    print(fault, over)
    for key in keys:
        assert over[key] > 1.0, (fault, key, over[key])
    if fault in ("stale_inv", "dgamma_row"):       # a backward fault leaves the forward alone
        assert all(over[key] <= 1.0 for key in R.FWD_KEYS)


def test_abi_declares_the_join_entry_points():
    from octcubem_amd import _lib
    header = open(os.path.join(ROOT, "include", "octmae.h")).read()
    assert _lib.expected_abi_version() >= 25
    assert re.search(r"^ \* 25: octmae_join_fwd", header, re.M)
    for sym in SYMBOLS:
        assert re.search(rf"^int {sym}\(", header, re.M), sym
        assert sym in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["octmae_join_fwd"]) == 16 and len(_lib.SIGNATURES["octmae_join_bwd"]) == 18
    mk = open(os.path.join(ROOT, "octcubem_amd", "csrc", "Makefile")).read()
    assert "join.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1)
    for lib in ("liboctmae.so", "liboctmae_f16.so"):
        path = os.path.join(ROOT, "octcubem_amd", lib)
        if os.path.exists(path):
            names = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
            for sym in SYMBOLS:
                assert re.search(rf"\bT {sym}$", names, re.M), (lib, sym)


def test_join_refuses_bad_shapes_on_the_host():
    """ops._join_check restates the kernel's refusals: ValueError before any tensor is made (CPU tensors reach the device check only
    after the shape checks that need no tensor)"""
    from octcubem_amd import ops
    f = [torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(2, 8)]
    for feats, mask in ((f[:1], 1), (f + f[:1], 15), (f, 0), (f, 8), (f[:2], 4), (f, True), ([None, None, None], 1)):
        with pytest.raises(ValueError):
            ops._join_check("join", feats, mask)


# --------------------------------------------------------------------------------------------------- loss and metrics
def test_regression_loss_and_metrics_equal_numpy():
    from octcubem_amd import coem_finetune as FT
    g = np.random.default_rng(5)
    N, C = 11, 4
    labels = g.standard_normal((N, C))
    logits = labels + 0.3 * g.standard_normal((N, C))
    logits[:, 1] = 2.5 * labels[:, 1] - 0.75            # perfectly correlated
    logits[:, 2] = 0.125                                # constant predictions
    lt, yt = torch.from_numpy(logits).float(), torch.from_numpy(labels).float()
    lo, la = lt.double().numpy(), yt.double().numpy()
    w = np.array([0.1, 1, 1, 1])
    want = float((w * (((lo - la) ** 2).mean(0) + np.abs(lo - la).mean(0))).sum() / (2 * w.sum()))
    assert abs(float(FT.regression_loss(lt, yt)) - want) <= 1e-6 * want
    with pytest.raises(ValueError):
        FT.regression_loss(lt, yt[:, :3])
    m = FT.column_metrics(lt, yt)
    for j in range(C):
        d = la[:, j] - lo[:, j]
        assert abs(m[f"mse_{j}"] - np.mean(d * d)) <= 1e-12 and abs(m[f"mae_{j}"] - np.mean(np.abs(d))) <= 1e-12
        if j == 2:
            assert all(math.isnan(m[f"{k}_{j}"]) for k in ("pearsonr", "r2", "PearsonR", "R2"))
            continue
        xc, yc = lo[:, j] - lo[:, j].mean(), la[:, j] - la[:, j].mean()
        r = float((xc * yc).sum() / math.sqrt((xc * xc).sum() * (yc * yc).sum()))
        for k in ("pearsonr", "PearsonR"):
            assert abs(m[f"{k}_{j}"] - r) <= 1e-12
        for k in ("r2", "R2"):
            assert abs(m[f"{k}_{j}"] - r * r) <= 1e-12
        assert abs(FT.compute_r2(la[:, j], lo[:, j]) - r * r) <= 1e-12
    assert abs(m["pearsonr_1"] - 1.0) <= 1e-6 and m["mse_1"] > 0.1       # r = 1 says nothing about the error
    assert set(m) == {f"{k}_{j}" for k in FT.METRIC_KEYS for j in range(C)}


def test_other_multimodal_types_point_to_the_contrastive_loop():
    import types
    from octcubem_amd import coem_finetune as FT
    args = types.SimpleNamespace(device="cpu", multimodal_type="oct_faf_ir", precision="amp")
    with pytest.raises(NotImplementedError, match="coem.train_one_epoch"):
        FT.train_one_epoch(None, {}, 0, [], None, None, args)
    args.multimodal_type = "oct3d_paired_faf_ir_cls"
    with pytest.raises(NotImplementedError, match="GradScaler"):
        FT.train_one_epoch(None, {}, 0, [], object(), None, args)
    args.wandb = True
    with pytest.raises(NotImplementedError, match="wandb"):
        FT.train_one_epoch(None, {}, 0, [], None, None, args)


# --------------------------------------------------------------------------------------------------- the model family
def _block_keys(depth):
    per = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "norm2.weight",
           "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")
    return [f"blocks.{i}.{k}" for i in range(depth) for k in per]


TOWER_2MOD_KEYS = ["cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias", "fc_norm.weight", "fc_norm.bias",
                   "head.weight", "head.bias", "mod_head_0.weight", "mod_head_0.bias", "mod_head_1.weight", "mod_head_1.bias"]
HEAD_KEYS = ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "input_norm.weight", "input_norm.bias"]


def small_cfg():
    """the *_3mod.json layout (vit_large_patch16_retFound_enface-vit_large_patch16_mae_joint_nodrop_3mod.json) at small sizes"""
    return {"embed_dim": 32,
            "vision_cfg": {"image_size": 32, "layers": 2, "width": 64, "patch_size": 16, "num_heads": 2, "t_patch_size": 3, "in_chans": 1,
                           "mlp_ratio": 4, "norm_layer_eps": 1e-6, "layer_decay": 0.65, "weight_decay": 0.05, "drop_path_rate": 0.2,
                           "use_flash_attn": True, "attn_drop_rate": 0.0, "drop_rate": 0.0, "global_pool": True, "num_frames": 6,
                           "model_name": "ViT_ST_nodrop"},
            "text_cfg": {"image_size": 48, "layers": 2, "width": 64, "patch_size": 16, "num_heads": 2, "in_chans": 3, "mlp_ratio": 4,
                         "norm_layer_eps": 1e-6, "layer_decay": 0.65, "weight_decay": 0.05, "drop_path_rate": 0.2, "use_flash_attn": True,
                         "dropout": 0.5, "attn_drop_rate": 0.0, "drop_rate": 0.0, "global_pool": True,
                         "vit_model_name": "ViT_flash_attn_2mod"}}


def test_state_dict_keys_are_the_references():
    from octcubem_amd import coem, models_vit_2mod
    t = models_vit_2mod.VisionTransformer(image_size=48, out_dim=32, embed_dim=64, depth=2, num_heads=2)
    assert sorted(t.state_dict()) == sorted(TOWER_2MOD_KEYS + _block_keys(2))
    assert tuple(t.head.weight.shape) == (64, 64) and tuple(t.mod_head_1.weight.shape) == (32, 64)
    assert isinstance(t.dropout, torch.nn.Dropout) and t.flash_compat is True          # flash semantics unless told otherwise
    c = models_vit_2mod.VisionTransformer(image_size=48, out_dim=32, embed_dim=64, depth=1, num_heads=2, global_pool=False)
    assert "norm.weight" in c.state_dict() and "fc_norm.weight" not in c.state_dict()
    with pytest.raises(ValueError):
        t.forward(torch.zeros(1, 3, 48, 48), modality=2)
    with pytest.raises(ValueError):
        models_vit_2mod.VisionTransformer(image_size=48, out_dim=30, embed_dim=64, depth=1, num_heads=2)
    assert list(coem.ClassificationHead(96, 32, 5).state_dict()) == HEAD_KEYS
    model = coem.create_model_from_config(small_cfg(), three=True, num_classes=5)
    keys = set(model.state_dict())
    assert {"logit_scale", "logit_scale1", "logit_scale2"} <= keys
    assert {f"classification_head.{k}" for k in HEAD_KEYS} <= keys and {f"text.{k}" for k in TOWER_2MOD_KEYS} <= keys
    assert keys == ({"logit_scale", "logit_scale1", "logit_scale2"} | {f"classification_head.{k}" for k in HEAD_KEYS}
                    | {f"text.{k}" for k in t.state_dict()} | {f"visual.{k}" for k in model.visual.state_dict()})
    assert tuple(model.classification_head.fc1.weight.shape) == (32, 96) and tuple(model.classification_head.fc2.weight.shape) == (5, 32)
    for p in (model.logit_scale, model.logit_scale1, model.logit_scale2):
        assert abs(float(p.detach()) - math.log(1 / 0.07)) < 1e-6
    two = coem.create_model_from_config(small_cfg(), num_classes=2)
    assert tuple(two.classification_head.fc1.weight.shape) == (32, 64) and "logit_scale1" not in two.state_dict()


@pytest.mark.parametrize("three,num_classes,want", [(False, None, "CustomTextCLIP"), (True, None, "CustomTextCLIP3Mod"),
                                                    (False, 2, "CustomTextCLIPClassification"), (True, 5, "CustomTextCLIP3ModClassification")])
def test_create_model_from_config_picks_the_class(three, num_classes, want):
    from octcubem_amd import coem, models_vit_2mod, models_vit_st
    model = coem.create_model_from_config(small_cfg(), three=three, num_classes=num_classes)
    assert type(model).__name__ == want
    assert isinstance(model.visual, models_vit_st.VisionTransformer) and isinstance(model.text, models_vit_2mod.VisionTransformer)
    assert len(model.text.blocks) == 2 and model.text.out_dim == 32 and model.text.flash_compat is True
    assert coem.create_model_from_config(small_cfg(), flash_semantics=False).text.flash_compat is False
    cfg = small_cfg()
    cfg["text_cfg"]["vit_model_name"] = "ViT_flash_attn_3mod"
    with pytest.raises(NotImplementedError):
        coem.create_model_from_config(cfg)


def test_lock_freezes_and_unlocks_the_references_groups():
    from octcubem_amd import models_vit_2mod
    t = models_vit_2mod.VisionTransformer(image_size=48, out_dim=32, embed_dim=64, depth=3, num_heads=2)
    t.lock()
    assert not any(p.requires_grad for p in t.parameters())
    t.lock(unlocked_groups=2)
    on = {k for k, p in t.named_parameters() if p.requires_grad}
    assert on == {"head.weight", "head.bias", "fc_norm.weight", "fc_norm.bias"} | {k for k in _block_keys(3) if k.startswith("blocks.2.")}
