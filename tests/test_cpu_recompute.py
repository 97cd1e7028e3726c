"""CPU tests of activation recomputation and tower locking: the ABI of the two rebuild kernels (octmae_ln_apply, octmae_gelu_apply), the
``recompute`` attribute of the Blocks and ``set_grad_checkpointing`` of the models, ``lock()`` of the OCT and the en-face tower against
the group lists of the reference written out by name, and the three tower calls of coem.CustomTextCLIP."""
import os
import re
import subprocess
from functools import partial

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("octmae_ln_apply", "octmae_gelu_apply")
LN = partial(nn.LayerNorm, eps=1e-6)


def test_abi_declares_the_rebuild_kernels():
    from octcubem_amd import _lib
    header = open(os.path.join(ROOT, "include", "octmae.h")).read()
    assert _lib.expected_abi_version() >= 26
    assert re.search(r"^ \* 26: octmae_ln_apply", header, re.M)
    for sym in SYMBOLS:
        assert re.search(rf"^int {sym}\(", header, re.M), sym
        assert sym in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["octmae_ln_apply"]) == 9 and len(_lib.SIGNATURES["octmae_gelu_apply"]) == 4
    mk = open(os.path.join(ROOT, "octcubem_amd", "csrc", "Makefile")).read()
    assert "recompute.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1)
    for lib in ("liboctmae.so", "liboctmae_f16.so"):
        path = os.path.join(ROOT, "octcubem_amd", lib)
        if os.path.exists(path):
            names = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
            for sym in SYMBOLS:
                assert re.search(rf"\bT {sym}$", names, re.M), (lib, sym)


def test_ops_has_the_two_wrappers_and_the_levels():
    from octcubem_amd import ops, video_vit
    assert callable(ops.ln_apply) and callable(ops.gelu_apply)
    assert (ops.RECOMPUTE_NONE, ops.RECOMPUTE_LIGHT, ops.RECOMPUTE_FULL) == (0, 1, 2)
    assert video_vit.RECOMPUTE_LEVELS == {"none": 0, "light": 1, "full": 2}


# ------------------------------------------------------------------------------------------------ towers built on the CPU
def st_tower(depth, flash=False):
    from octcubem_amd import models_vit_st
    return models_vit_st.VisionTransformer(num_frames=4, t_patch_size=2, img_size=32, patch_size=16, in_chans=1, num_classes=8, embed_dim=64,
                                           depth=depth, num_heads=2, norm_layer=LN, sep_pos_embed=True, cls_embed=True, use_flash_attn=flash)


def enface_tower(depth, global_pool=False):
    from octcubem_amd import models_vit_flash_attn
    return models_vit_flash_attn.VisionTransformer(img_size=32, patch_size=16, in_chans=3, num_classes=8, embed_dim=64, depth=depth,
                                                   num_heads=2, norm_layer=LN, global_pool=global_pool)


def test_set_recompute_reaches_every_block_and_rejects_unknown_modes():
    from octcubem_amd import video_vit
    assert video_vit.Block.recompute == "none" and video_vit.FlashBlock.recompute == "none"
    for m in (st_tower(3), st_tower(3, flash=True), enface_tower(3)):
        assert [b.recompute for b in m.blocks] == ["none"] * 3
        for mode in ("light", "full", "none"):
            assert video_vit.set_recompute(m, mode) == 3
            assert [b.recompute for b in m.blocks] == [mode] * 3
        for bad in ("Full", "checkpoint", "", None, 2, True):
            with pytest.raises(ValueError):
                video_vit.set_recompute(m, bad)
        assert [b.recompute for b in m.blocks] == ["none"] * 3          # a refused mode changes nothing
    blk = video_vit.Block(64, 2)
    assert video_vit.set_recompute(blk, "full") == 1 and blk.recompute == "full"            # the module itself counts
    assert video_vit.Block.recompute == "none"                                              # instances, never the class


def test_set_grad_checkpointing_of_the_models():
    from octcubem_amd import models_mae, models_mae_2d, models_vit, models_vit_2mod, models_vit_3dhead
    mae = models_mae.MaskedAutoencoderViT(input_size=32, patch_size=16, in_chans=1, embed_dim=64, depth=2, num_heads=2, decoder_embed_dim=64,
                                          decoder_depth=2, decoder_num_heads=2, norm_layer=LN, num_frames=4, t_patch_size=2,
                                          sep_pos_embed=True, cls_embed=True, pred_t_dim=4)
    mae2d = models_mae_2d.MaskedAutoencoderViT(img_size=32, patch_size=16, in_chans=3, embed_dim=64, depth=2, num_heads=2,
                                               decoder_embed_dim=64, decoder_depth=2, decoder_num_heads=2, norm_layer=LN)
    vit = models_vit.VisionTransformer(img_size=32, patch_size=16, num_classes=8, embed_dim=64, depth=2, num_heads=2, norm_layer=LN)
    twomod = models_vit_2mod.VisionTransformer(image_size=32, out_dim=8, embed_dim=64, depth=2, num_heads=2, norm_layer=LN)
    head3d = models_vit_3dhead.VisionTransformerWith3DPoolingHead(img_size=32, num_classes=8, embed_dim=64, depth=2, num_heads=2, norm_layer=LN)
    for m in (mae, mae2d, vit, twomod, head3d, st_tower(2), st_tower(2, flash=True), enface_tower(2)):
        stacks = [m.blocks] + ([m.decoder_blocks] if hasattr(m, "decoder_blocks") else [])
        modes = lambda: {b.recompute for s in stacks for b in s}      # noqa: E731
        assert modes() == {"none"}
        m.set_grad_checkpointing()                   # the reference's call with its default arguments: torch.utils.checkpoint's effect
        assert modes() == {"full"}
        m.set_grad_checkpointing(True, "light")
        assert modes() == {"light"}
        m.set_grad_checkpointing(enable=False)
        assert modes() == {"none"}
        m.set_grad_checkpointing(False, mode="light")
        assert modes() == {"none"}
        with pytest.raises(ValueError):
            m.set_grad_checkpointing(True, "heavy")


# ------------------------------------------------------------------------------------------------ lock()
# The reference's group lists by parameter-name prefix, first group to last:
#   models_vit_st_flash_attn_nodrop.py:307-331   [patch_embed, pos_embed_spatial, pos_embed_temporal, pos_embed_class, cls_token],
#                                                blocks[:-1] one each, [blocks[-1], norm], [fc_aggregate_cls, aggregate_cls_norm, head]
#   models_vit_flash_attn.py:207-219             [patch_embed, cls_token, pos_embed], blocks[:-1] one each, [blocks[-1], fc_norm | norm], head
ST_GROUPS = [["patch_embed", "pos_embed_spatial", "pos_embed_temporal", "pos_embed_class", "cls_token"], ["blocks.0"], ["blocks.1"],
             ["blocks.2"], ["blocks.3", "norm"], ["fc_aggregate_cls", "aggregate_cls_norm", "head"]]
ENFACE_GROUPS = [["patch_embed", "cls_token", "pos_embed"], ["blocks.0"], ["blocks.1"], ["blocks.2"], ["blocks.3", "norm"], ["head"]]
ENFACE_POOL_GROUPS = ENFACE_GROUPS[:4] + [["blocks.3", "fc_norm"], ["head"]]


def expected_trainable(names, groups, k):
    open_ = [p for g in (groups[-k:] if k else []) for p in g]
    return {n for n in names if any(n == p or n.startswith(p + ".") for p in open_)}


@pytest.mark.parametrize("k", [0, 1, 2, 3, 99])
@pytest.mark.parametrize("which", ["st", "st_flash", "enface", "enface_pool"])
def test_lock_follows_the_reference_group_lists(which, k):
    m, groups = {"st": (lambda: st_tower(4), ST_GROUPS), "st_flash": (lambda: st_tower(4, flash=True), ST_GROUPS),
                 "enface": (lambda: enface_tower(4), ENFACE_GROUPS),
                 "enface_pool": (lambda: enface_tower(4, global_pool=True), ENFACE_POOL_GROUPS)}[which]
    m = m()
    names = [n for n, _ in m.named_parameters()]
    assert all(any(n == p or n.startswith(p + ".") for g in groups for p in g) for n in names)     # the groups cover the model
    for p in m.parameters():                    # as after a first forward: every gradient is a (zero-filled) buffer
        p.grad = torch.zeros_like(p)
    m.lock(unlocked_groups=k, freeze_bn_stats=False)
    got = {n for n, p in m.named_parameters() if p.requires_grad}
    assert got == expected_trainable(names, groups, k), (which, k)
    if k == 0:
        assert got == set()
    if k == 1:
        assert got == {"head.weight", "head.bias"}
    if k == 2:
        last_norm = "fc_norm" if which == "enface_pool" else "norm"
        assert {"head.weight", f"{last_norm}.weight", "blocks.3.norm1.weight", "blocks.3.mlp.fc2.bias"} <= got
        assert not any(n.startswith(("blocks.2.", "blocks.0.", "patch_embed.")) or n == "cls_token" for n in got)
    if k == 3:
        assert any(n.startswith("blocks.2.") for n in got) and not any(n.startswith("blocks.1.") for n in got)
    if k == 99:
        assert got == set(names)
    for n, p in m.named_parameters():
        assert (p.grad is None) == (not p.requires_grad), n       # what is frozen has given up its gradient; what is open keeps it
    m.lock()                                    # locking again closes what was open
    assert not any(p.requires_grad for p in m.parameters()) and all(p.grad is None for p in m.parameters())


def test_the_two_older_lock_methods_also_drop_the_gradients():
    from octcubem_amd import models_vit_2mod, models_vit_3dhead
    twomod = models_vit_2mod.VisionTransformer(image_size=32, out_dim=8, embed_dim=64, depth=2, num_heads=2, norm_layer=LN)
    head3d = models_vit_3dhead.VisionTransformerWith3DPoolingHead(img_size=32, num_classes=8, embed_dim=64, depth=2, num_heads=2, norm_layer=LN)
    for m, open_ in ((twomod, {"head.weight", "head.bias"}),
                     (head3d, {f"{h}.{w}" for h in ("fc_aggregate_cls", "aggregate_cls_norm", "head") for w in ("weight", "bias")})):
        for p in m.parameters():
            p.grad = torch.zeros_like(p)
        m.lock(unlocked_groups=1)
        assert {n for n, p in m.named_parameters() if p.requires_grad} == open_
        for n, p in m.named_parameters():
            assert (p.grad is None) == (n not in open_), n


# ------------------------------------------------------------------------------------------------ the COEM model's three calls
class _StubTower(nn.Module):
    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(1))
        self.calls = []

    def lock(self, *args, **kwargs):
        self.calls.append(("lock", args, kwargs))

    def set_grad_checkpointing(self, *args, **kwargs):
        self.calls.append(("ckpt", args, kwargs))


def test_custom_text_clip_reaches_the_towers():
    from octcubem_amd import coem
    for cls, extra in ((coem.CustomTextCLIP, ()), (coem.CustomTextCLIP3Mod, ()), (coem.CustomTextCLIPClassification, (4, 8)),
                       (coem.CustomTextCLIP3ModClassification, (4, 8))):
        v, t = _StubTower(), _StubTower()
        m = cls(v, t, *extra)
        m.lock_image_tower(unlocked_groups=9, freeze_bn_stats=True)
        assert v.calls == [("lock", (), {"unlocked_groups": 9, "freeze_bn_stats": True})] and t.calls == []
        m.lock_text_tower(3, False)
        assert t.calls == [("lock", (3, False), {})] and len(v.calls) == 1           # positionally, as model.py:653-654
        m.lock_text_tower()
        assert t.calls[-1] == ("lock", (0, True), {})
        m.set_grad_checkpointing()
        assert v.calls[-1] == ("ckpt", (True, "full"), {}) and t.calls[-1] == ("ckpt", (True, "full"), {})
        m.set_grad_checkpointing(enable=False)
        assert v.calls[-1][1][0] is False and t.calls[-1][1][0] is False
        m.set_grad_checkpointing(True, mode="light")
        assert v.calls[-1] == ("ckpt", (True, "light"), {}) and t.calls[-1] == ("ckpt", (True, "light"), {})


def test_custom_text_clip_on_real_towers():
    from octcubem_amd import coem
    m = coem.CustomTextCLIP(st_tower(4, flash=True), enface_tower(4))
    m.lock_image_tower(unlocked_groups=2)
    m.set_grad_checkpointing()
    assert {n for n, p in m.visual.named_parameters() if p.requires_grad} == expected_trainable(
        [n for n, _ in m.visual.named_parameters()], ST_GROUPS, 2)
    assert all(p.requires_grad for p in m.text.parameters()) and m.logit_scale.requires_grad
    assert {b.recompute for b in list(m.visual.blocks) + list(m.text.blocks)} == {"full"}
    m.lock_text_tower(1)
    assert {n for n, p in m.text.named_parameters() if p.requires_grad} == {"head.weight", "head.bias"}
