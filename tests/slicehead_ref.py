"""fp32 CPU composition of the RETFound-all model (the slice-pooled 2-D ViT, OCTCube/models_vit_3dhead.py and
models_vit_3dhead_flash_attn.py) from oracle.vit_ref's pieces: the oracle the slice-head tests compare against, pinned to the
reference by tests/golden/slicehead_small.npz (tools/gen_golden_slicehead.py)."""
import torch
import torch.nn.functional as F

from oracle import vit_ref as V

# the reduced configuration of the fixture: real kernels (head_dim 64), T = 17 tokens, 4 slices per volume, an odd class count
SMALL = dict(img_size=64, patch_size=16, in_chans=3, num_classes=3, embed_dim=128, depth=2, num_heads=2)
SLICES, BATCH, PARAM_SEED, DATA_SEED = 4, 2, 71, 72


def config(global_pool=True, **kw):
    return V.ViT2DConfig(**{**SMALL, **kw, "global_pool": global_pool})


def param_shapes(cfg):
    """The reference's state_dict shapes: the 2-D ViT's, then fc_aggregate_cls and aggregate_cls_norm (registration order)."""
    s = dict(V.vit2d_param_shapes(cfg))
    D = cfg.embed_dim
    s.update({"fc_aggregate_cls.weight": (D, D), "fc_aggregate_cls.bias": (D,), "aggregate_cls_norm.weight": (D,),
              "aggregate_cls_norm.bias": (D,)})
    return s


def init(cfg, seed=PARAM_SEED):
    return V.init_from_shapes(param_shapes(cfg), seed=seed)


def inputs(cfg, B=BATCH, S=SLICES, seed=DATA_SEED):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, cfg.in_chans, cfg.img_size, cfg.img_size, generator=g)
    return x, torch.randint(0, cfg.num_classes, (B,), generator=g)


def slice_tokens(P, x, cfg, flash=False):
    """[B, S, C, H, W] -> the token stream after the last block, [B*S, 1 + L, D]; ``flash``: the last block returns its MLP branch."""
    B, S = x.shape[:2]
    x = x.reshape(B * S, *x.shape[2:])
    y = F.conv2d(x, P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], stride=cfg.patch_size).flatten(2).transpose(1, 2)
    y = torch.cat((P["cls_token"].expand(y.shape[0], -1, -1), y), dim=1) + P["pos_embed"]
    for i in range(cfg.depth):
        y = V.timm_block(y, P, f"blocks.{i}", cfg.num_heads, cfg.ln_eps, final_residual=not (flash and i == cfg.depth - 1))
    return y


def slice_pool(y, P, cfg, S):
    """[B*S, T, D] -> [B, D]: fc_norm(mean of the patch tokens) or norm(y)[:, 0] per slice, averaged over the S slices."""
    D = cfg.embed_dim
    if cfg.global_pool:
        f = F.layer_norm(y[:, 1:, :].mean(dim=1), (D,), P["fc_norm.weight"], P["fc_norm.bias"], cfg.ln_eps)
    else:
        f = F.layer_norm(y, (D,), P["norm.weight"], P["norm.bias"], cfg.ln_eps)[:, 0]
    return f.view(-1, S, D).mean(dim=1)


def forward(P, x, cfg, flash=False):
    """(logits [B, num_classes], features [B, D]) of VisionTransformerWith3DPoolingHead."""
    S = x.shape[1]
    f = slice_pool(slice_tokens(P, x, cfg, flash), P, cfg, S)
    f = F.linear(f, P["fc_aggregate_cls.weight"], P["fc_aggregate_cls.bias"])
    f = F.layer_norm(f, (cfg.embed_dim,), P["aggregate_cls_norm.weight"], P["aggregate_cls_norm.bias"], cfg.ln_eps)
    return F.linear(f, P["head.weight"], P["head.bias"]), f


# the gradients the fixture stores (whole when small, every 11th element otherwise)
GRAD_KEYS = ("head.weight", "head.bias", "fc_aggregate_cls.weight", "fc_aggregate_cls.bias", "aggregate_cls_norm.weight",
             "aggregate_cls_norm.bias", "{norm}.weight", "{norm}.bias", "blocks.{last}.mlp.fc2.weight", "blocks.{last}.mlp.fc2.bias",
             "patch_embed.proj.weight", "patch_embed.proj.bias")


def grad_keys(cfg):
    nm = "fc_norm" if cfg.global_pool else "norm"
    return [k.format(norm=nm, last=cfg.depth - 1) for k in GRAD_KEYS]


def sub(t):
    return t.flatten() if t.numel() <= 4096 else t.flatten()[::11]
