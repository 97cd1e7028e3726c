"""Plain-torch CPU restatement of OCTCube with the SLIViT slice head (octcubem_amd/models_vit_st_flash_attn_slivit.py) as a function of
a parameter dict with the reference's state-dict keys: the spatio-temporal trunk (oracle/vit_ref.vit_st_forward's order, non-flash
blocks), the ``[N, T, C, L]`` transposed view of its token stream, and tests/slivit_ref.head_forward on top.  Not a test module.

``dt`` (None, torch.bfloat16 or torch.float16) is the ROUNDING MODEL of tests/slivit_ref.py carried into the trunk: values are rounded to
it where the library rounds -- the operands of every GEMM and of the attention kernel, what those kernels and the LayerNorm kernels
store in 16 bits, and the activation gradients handed from kernel to kernel in 16 bits.  It fixes neither the accumulation order nor the
GELU formula's own error.  With None everything is fp32.

Weights are regenerated from seeds by shape (``init_params``), never stored.  How the default seeds and the batch were chosen, from the
restatement's own numbers alone (the fixture's ``rounding_err`` is what tests/test_gpu_stslivit.py takes its tolerances from, so it
has to be a typical value of the reference's rounding error and not a lucky draw):
  * weights, seed 2: logits of size 0.5 ... 1 on every volume.  With one output per volume a draw whose logits come out near 0
    (seed 0: 0.02 ... 0.1) makes every relative error a statement about cancellation in the last dot product, not about the model.
  * 16 volumes: the relative L2 error of FOUR logits under bfloat16 rounding ranges over 1.9e-3 ... 6.0e-3 from one input draw to the
    next (input seeds 12 ... 19); of sixteen, over 3.7e-3 ... 5.5e-3.
  * inputs, seed 16: the error of the scalar loss is a signed sum over the volumes and scatters around 0 whatever the batch (input
    seeds 12 ... 27 at 16 volumes: 6e-4 ... 4.3e-3 in bfloat16, RMS 2.3e-3; 1e-5 ... 3.2e-4 in half, RMS 1.6e-4).  Seed 16 is the draw
    closest to the RMS in both types (2.8e-3 and 1.3e-4).
Pinned against tests/golden/stslivit_small.npz, which
tools/gen_golden_stslivit.py produced by running the reference's own model class."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import vit_ref as V
from tests import slivit_ref as R
from tests.slivit_ref import linear, rb, rf

HP = "SLIViT_head."
SMALL = dict(num_frames=9, t_patch_size=3, img_size=48, patch_size=16, in_chans=1, embed_dim=64, depth=2, num_heads=2, slivit_depth_num=2,
             num_classes=1, batch=16)


def trunk_cfg(cfg=SMALL):
    return V.ViTSTConfig(num_frames=cfg["num_frames"], t_patch_size=cfg["t_patch_size"], img_size=cfg["img_size"], patch_size=cfg["patch_size"],
                         in_chans=cfg["in_chans"], num_classes=cfg["num_classes"], embed_dim=cfg["embed_dim"], depth=cfg["depth"],
                         num_heads=cfg["num_heads"], global_pool=True)


def head_cfg(cfg=SMALL):
    """the head's sizes as the reference fixes them (models_vit_st_flash_attn_slivit.py:92-94), in tests/slivit_ref's vocabulary"""
    T, h, w = trunk_cfg(cfg).grid
    return dict(num_patches=T, vit_dim=256, heads=20, dim_head=64, vit_depth=cfg["slivit_depth_num"], mlp_dim=512,
                patch_height=cfg["embed_dim"], patch_width=h * w, num_classes=cfg["num_classes"], batch=cfg["batch"],
                depths=(0, 0, 0, 0), hidden_sizes=(8, 8, 8, 8))


def model_shapes(cfg=SMALL):
    """the reference's state dict: the trunk's keys without ``head.*`` (``norm.*`` included), then the head's under ``SLIViT_head.``"""
    out = OrderedDict((k, v) for k, v in V.vit_st_param_shapes(trunk_cfg(cfg)).items() if not k.startswith("head."))
    for k, v in R.head_shapes(head_cfg(cfg)).items():
        out[HP + k] = v
    return out


def init_params(cfg=SMALL, seed=2):
    trunk = V.init_from_shapes(OrderedDict((k, v) for k, v in model_shapes(cfg).items() if not k.startswith(HP)), seed=seed, bias_std=0.1)
    head = R.init_params(head_cfg(cfg), seed=seed + 1)
    P = OrderedDict(trunk)
    for k in R.head_shapes(head_cfg(cfg)):
        P[HP + k] = head[k]
    assert list(P.keys()) == list(model_shapes(cfg).keys())
    return P


def make_inputs(cfg=SMALL, seed=16):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((cfg["batch"], cfg["in_chans"], cfg["num_frames"], cfg["img_size"], cfg["img_size"]), generator=g)
    target = torch.randn((cfg["batch"], cfg["num_classes"]), generator=g)
    return x, target


def _ln(x, P, k, eps):
    return F.layer_norm(x, (x.shape[-1],), P[k + ".weight"], P[k + ".bias"], eps)


def st_block(x, P, p, H, eps, dt, final_residual=True):
    """util/video_vit.Block (:181-184) with separate q / k / v Linears, rounded where ops.BlockFn rounds"""
    Bn, N, C = x.shape
    HD = C // H
    y = rb(rf(_ln(x, P, p + ".norm1", eps), dt), dt)
    q, k, v = (rb(rf(rf(y, dt) @ rf(P[f"{p}.attn.{n}.weight"], dt).t() + P[f"{p}.attn.{n}.bias"], dt), dt).view(Bn, N, H, HD).transpose(1, 2)
               for n in ("q", "k", "v"))
    att = torch.softmax((q @ k.transpose(-1, -2)) * HD ** -0.5, dim=-1)
    o = rb(rf((att @ v).transpose(1, 2).reshape(Bn, N, C), dt), dt)
    x = x + linear(o, P[p + ".attn.proj.weight"], P[p + ".attn.proj.bias"], dt)
    y = rb(rf(_ln(x, P, p + ".norm2", eps), dt), dt)
    pre = rf(linear(y, P[p + ".mlp.fc1.weight"], P[p + ".mlp.fc1.bias"], dt), dt)
    h = linear(rf(F.gelu(pre), dt), P[p + ".mlp.fc2.weight"], P[p + ".mlp.fc2.bias"], dt)
    return x + h if final_residual else h


def trunk_forward(P, x, cfg=SMALL, dt=None, last_residual=True):
    """fp32 volumes [N, C, T, H, W] -> the final token stream [N, 1 + T L, C]"""
    c = trunk_cfg(cfg)
    k = (c.t_patch_size, c.patch_size, c.patch_size)
    y = F.conv3d(rf(x, dt), rf(P["patch_embed.proj.weight"], dt), P["patch_embed.proj.bias"], stride=k).flatten(3)
    y = rb(rf(torch.einsum("ncts->ntsc", y), dt), dt)                      # the patch GEMM stores 16-bit tokens
    N, T, L, C = y.shape
    y = torch.cat((P["cls_token"].expand(N, -1, -1), y.reshape(N, T * L, C)), dim=1)
    pos = P["pos_embed_spatial"].repeat(1, T, 1) + torch.repeat_interleave(P["pos_embed_temporal"], L, dim=1)
    y = y + torch.cat([P["pos_embed_class"].expand(1, -1, -1), pos], 1)
    for i in range(c.depth):
        y = st_block(y, P, f"blocks.{i}", c.num_heads, c.ln_eps, dt, final_residual=last_residual or i < c.depth - 1)
    return y


def forward(P, x, cfg=SMALL, dt=None, last_residual=True):
    """(embedding [N, T, C, L] -- the reference's strided view, logits [N, num_classes])"""
    stream = trunk_forward(P, x, cfg, dt, last_residual)
    N, _, C = stream.shape
    T, h, w = trunk_cfg(cfg).grid
    emb = stream[:, 1:, :].reshape(N, T, h * w, C).transpose(2, 3)
    head = {k[len(HP):]: v for k, v in P.items() if k.startswith(HP)}
    return emb, R.head_forward(head, emb, head_cfg(cfg), dt)


def forward_backward(P, x, target, cfg=SMALL, dt=None, last_residual=True):
    """(embedding, logits, MSE loss, {key: gradient or None}) with autograd over fresh leaves of P"""
    leaves = OrderedDict((k, v.detach().clone().requires_grad_(True)) for k, v in P.items())
    emb, logits = forward(leaves, x, cfg, dt, last_residual)
    loss = F.mse_loss(logits, target)
    loss.backward()
    return emb.detach(), logits.detach(), loss.detach(), OrderedDict((k, v.grad) for k, v in leaves.items())


def subsample(t, n=256):
    """n entries of t at an ODD stride: a stride that divides the row length (256 samples of a [256, 576] matrix: every 576th entry)
    would read one column only"""
    f = t.reshape(-1)
    return f[::max(1, f.numel() // n) | 1][:n]


NO_GRAD = ("norm.weight", "norm.bias")            # the reference builds ``norm`` and never applies it
