"""Plain-torch CPU restatement of the SLIViT baseline (octcubem_amd/model_slivit_baseline.py): HF ConvNextModel's embeddings + encoder
and the vit-pytorch 1.x ViT on top, as functions of a parameter dict with the reference's state-dict keys.  Not a test module.

``operand_dtype`` (None, torch.bfloat16 or torch.float16) is the ROUNDING MODEL: with a dtype, values are rounded to it (and widened
back to fp32) at the points where the library rounds -- the weights and activations that enter a GEMM or the attention kernel, what
those kernels store in 16 bits, and, in the backward, the activation gradients the library hands from GEMM to GEMM in 16 bits.  It
fixes neither the accumulation order nor the GELU formula's own error.  With None everything is fp32.

Weights are regenerated from a seed by shape (``init_params``), never stored.  ``layer_scale_parameter`` is drawn from U(0.5, 1.5): at
HF's initial 1e-6 every ConvNeXt branch is invisible in the output and a broken branch would pass."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

SMALL = dict(depths=(1, 1, 2, 1), hidden_sizes=(32, 64, 96, 128), num_patches=3, vit_dim=64, heads=2, dim_head=64, vit_depth=2, mlp_dim=128,
             patch_height=128, patch_width=4, batch=2, num_classes=3, input_shape=(2, 3, 64, 192))
FE = "feature_extractor."


class _RoundFwd(torch.autograd.Function):
    """value rounded to ``dt`` in the forward, gradient untouched"""

    @staticmethod
    def forward(ctx, x, dt):
        return x.to(dt).float()

    @staticmethod
    def backward(ctx, g):
        return g, None


class _RoundBwd(torch.autograd.Function):
    """value untouched, gradient rounded to ``dt``"""

    @staticmethod
    def forward(ctx, x, dt):
        ctx.dt = dt
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dt).float(), None


def rf(x, dt):
    return x if dt is None else _RoundFwd.apply(x, dt)


def rb(x, dt):
    return x if dt is None else _RoundBwd.apply(x, dt)


def linear(x, w, b, dt):
    """x @ w.T + b on operands rounded to dt; the gradient arriving at the output is rounded too (the library casts dy once and feeds
    that copy to both the weight- and the input-gradient GEMM)."""
    y = rf(x, dt) @ rf(w, dt).t()
    if b is not None:
        y = y + b
    return rb(y, dt)


# ------------------------------------------------------------------------------------------------ parameters
def extractor_shapes(cfg):
    d, h = cfg["depths"], cfg["hidden_sizes"]
    out = OrderedDict()
    out["0.patch_embeddings.weight"] = (h[0], 3, 4, 4)
    out["0.patch_embeddings.bias"] = (h[0],)
    out["0.layernorm.weight"] = (h[0],)
    out["0.layernorm.bias"] = (h[0],)
    prev = h[0]
    for s in range(4):
        c = h[s]
        if s > 0:
            out[f"1.stages.{s}.downsampling_layer.0.weight"] = (prev,)
            out[f"1.stages.{s}.downsampling_layer.0.bias"] = (prev,)
            out[f"1.stages.{s}.downsampling_layer.1.weight"] = (c, prev, 2, 2)
            out[f"1.stages.{s}.downsampling_layer.1.bias"] = (c,)
        for l in range(d[s]):
            p = f"1.stages.{s}.layers.{l}."
            out[p + "layer_scale_parameter"] = (c,)
            out[p + "dwconv.weight"] = (c, 1, 7, 7)
            out[p + "dwconv.bias"] = (c,)
            out[p + "layernorm.weight"] = (c,)
            out[p + "layernorm.bias"] = (c,)
            out[p + "pwconv1.weight"] = (4 * c, c)
            out[p + "pwconv1.bias"] = (4 * c,)
            out[p + "pwconv2.weight"] = (c, 4 * c)
            out[p + "pwconv2.bias"] = (c,)
        prev = c
    return out


def head_shapes(cfg):
    D, P, inner = cfg["vit_dim"], cfg["num_patches"], cfg["heads"] * cfg["dim_head"]
    pd = cfg["patch_height"] * cfg["patch_width"]
    out = OrderedDict()
    out["pos_embedding"] = (1, P + 1, D)
    out["cls_token"] = (1, 1, D)
    out["to_patch_embedding.1.weight"] = (pd,)
    out["to_patch_embedding.1.bias"] = (pd,)
    out["to_patch_embedding.2.weight"] = (D, pd)
    out["to_patch_embedding.2.bias"] = (D,)
    out["to_patch_embedding.3.weight"] = (D,)
    out["to_patch_embedding.3.bias"] = (D,)
    out["transformer.norm.weight"] = (D,)
    out["transformer.norm.bias"] = (D,)
    for i in range(cfg["vit_depth"]):
        p = f"transformer.layers.{i}."
        out[p + "0.norm.weight"] = (D,)
        out[p + "0.norm.bias"] = (D,)
        out[p + "0.to_qkv.weight"] = (3 * inner, D)
        out[p + "0.to_out.0.weight"] = (D, inner)
        out[p + "0.to_out.0.bias"] = (D,)
        out[p + "1.net.0.weight"] = (D,)
        out[p + "1.net.0.bias"] = (D,)
        out[p + "1.net.1.weight"] = (cfg["mlp_dim"], D)
        out[p + "1.net.1.bias"] = (cfg["mlp_dim"],)
        out[p + "1.net.4.weight"] = (D, cfg["mlp_dim"])
        out[p + "1.net.4.bias"] = (D,)
    out["mlp_head.weight"] = (cfg["num_classes"], D)
    out["mlp_head.bias"] = (cfg["num_classes"],)
    return out


def model_shapes(cfg):
    """The SLIViT state dict: the head's keys, then the extractor's under ``feature_extractor.``."""
    out = head_shapes(cfg)
    for k, v in extractor_shapes(cfg).items():
        out[FE + k] = v
    return out


def _is_norm_weight(k):
    return k.endswith(("layernorm.weight", "norm.weight", "downsampling_layer.0.weight", "to_patch_embedding.1.weight",
                       "to_patch_embedding.3.weight", "net.0.weight"))


def init_params(cfg=SMALL, seed=0):
    """fp32 parameters by key and shape from one generator: matrices and filters N(0, 1 / fan_in), biases N(0, 0.1^2), LayerNorm
    weights 1 + N(0, 0.1^2), layer scale U(0.5, 1.5), cls token N(0, 1), pos_embedding the reference's constant rows."""
    g = torch.Generator().manual_seed(seed)
    P = OrderedDict()
    for k, shp in model_shapes(cfg).items():
        if k == "pos_embedding":
            v = torch.arange(shp[1]).repeat(shp[2], 1).t().unsqueeze(0).float()
        elif k.endswith("layer_scale_parameter"):
            v = 0.5 + torch.rand(shp, generator=g)
        elif _is_norm_weight(k):
            v = 1.0 + 0.1 * torch.randn(shp, generator=g)
        elif k.endswith("bias"):
            v = 0.1 * torch.randn(shp, generator=g)
        elif k == "cls_token":
            v = torch.randn(shp, generator=g)
        else:
            fan_in = 1
            for n in shp[1:]:
                fan_in *= n
            v = torch.randn(shp, generator=g) * fan_in ** -0.5
        P[k] = v
    return P


def make_inputs(cfg=SMALL, seed=1):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(cfg["input_shape"], generator=g)
    target = torch.randn((cfg["batch"], cfg["num_classes"]), generator=g)
    return img, target


# ------------------------------------------------------------------------------------------------ forward
def _ln(x, P, k, eps):
    return F.layer_norm(x, (x.shape[-1],), P[k + ".weight"], P[k + ".bias"], eps)


def convnext_layer(x, P, p, dt):
    """x: channels-last fp32 [B, H, W, C]"""
    C = x.shape[-1]
    z = F.conv2d(x.permute(0, 3, 1, 2), P[p + "dwconv.weight"], P[p + "dwconv.bias"], padding=3, groups=C).permute(0, 2, 3, 1)
    y = rb(rf(_ln(z, P, p + "layernorm", 1e-6), dt), dt)           # the LayerNorm kernel's 16-bit output; its gradient arrives in 16 bits
    pre = rf(linear(y, P[p + "pwconv1.weight"], P[p + "pwconv1.bias"], dt), dt)      # stored pre-activation (16 bits); d pre is rounded once
    act = rf(F.gelu(pre), dt)
    branch = rf(act, dt) @ rf(P[p + "pwconv2.weight"], dt).t() + P[p + "pwconv2.bias"]
    return x + P[p + "layer_scale_parameter"] * rb(branch, dt)    # d branch = gamma * dout, rounded once


def extractor_forward(P, img, cfg=SMALL, dt=None, prefix=""):
    """fp32 NCHW image -> fp32 NCHW feature map [B, C4, H / 32, W / 32]"""
    P = {k[len(prefix):]: v for k, v in P.items() if k.startswith(prefix)}
    B, Cin, H, W = img.shape
    rows = img.view(B, Cin, H // 4, 4, W // 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(B, H // 4, W // 4, Cin * 16)
    x = linear(rows, P["0.patch_embeddings.weight"].flatten(1), P["0.patch_embeddings.bias"], dt)
    x = rb(rf(_ln(x, P, "0.layernorm", 1e-6), dt), dt)             # the stem's LayerNorm kernel writes, and its backward reads, 16 bits
    for s in range(4):
        if s > 0:
            B, H, W, C = x.shape
            y = rb(rf(_ln(x, P, f"1.stages.{s}.downsampling_layer.0", 1e-6), dt), dt)
            rows = y.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C * 4)
            x = linear(rows, P[f"1.stages.{s}.downsampling_layer.1.weight"].flatten(1), P[f"1.stages.{s}.downsampling_layer.1.bias"], dt)
        for l in range(cfg["depths"][s]):
            x = convnext_layer(x, P, f"1.stages.{s}.layers.{l}.", dt)
    return x.permute(0, 3, 1, 2).contiguous()


def head_forward(P, feat, cfg=SMALL, dt=None):
    """fp32 feature map -> logits [B, num_classes]"""
    Bn, Pn, D, H, HD = feat.shape[0], cfg["num_patches"], cfg["vit_dim"], cfg["heads"], cfg["dim_head"]
    x = feat.reshape(Bn, Pn, cfg["patch_height"] * cfg["patch_width"])
    x = _ln(x, P, "to_patch_embedding.1", 1e-5)
    x = linear(x, P["to_patch_embedding.2.weight"], P["to_patch_embedding.2.bias"], dt)
    x = _ln(x, P, "to_patch_embedding.3", 1e-5)
    x = torch.cat((P["cls_token"].expand(Bn, -1, -1), x), dim=1) + P["pos_embedding"][:, :Pn + 1]
    N = Pn + 1
    for i in range(cfg["vit_depth"]):
        p = f"transformer.layers.{i}."
        y = rb(rf(_ln(x, P, p + "0.norm", 1e-5), dt), dt)
        qkv = rf(rf(y, dt) @ rf(P[p + "0.to_qkv.weight"], dt).t(), dt)           # the qkv GEMM stores 16 bits
        qkv = rb(qkv, dt).view(Bn, N, 3, H, HD)                                   # the attention backward writes dqkv in 16 bits
        q, k, v = (qkv[:, :, j].transpose(1, 2) for j in range(3))              # [B, H, N, HD]
        att = torch.softmax((q @ k.transpose(-1, -2)) * HD ** -0.5, dim=-1)
        o = rb(rf((att @ v).transpose(1, 2).reshape(Bn, N, H * HD), dt), dt)     # o is stored, and dO handed over, in 16 bits
        x = x + linear(o, P[p + "0.to_out.0.weight"], P[p + "0.to_out.0.bias"], dt)
        y = rb(rf(_ln(x, P, p + "1.net.0", 1e-5), dt), dt)
        pre = rf(linear(y, P[p + "1.net.1.weight"], P[p + "1.net.1.bias"], dt), dt)
        act = rf(F.gelu(pre), dt)
        x = x + linear(act, P[p + "1.net.4.weight"], P[p + "1.net.4.bias"], dt)
    c = rb(rf(_ln(x[:, 0], P, "transformer.norm", 1e-5), dt), dt)
    return c @ P["mlp_head.weight"].t() + P["mlp_head.bias"]


def forward(P, img, cfg=SMALL, dt=None):
    feat = extractor_forward(P, img, cfg, dt, prefix=FE)
    return feat, head_forward(P, feat, cfg, dt)


def forward_backward(P, img, target, cfg=SMALL, dt=None):
    """(feature map, logits, MSE loss, {key: gradient}) with autograd over fresh leaves of P"""
    leaves = OrderedDict((k, v.detach().clone().requires_grad_(True)) for k, v in P.items())
    feat, logits = forward(leaves, img, cfg, dt)
    loss = F.mse_loss(logits, target)
    loss.backward()
    return feat.detach(), logits.detach(), loss.detach(), OrderedDict((k, v.grad) for k, v in leaves.items())


# ------------------------------------------------------------------------------------------------ per-element bound of the depthwise convolution
U32 = 2.0 ** -24


def gamma_n(n):
    """n fp32 roundings in any order: |computed - exact| <= gamma_n * sum |terms| (Higham, Accuracy and Stability, section 3.1)"""
    return n * U32 / (1.0 - n * U32)


def dwconv_ref64(x, wt, bias):
    """(z, sum |terms|) in float64 for channels-last x [B, H, W, C], wt [C, 7, 7], bias [C] or None"""
    C = x.shape[-1]
    xd, wd = x.double().permute(0, 3, 1, 2), wt.double().view(C, 1, 7, 7)
    z = F.conv2d(xd, wd, None if bias is None else bias.double(), padding=3, groups=C)
    m = F.conv2d(xd.abs(), wd.abs(), None if bias is None else bias.double().abs(), padding=3, groups=C)
    return z.permute(0, 2, 3, 1).contiguous(), m.permute(0, 2, 3, 1).contiguous()


def dwconv_bound(mag):
    """the issue's per-element bound for the forward and the input gradient: 50 fp32 terms (49 taps + bias / residual gradient) in any order"""
    return gamma_n(50) * mag


# ------------------------------------------------------------------------------------------------ launch plans of csrc/convnext.hip, restated
DW_TH, DW_TW, DW_CB = 8, 16, 32          # output pixels per tile, channels per tile
WGRAD_CAP = 1024                         # workgroups of dwconv7_wgrad_kernel over all channel blocks: G <= 1024 / cblocks
LS_CAP = 1024                            # ... and of layer_scale_bwd_kernel: G <= 1024 / ncb
# shapes at which a workgroup of those kernels makes a second trip (tests/test_cpu_slivit.py compares the constants with the source and
# the plans with these numbers; tests/test_gpu_slivit_kernels.py runs them): (B, H, W, C) -> (ntiles, cblocks, G), (M, C) -> (CVB, RP, ncb, G)
DW_TRIP_SHAPES = ((2, 33, 100, 512), (3, 48, 112, 264))
DW_TRIP_PLANS = ((70, 16, 64), (126, 9, 113))
LS_TRIP_SHAPE = (2 * 1024 * 128 + 77, 8)
LS_TRIP_PLAN = (2, 128, 1, 1024)


def dw_wgrad_plan(B, H, W, C):
    """(ntiles, cblocks, G): workgroup g of each channel block walks the tiles g, g + G, ... and leaves one partial of 50 x C floats"""
    ntiles = B * (-(-H // DW_TH)) * (-(-W // DW_TW))
    cblocks = -(-C // DW_CB)
    return ntiles, cblocks, min(ntiles, max(1, WGRAD_CAP // cblocks))


def ls_bwd_plan(M, C):
    """(CVB, RP, ncb, G): a workgroup is RP rows x CVB channel vectors; workgroup g walks the rows g RP + part, + G RP, ..."""
    CV = C // 4
    CVB = min(CV, 256)
    RP = 256 // CVB
    ncb = -(-CV // CVB)
    return CVB, RP, ncb, min(-(-M // RP), max(1, LS_CAP // ncb))


# ---- the layer-scale gamma gradient, exactly: a dyadic family (as the retrieval tests' one) and the walk that visits the rows
def ls_dyadic_problem(M, C, seed):
    """dout, branch [M, C] with entries in {-2 .. 2} / 4 and an earlier gradient gg0 [C] in multiples of 1/16 below 64; gamma U(0.5, 1.5).
    Every product dout * branch is a multiple of 1/16 of size <= 1/4 and every partial sum of up to 2^20 of them, with gg0, stays below
    2^18 in multiples of 1/16: exact in fp32 whatever the order, fused or not.  The gamma gradient is then ONE number, and each trip of
    each workgroup, each of the RP row parts and each of the G partials has to arrive in it."""
    g = torch.Generator().manual_seed(seed)
    dout = torch.randint(-2, 3, (M, C), generator=g).float() / 4
    branch = torch.randint(-2, 3, (M, C), generator=g).float() / 4
    gg0 = torch.randint(-1000, 1001, (C,), generator=g).float() / 16
    gamma = torch.rand((C,), generator=g) + 0.5
    assert M <= 2 ** 20
    return dout, branch, gamma, gg0


def ls_bwd_walk_sum(dout, branch, fault=None):
    """The column sums of dout * branch (float64, exact for the dyadic family) as layer_scale_bwd_kernel's walk collects them: row r
    belongs to part r % RP of workgroup (r // RP) % G on its trip (r // RP) // G.  fault in {None, "restart", "drop_trip", "fold"}: the
    accumulator starts again at every trip (only a thread's last trip survives), workgroup 5 loses its second trip, the fold of the RP
    parts stops one part short."""
    M, C = dout.shape
    CVB, RP, ncb, G = ls_bwd_plan(M, C)
    r = torch.arange(M)
    part, grp, trip = r % RP, (r // RP) % G, (r // RP) // G
    keep = torch.ones(M, dtype=torch.bool)
    if fault == "restart":
        last = (M - 1 - (grp * RP + part)) // (G * RP)          # the last trip of the thread that owns the row
        keep = trip == last
    elif fault == "drop_trip":
        keep = ~((grp == 5) & (trip == 1))
    elif fault == "fold":
        keep = part != RP - 1 if RP > 1 else keep
    else:
        assert fault is None
    return (dout.double() * branch.double())[keep].sum(0)
