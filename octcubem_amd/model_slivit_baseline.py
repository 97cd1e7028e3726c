"""SLIViT baseline (``patient_dataset_type`` ``convnext_slivit``): drop-in for the reference's ``OCTCube/model_slivit_baseline.py`` --
``SLIViT`` (:18-49), ``get_feature_extractor`` (:72-85), ``get_slivit_model`` (:88-93) -- a ConvNeXt-T feature extractor over the slices
of a volume laid side by side, and a small ViT over the feature map cut into one "patch" per slice.

``ConvNextFeatureExtractor`` is HF ``ConvNextModel``'s ``embeddings`` + ``encoder`` without the model's pooled LayerNorm -- what the
reference keeps as ``Sequential(*children[:2])`` and reads through ``.last_hidden_state`` -- under the same state-dict keys
(``0.patch_embeddings.*``, ``0.layernorm.*``, ``1.stages.{s}.downsampling_layer.{0,1}.*``, ``1.stages.{s}.layers.{l}.*``).  The residual
stream is channels-last fp32 ``[B, H, W, C]``: every ConvNeXt layer is one ``ops.ConvNextLayerFn`` (HIP depthwise convolution and layer
scale around the package's LayerNorm and GEMM kernels); the stem and the three downsampling convolutions are kernel = stride
patchifies, an ATen view / permute / contiguous in front of the GEMM (ops.patch_gather moves 8-wide patches; these are 4 and 2 wide);
the channels-first LayerNorms are the row LayerNorm in this layout.  The module returns fp32 NCHW ``[B, C4, H / 32, W / 32]`` because the
head reshapes that memory flat.

``SLIViT`` restates vit-pytorch's ``ViT`` (the 1.x layout: ``to_patch_embedding.{1,2,3}``, ``cls_token``, ``pos_embedding``,
``transformer.layers.{i}.0.{norm,to_qkv,to_out.0}``, ``transformer.layers.{i}.1.net.{0,1,4}``, ``transformer.norm``, ``mlp_head``) as the
reference subclasses it; the package is not a dependency.  Its attention has ``heads * dim_head != dim`` (20 x 64 over 256), so it is
an autograd function of its own (``HeadAttentionFn``) over the same GEMM and attention kernels.  Two LayerNorms stay in ATen: the one
over the ``patch_height * patch_width`` = 49152 columns of a slice (beyond the row kernel's 2048; B * P rows) and the one after the
patch projection, whose output is the fp32 residual stream and not a 16-bit GEMM operand; so do the cls / positional assembly and a
class head that is not a multiple of 8 wide.

Departures from the reference, on purpose: nothing is ever fetched (the reference downloads ``facebook/convnext-tiny-224`` from the hub
before it loads ``pretrained_weights``; here the extractor is initialised as HF initialises it, or loaded from the given file);
dropout, embedding dropout and drop-path must be 0 (the reference never sets them); GPU only."""
from __future__ import annotations

from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .arena import get_arena
from .video_vit import layer_norm
from ._autocast import autocast_invariant


# ------------------------------------------------------------------------------------------------
# ConvNeXt feature extractor
# ------------------------------------------------------------------------------------------------
class ConvNextLayer(nn.Module):
    """HF ConvNextLayer: dwconv 7x7 -> LayerNorm -> pwconv1 -> GELU -> pwconv2 -> layer scale -> + residual (drop-path 0)."""

    def __init__(self, dim: int, layer_scale_init_value: float = 1e-6):
        super().__init__()
        if dim % 8:
            raise ValueError(f"ConvNextLayer: dim = {dim} is not a multiple of 8")
        self.dwconv = nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.layernorm = nn.LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.pwconv2 = nn.Linear(4 * dim, dim)
        self.layer_scale_parameter = nn.Parameter(layer_scale_init_value * torch.ones(dim))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """fp32 channels-last [B, H, W, C] -> the same."""
        a = get_arena(self)
        ps = (self.dwconv.weight, self.dwconv.bias, self.layernorm.weight, self.layernorm.bias, self.pwconv1.weight, self.pwconv1.bias,
              self.pwconv2.weight, self.pwconv2.bias, self.layer_scale_parameter)
        C = self.layer_scale_parameter.numel()
        views = (a.f32_view(self.dwconv.weight, shape=(C, 7, 7)), a.f32_view(self.dwconv.bias), a.f32_view(self.layernorm.weight),
                 a.f32_view(self.layernorm.bias), a.f32_view(self.layer_scale_parameter))

        def grads():
            return (a.grad_view(ps[0], shape=(C, 7, 7)),) + tuple(a.grad_view(p) for p in ps[1:])

        return ops.ConvNextLayerFn.apply(x, views, a.lp_view(self.pwconv1.weight), a.f32_view(self.pwconv1.bias),
                                         a.lp_view(self.pwconv2.weight), a.f32_view(self.pwconv2.bias), grads, self.layernorm.eps, *ps)


def _patchify_linear(module: nn.Module, conv: nn.Conv2d, rows: torch.Tensor) -> torch.Tensor:
    """A kernel = stride convolution over gathered patches ``rows`` [M, Cin * k * k] (columns in the weight's (c, kh, kw) order): the
    GEMM with an fp32 output, its gradients through ops.LinearFn."""
    a = get_arena(module)
    n = conv.weight.shape[0]
    return ops.LinearFn.apply(rows, a.lp_view(conv.weight, shape=(n, rows.shape[1])), a.f32_view(conv.bias),
                              lambda: a.grad_view(conv.weight, shape=(n, rows.shape[1])), lambda: a.grad_view(conv.bias), True,
                              conv.weight, conv.bias)


class ConvNextEmbeddings(nn.Module):
    def __init__(self, num_channels: int, dim: int, patch_size: int):
        super().__init__()
        self.patch_embeddings = nn.Conv2d(num_channels, dim, kernel_size=patch_size, stride=patch_size)
        self.layernorm = nn.LayerNorm(dim, eps=1e-6)          # HF: channels_first; the row LayerNorm in the channels-last layout
        self.patch_size = patch_size

    def forward(self, img: torch.Tensor) -> torch.Tensor:
        """fp32 NCHW image -> the 16-bit channels-last map [B, H / p, W / p, dim] AFTER the LayerNorm, widened to fp32 (the residual stream)."""
        B, Cin, H, W = img.shape
        p = self.patch_size
        rows = img.view(B, Cin, H // p, p, W // p, p).permute(0, 2, 4, 1, 3, 5).reshape(B * (H // p) * (W // p), Cin * p * p)
        k = rows.shape[1]
        if k % 8:                                             # the GEMM reads k in whole 8-element pieces (3 x 4 x 4 = 48 is six of them)
            raise ValueError(f"patch embedding: {Cin} channels x {p} x {p} = {k} columns is not a multiple of 8")
        tok = _patchify_linear(self, self.patch_embeddings, rows)
        return layer_norm(self.layernorm, tok).float().view(B, H // p, W // p, -1)


class ConvNextStage(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, stride: int, depth: int, layer_scale_init_value: float):
        super().__init__()
        if in_channels != out_channels or stride > 1:
            self.downsampling_layer = nn.ModuleList([nn.LayerNorm(in_channels, eps=1e-6),
                                                     nn.Conv2d(in_channels, out_channels, kernel_size=2, stride=2)])
        else:
            self.downsampling_layer = nn.ModuleList()
        self.layers = nn.ModuleList([ConvNextLayer(out_channels, layer_scale_init_value) for _ in range(depth)])

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if len(self.downsampling_layer):
            norm, conv = self.downsampling_layer
            B, H, W, C = x.shape
            y = layer_norm(norm, x)                           # 16-bit [B, H, W, C]: the GEMM operand once gathered
            rows = y.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B * (H // 2) * (W // 2), C * 4)
            x = _patchify_linear(self, conv, rows).view(B, H // 2, W // 2, -1)
        for layer in self.layers:
            x = layer(x)
        return x


class ConvNextEncoder(nn.Module):
    def __init__(self, depths, hidden_sizes, layer_scale_init_value: float):
        super().__init__()
        self.stages = nn.ModuleList()
        prev = hidden_sizes[0]
        for i, (d, c) in enumerate(zip(depths, hidden_sizes)):
            self.stages.append(ConvNextStage(prev, c, 2 if i > 0 else 1, d, layer_scale_init_value))
            prev = c

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        for stage in self.stages:
            x = stage(x)
        return x


def _hf_init(module: nn.Module, std: float = 0.02, layer_scale_init_value: float = 1e-6):
    """HF ConvNextPreTrainedModel._init_weights: normal(0, 0.02) weights, zero biases, LayerNorm ones / zeros, layer scale constant."""
    for m in module.modules():
        if isinstance(m, (nn.Linear, nn.Conv2d)):
            nn.init.normal_(m.weight, mean=0.0, std=std)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, nn.LayerNorm):
            nn.init.ones_(m.weight)
            nn.init.zeros_(m.bias)
        elif isinstance(m, ConvNextLayer):
            nn.init.constant_(m.layer_scale_parameter, layer_scale_init_value)


class _ArenaModel(nn.Module):
    def prepare(self):
        arena = get_arena(self, full_check=True)
        if torch.is_grad_enabled():
            arena.rebind_grads()
        arena.refresh_lp()
        return arena

    @property
    def arena(self):
        return get_arena(self, full_check=True)

    def invalidate_lp(self):
        """Call after writing weights behind PyTorch's version counters."""
        self.arena.invalidate_lp()


@autocast_invariant
class ConvNextFeatureExtractor(nn.Sequential, _ArenaModel):
    """HF ConvNextModel's ``embeddings`` (index 0) and ``encoder`` (index 1).  fp32 NCHW [B, 3, H, W], H and W multiples of 32 ->
    fp32 NCHW [B, hidden_sizes[-1], H / 32, W / 32]."""

    def __init__(self, depths=(3, 3, 9, 3), hidden_sizes=(96, 192, 384, 768), num_channels: int = 3, patch_size: int = 4,
                 layer_scale_init_value: float = 1e-6, drop_path_rate: float = 0.0):
        assert drop_path_rate == 0, "drop-path inside ConvNeXt is not built (the reference never sets it)"
        assert len(depths) == len(hidden_sizes) == 4
        super().__init__(ConvNextEmbeddings(num_channels, hidden_sizes[0], patch_size),
                         ConvNextEncoder(tuple(depths), tuple(hidden_sizes), layer_scale_init_value))
        self.depths, self.hidden_sizes = tuple(depths), tuple(hidden_sizes)
        self.reduction = patch_size * 8
        _hf_init(self, layer_scale_init_value=layer_scale_init_value)

    def features(self, img: torch.Tensor) -> torch.Tensor:
        """The forward without ``prepare()``: for a model that owns this one and has prepared the shared arena itself."""
        assert img.dim() == 4 and img.shape[2] % self.reduction == 0 and img.shape[3] % self.reduction == 0, \
            f"ConvNextFeatureExtractor: H and W must be multiples of {self.reduction}, got {tuple(img.shape)}"
        x = self[1](self[0](img.float().contiguous()))
        return x.permute(0, 3, 1, 2).contiguous()

    def forward(self, img: torch.Tensor) -> torch.Tensor:
        self.prepare()
        return self.features(img)


def map_pretrained_keys(state_dict) -> "OrderedDict[str, torch.Tensor]":
    """A ``CustomHuggingFaceModel`` state dict (``model.convnext.embeddings.*``, ``model.convnext.encoder.*``, ``model.convnext.layernorm.*``,
    ``model.classifier.*``) -> the extractor's keys (``0.*``, ``1.*``); the pooled LayerNorm and the classifier are dropped, as the
    reference drops them with ``children()[:2]``.  Any other key raises."""
    out = OrderedDict()
    for k, v in state_dict.items():
        if k.startswith("model.convnext.embeddings."):
            out["0." + k[len("model.convnext.embeddings."):]] = v
        elif k.startswith("model.convnext.encoder."):
            out["1." + k[len("model.convnext.encoder."):]] = v
        elif k.startswith(("model.convnext.layernorm.", "model.classifier.")):
            continue
        else:
            raise KeyError(f"get_feature_extractor: unexpected key {k!r} in the pretrained weights")
    return out


def get_feature_extractor(num_labels, pretrained_weights="", **kwargs) -> ConvNextFeatureExtractor:
    """The reference's call (model_slivit_baseline.py:72-85).  ``num_labels`` sizes the classifier the reference builds and then drops:
    unused.  Nothing is downloaded: without ``pretrained_weights`` the extractor keeps HF's initialisation."""
    fe = ConvNextFeatureExtractor(**kwargs)
    if pretrained_weights:
        sd = torch.load(pretrained_weights, map_location="cpu")
        fe.load_state_dict(map_pretrained_keys(sd), strict=True)
    return fe


# ------------------------------------------------------------------------------------------------
# the ViT on top
# ------------------------------------------------------------------------------------------------
class _GatedParamFn(torch.autograd.Function):
    """A parameter on its way into one of the ATen islands of the head: the identity, whose backward hands the gradient on only while
    ``ops.weight_grads`` is on (read when the backward runs, as every Function of ops.py reads it)."""

    @staticmethod
    def forward(ctx, p):
        return p.view_as(p)

    @staticmethod
    def backward(ctx, g):
        return g if ops.weight_grads_enabled() else None


def _gp(p):
    return _GatedParamFn.apply(p) if p.requires_grad and torch.is_grad_enabled() else p


class HeadAttentionFn(torch.autograd.Function):
    """vit-pytorch's Attention behind its LayerNorm: to_qkv (no bias) -> softmax(q k^T * dim_head^-0.5) v -> to_out.0, the residual added
    in that GEMM's epilogue.  ``heads * dim_head`` need not equal the model width.  y: 16-bit [B, N, D]; res: fp32 [B, N, D]."""

    @staticmethod
    def forward(ctx, y, res, wqkv_lp, wout_lp, bout32, grads, H, HD, *params):
        Bn, N, D = y.shape
        scale = HD ** -0.5
        y2 = ops.cast_bf16(y.reshape(-1, D))
        qkv = ops.linear_fwd(y2, wqkv_lp, None, "bf16")
        o, lse = ops.attn_fwd(qkv, Bn, N, H, HD, scale)
        out = ops.linear_fwd(o, wout_lp, bout32, "resid", res=ops._chk(res.reshape(-1, D), ops.F32, "residual"))
        ctx.save_for_backward(y2, qkv, o, lse, wqkv_lp, wout_lp)
        ctx.meta = (Bn, N, H, HD, scale, D)
        ctx.grads, ctx.params = grads, params
        return out.view(Bn, N, D)

    @staticmethod
    def backward(ctx, dout):
        y2, qkv, o, lse, wqkv_lp, wout_lp = ctx.saved_tensors
        Bn, N, H, HD, scale, D = ctx.meta
        wg = ops.weight_grads_enabled()
        gwqkv, gwout, gbout = ctx.grads() if wg else (None,) * 3
        d2 = dout.reshape(-1, D)
        if not d2.is_contiguous():
            d2 = d2.contiguous()
        dob = ops.cast_bf16(d2)
        if wg:
            ops.colsum_accum(d2, gbout)
            ops.linear_wgrad_accum(dob, o, gwout)
        do = ops.linear_dgrad(dob, wout_lp)
        dqkv = ops.attn_bwd(qkv, o, do, lse, Bn, N, H, HD, scale)
        if wg:
            ops.linear_wgrad_accum(dqkv, y2, gwqkv)
            ops.notify_grad_ready(ctx.params)
        dy = ops.linear_dgrad(dqkv, wqkv_lp).view(Bn, N, D)
        return (dy, dout) + (None,) * (6 + len(ctx.params))


class _Attention(nn.Module):
    def __init__(self, dim, heads, dim_head):
        super().__init__()
        inner = heads * dim_head
        if dim_head not in (32, 64):
            raise ValueError(f"dim_head = {dim_head}: the attention kernels are built for 32 and 64")
        self.heads, self.dim_head = heads, dim_head
        self.norm = nn.LayerNorm(dim)
        self.to_qkv = nn.Linear(dim, inner * 3, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner, dim))       # vit-pytorch: Sequential(Linear, Dropout); the Dropout has no state

    def forward(self, x):
        a = get_arena(self)
        out = self.to_out[0]
        ps = (self.to_qkv.weight, out.weight, out.bias)
        return HeadAttentionFn.apply(layer_norm(self.norm, x), x, a.lp_view(self.to_qkv.weight), a.lp_view(out.weight), a.f32_view(out.bias),
                                     lambda: tuple(a.grad_view(p) for p in ps), self.heads, self.dim_head, *ps)


class _FeedForward(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        # vit-pytorch: Sequential(LayerNorm, Linear, GELU, Dropout, Linear, Dropout): indices 0, 1 and 4 hold parameters
        self.net = nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, hidden), nn.GELU(), nn.Identity(), nn.Linear(hidden, dim), nn.Identity())

    def forward(self, x):
        a = get_arena(self)
        fc1, fc2 = self.net[1], self.net[4]
        ps = (fc1.weight, fc1.bias, fc2.weight, fc2.bias)
        return ops.MlpFn.apply(layer_norm(self.net[0], x), x, a.lp_view(fc1.weight), a.f32_view(fc1.bias), a.lp_view(fc2.weight),
                               a.f32_view(fc2.bias), lambda: tuple(a.grad_view(p) for p in ps), *ps)


class _Transformer(nn.Module):
    def __init__(self, dim, depth, heads, dim_head, mlp_dim):
        super().__init__()
        self.norm = nn.LayerNorm(dim)
        self.layers = nn.ModuleList([nn.ModuleList([_Attention(dim, heads, dim_head), _FeedForward(dim, mlp_dim)]) for _ in range(depth)])


@autocast_invariant
class SLIViT(_ArenaModel):
    """The reference's SLIViT(ViT) (model_slivit_baseline.py:18-49; vit-pytorch 1.x ``ViT`` restated)."""

    def __init__(self, *, feature_extractor, vit_dim, vit_depth, heads, mlp_dim, num_of_patches, dropout=0., emb_dropout=0., patch_height=768,
                 patch_width=64, rnd_pos_emb=False, num_classes=1, dim_head=64):
        super().__init__()
        assert dropout == 0 and emb_dropout == 0, "dropout inside the SLIViT head is not built (the reference passes 0)"
        if vit_dim % 8 or mlp_dim % 8:
            raise ValueError(f"vit_dim = {vit_dim}, mlp_dim = {mlp_dim}: GEMM operands come in multiples of 8")
        patch_dim = patch_height * patch_width
        self.to_patch_embedding = nn.Sequential(nn.Identity(), nn.LayerNorm(patch_dim), nn.Linear(patch_dim, vit_dim), nn.LayerNorm(vit_dim))
        self.pos_embedding = nn.Parameter(torch.randn(1, num_of_patches + 1, vit_dim))
        self.cls_token = nn.Parameter(torch.randn(1, 1, vit_dim))
        self.transformer = _Transformer(vit_dim, vit_depth, heads, dim_head, mlp_dim)
        self.mlp_head = nn.Linear(vit_dim, num_classes)
        self.feature_extractor = feature_extractor
        self.num_patches = num_of_patches
        self.patch_height, self.patch_width = patch_height, patch_width
        if not rnd_pos_emb:          # row i is the constant i, trainable (model_slivit_baseline.py:34-37)
            self.pos_embedding = nn.Parameter(torch.arange(self.num_patches + 1).repeat(vit_dim, 1).t().unsqueeze(0).float())

    def forward_head(self, feat: torch.Tensor) -> torch.Tensor:
        """fp32 feature map (any shape with B * P * patch_height * patch_width elements, read flat as the reference's reshape does)
        -> logits [B, num_classes]."""
        a = get_arena(self)
        Bn, P = feat.shape[0], self.num_patches
        x = feat.reshape(Bn, P, self.patch_height * self.patch_width)
        ln1, proj = self.to_patch_embedding[1], self.to_patch_embedding[2]
        x = F.layer_norm(x, ln1.normalized_shape, _gp(ln1.weight), _gp(ln1.bias), ln1.eps)
        x = ops.LinearFn.apply(x, a.lp_view(proj.weight), a.f32_view(proj.bias), lambda: a.grad_view(proj.weight),
                               lambda: a.grad_view(proj.bias), True, proj.weight, proj.bias)
        return self.forward_embedded(x)

    def forward_embedded(self, x: torch.Tensor) -> torch.Tensor:
        """The head from the patch projection's output on, fp32 [B, P, vit_dim] -> logits [B, num_classes]: what forward_head ends in,
        and what models_slivit_head.SLIViT runs behind its own patch embedding."""
        a = get_arena(self)
        Bn, P = x.shape[0], self.num_patches
        ln2 = self.to_patch_embedding[3]
        x = F.layer_norm(x, ln2.normalized_shape, _gp(ln2.weight), _gp(ln2.bias), ln2.eps)
        x = torch.cat((_gp(self.cls_token).expand(Bn, -1, -1), x), dim=1) + _gp(self.pos_embedding)[:, :P + 1]
        x = x.contiguous()
        for attn, ff in self.transformer.layers:
            x = attn(x)
            x = ff(x)
        x = layer_norm(self.transformer.norm, x[:, :1].contiguous())[:, 0]        # row-wise: the norm of the cls row alone
        head = self.mlp_head
        if head.out_features % 8 == 0:
            return ops.LinearFn.apply(x, a.lp_view(head.weight), a.f32_view(head.bias), lambda: a.grad_view(head.weight),
                                      lambda: a.grad_view(head.bias), True, head.weight, head.bias)
        return F.linear(x.float(), _gp(head.weight), _gp(head.bias))     # class counts that are no multiple of 8: see models_vit_st

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self.prepare()
        feat = self.feature_extractor.features(x)
        assert feat[0].numel() == self.num_patches * self.patch_height * self.patch_width, \
            f"SLIViT: a feature map of {tuple(feat.shape)} is not {self.num_patches} patches of {self.patch_height} x {self.patch_width}"
        return self.forward_head(feat)


def get_slivit_model(args) -> SLIViT:
    """The reference's call (model_slivit_baseline.py:88-93): ConvNeXt-T extractor from ``args.slivit_fe_path`` (may be empty), a ViT of
    width 256, depth 5, 20 heads of 64, MLP 512 over ``args.slivit_num_of_patches`` slices, ``args.nb_classes`` outputs."""
    return SLIViT(feature_extractor=get_feature_extractor(4, args.slivit_fe_path), num_classes=args.nb_classes, vit_dim=256, vit_depth=5,
                  heads=20, mlp_dim=512, num_of_patches=args.slivit_num_of_patches, dropout=0, emb_dropout=0)
