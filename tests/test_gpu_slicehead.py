"""GPU: the slice-pooling kernels (csrc/pool.hip through ops.SlicePoolFn) against an fp32 torch composition, and the RETFound-all
model (models_vit_3dhead) / the 2-D flash ViT (models_vit_flash_attn) against the reference fixture and the CPU oracle.

Tolerances: the pooling kernels are fp32 end to end: out / dx / dgamma / dbeta <= 1e-5 relative (L2) against a float64 composition,
bit-identical across two calls, exact zeros on the tokens that are not pooled.  Models (bf16 GEMM / attention operands): the
bounds of test_gpu_coem.py::test_vit2d_tower_vs_reference_golden (output 1e-2, loss 1e-2, gradients 5e-2); the fine-tune loop
the bounds of test_gpu_finetune.py::test_finetune_loop_matches_reference_trajectory."""
import json
import os
import warnings
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import engine_finetune, lr_decay, lr_sched, misc, models_vit_3dhead, models_vit_flash_attn, ops
    from octcubem_amd import optim as foptim
from oracle import vit_ref as V
from tests import slicehead_ref as R

DEV = "cuda"


def rel(a, b):
    a = torch.as_tensor(a).detach().double().flatten().cpu(); b = torch.as_tensor(b).detach().double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ---------------------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def _pool_ref(x, g, b, eps, S, cls):
    D = x.shape[-1]
    p = x[:, 0] if cls else x[:, 1:].mean(dim=1)
    return torch.nn.functional.layer_norm(p, (D,), g, b, eps).view(-1, S, D).mean(dim=1)


def _run_pool(x, g, b, S, cls, dout):
    xg = x.clone().requires_grad_(True)
    gp, bp = torch.nn.Parameter(g.clone()), torch.nn.Parameter(b.clone())
    out = ops.SlicePoolFn.apply(xg, gp, bp, 1e-6, S, cls)
    out.backward(dout)
    torch.cuda.synchronize()
    return out.detach(), xg.grad, gp.grad, bp.grad


SHAPES = [(1, 197, 1024), (18, 197, 1024), (24, 197, 1024), (24, 257, 1024), (4, 17, 128), (3, 5, 64)]


@pytest.mark.parametrize("cls", [False, True], ids=["mean", "cls"])
@pytest.mark.parametrize("S,T,D", SHAPES)
@pytest.mark.parametrize("B", [1, 2, 8])
def test_slice_pool_kernels_vs_fp32_composition(B, S, T, D, cls):
    gen = torch.Generator(device=DEV).manual_seed(B * 1000 + S * 10 + T + D + int(cls))
    x = torch.randn(B * S, T, D, device=DEV, generator=gen) * 2 + 0.5
    g = 1 + 0.1 * torch.randn(D, device=DEV, generator=gen)
    b = 0.1 * torch.randn(D, device=DEV, generator=gen)
    dout = torch.randn(B, D, device=DEV, generator=gen)
    out, dx, dg, db = _run_pool(x, g, b, S, cls, dout)
    xd, gd, bd = x.double().requires_grad_(True), g.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = _pool_ref(xd, gd, bd, 1e-6, S, cls)
    ref.backward(dout.double())
    assert rel(out, ref) <= 1e-5
    assert rel(dx, xd.grad) <= 1e-5
    assert rel(dg, gd.grad) <= 1e-5
    assert rel(db, bd.grad) <= 1e-5
    # the tokens that are not pooled receive exact zeros
    if cls:
        assert int(torch.count_nonzero(dx[:, 1:])) == 0
    else:
        assert int(torch.count_nonzero(dx[:, 0])) == 0
    # deterministic: a second call is bit-identical
    out2, dx2, dg2, db2 = _run_pool(x, g, b, S, cls, dout)
    assert torch.equal(out, out2) and torch.equal(dx, dx2) and torch.equal(dg, dg2) and torch.equal(db, db2)


def test_slice_pool_sidecar_matches_its_gradient():
    """The 16-bit copy and column sums the backward leaves for the producing Block are those of the dx it returns."""
    B, S, T, D = 2, 4, 17, 128
    x = torch.randn(B * S, T, D, device=DEV, requires_grad=True)
    g, b = torch.nn.Parameter(torch.ones(D, device=DEV)), torch.nn.Parameter(torch.zeros(D, device=DEV))
    seen = {}
    orig = ops._sidecar_put

    def spy(dx, dxb, colsum):
        seen["v"] = (dx, dxb, colsum.clone())
        orig(dx, dxb, colsum)
    ops._sidecar_put = spy
    try:
        ops.SlicePoolFn.apply(x, g, b, 1e-6, S, False).backward(torch.randn(B, D, device=DEV))
    finally:
        ops._sidecar_put = orig
    dx, dxb, colsum = seen["v"]
    assert torch.equal(dxb, dx.to(ops.BF16)) and dxb.shape == dx.shape
    assert rel(colsum, dx.double().sum(dim=(0, 1))) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------------------
def small_model(cfg, flash, P=None, **kw):
    m = models_vit_3dhead.VisionTransformerWith3DPoolingHead(
        img_size=cfg.img_size, patch_size=cfg.patch_size, in_chans=cfg.in_chans, num_classes=cfg.num_classes, embed_dim=cfg.embed_dim,
        depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=4, qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
        global_pool=cfg.global_pool, use_flash_attn=flash, **kw)
    if P is not None:
        m.load_state_dict(P, strict=True)
    return m.to(DEV)


def _grads_vs(m, ref_grads, ref_norms, keys, bound=5e-2):
    total = float(np.sqrt(sum(float(v) ** 2 for v in ref_norms.values())))
    named = dict(m.named_parameters())
    for k in keys:
        if float(ref_norms[k]) < 1e-3 * total:
            continue
        ref = torch.as_tensor(ref_grads[k])
        mine = R.sub(named[k].grad.detach().cpu())
        assert rel(mine, ref) <= bound, (k, rel(mine, ref))


@pytest.mark.parametrize("tag", ["gp1", "gp0"])
def test_slicehead_timm_vs_reference_golden(golden_dir, tag):
    z = np.load(os.path.join(golden_dir, "slicehead_small.npz"))
    cfg = V.ViT2DConfig(**json.loads(str(z[f"{tag}/cfg"])))
    m = small_model(cfg, False, R.init(cfg, seed=int(z["param_seed"]))).eval()
    x, tgt = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["target"]).to(DEV)
    feats = m.forward_features(x)
    assert rel(feats, z[f"{tag}/features"]) <= 1e-2
    out = m(x)
    assert rel(out, z[f"{tag}/out"]) <= 1e-2
    loss = torch.nn.functional.cross_entropy(out.float(), tgt)
    assert abs(float(loss) - float(z[f"{tag}/loss"])) <= 1e-2 * float(z[f"{tag}/loss"])
    loss.backward()
    keys = R.grad_keys(cfg)
    _grads_vs(m, {k: z[f"{tag}/grad/{k}"] for k in keys}, {k: z[f"{tag}/gnorm/{k}"] for k in keys}, keys)


def _oracle_grads(P, x, tgt, cfg, flash):
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    out, feats = R.forward(Pg, x, cfg, flash=flash)
    loss = torch.nn.functional.cross_entropy(out, tgt)
    loss.backward()
    return out.detach(), feats.detach(), loss.detach(), {k: R.sub(v.grad) for k, v in Pg.items()}, \
        {k: float(v.grad.double().norm()) for k, v in Pg.items()}


@pytest.mark.parametrize("gp", [True, False])
def test_slicehead_flash_vs_oracle(gp):
    cfg = R.config(gp)
    P = R.init(cfg)
    x, tgt = R.inputs(cfg)
    out_r, feats_r, loss_r, G, N = _oracle_grads(P, x, tgt, cfg, flash=True)
    m = small_model(cfg, True, P).eval()
    assert m.flash_compat
    out = m(x.to(DEV))
    assert rel(out, out_r) <= 1e-2
    assert rel(m.forward_features(x.to(DEV)), feats_r) <= 1e-2
    loss = torch.nn.functional.cross_entropy(out.float(), tgt.to(DEV))
    assert abs(float(loss) - float(loss_r)) <= 1e-2 * float(loss_r)
    loss.backward()
    _grads_vs(m, G, N, list(P))


def test_center2d_flash_model_vs_oracle_and_hidden_states():
    cfg = V.ViT2DConfig(**{**R.SMALL, "num_classes": 16, "global_pool": True})
    P = V.init_from_shapes(V.vit2d_param_shapes(cfg), seed=81)
    x = torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(82))
    ref_tok = R.slice_tokens(P, x.unsqueeze(1), cfg, flash=True)
    f = R.slice_pool(ref_tok, P, cfg, 1)
    ref = torch.nn.functional.linear(f, P["head.weight"], P["head.bias"])
    kw = dict(img_size=64, patch_size=16, in_chans=3, num_classes=16, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4,
              qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), global_pool=True)
    m = models_vit_flash_attn.VisionTransformer(**kw)
    m.load_state_dict(P, strict=True)
    m = m.to(DEV).eval()
    assert m.flash_compat and not m.fused_pool
    out = m(x.to(DEV))
    assert rel(out, ref) <= 1e-2
    mf = models_vit_flash_attn.VisionTransformer(fused_pool=True, **kw)
    mf.load_state_dict(P, strict=True)
    assert rel(mf.to(DEV).eval()(x.to(DEV)), ref) <= 1e-2
    hs = m(x.to(DEV), hidden_states=True)
    assert isinstance(hs, list) and len(hs) == cfg.depth
    assert all(tuple(h.shape) == (3, 17, 128) for h in hs)
    assert rel(hs[-1], ref_tok) <= 1e-2                     # the last entry is the MLP branch alone (flash semantics)
    # without flash_compat the last block keeps its residual: a different model
    mt = models_vit_flash_attn.VisionTransformer(use_flash_attn=False, **kw)
    mt.load_state_dict(P, strict=True)
    assert rel(mt.to(DEV).eval()(x.to(DEV)), V.vit2d_forward(P, x, cfg)) <= 1e-2


@pytest.mark.parametrize("ctx", ["fp16", "bf16"])
def test_slicehead_autocast_invariant(ctx):
    cfg = R.config(True, num_classes=8)
    P = R.init(cfg)
    x, _ = R.inputs(cfg)
    x = x.to(DEV)

    def run(ac):
        m = small_model(cfg, True, P)
        if ac is None:
            out = m(x)
        else:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                with ac():
                    out = m(x)
        (out.float() ** 2).sum().backward()
        torch.cuda.synchronize()
        return out.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    o0, g0 = run(None)
    o1, g1 = run(torch.cuda.amp.autocast if ctx == "fp16" else (lambda: torch.autocast("cuda", dtype=torch.bfloat16)))
    assert o1.dtype == o0.dtype and torch.equal(o0, o1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


class Args:
    accum_iter = 1; lr = 5e-4; min_lr = 1e-6; warmup_epochs = 0; epochs = 4; task_mode = "multi_cls"


def test_finetune_loop_follows_cpu_trajectory():
    """Three train_one_epoch steps (AdamW, layer decay 0.65, clip 1.0) against an fp32 CPU trajectory: the oracle composition +
    torch.optim.AdamW over the same param_groups_lrd groups, driven through the same LR schedule."""
    cfg = R.config(True)
    P0 = R.init(cfg)
    g = torch.Generator().manual_seed(91)
    xs = torch.randn(3, 2, 4, 3, 64, 64, generator=g)
    ts = torch.randint(0, 3, (3, 2), generator=g)
    m = small_model(cfg, True, P0, drop_path_rate=0.0, dropout=0.0)
    groups = lr_decay.param_groups_lrd(m, 0.05, no_weight_decay_list=m.no_weight_decay(), layer_decay=0.65)
    opt = foptim.FusedAdamW(groups, lr=Args.lr)
    scaler = misc.NativeScalerWithGradNormCount()
    losses = []

    def crit(o, t):
        l = torch.nn.functional.cross_entropy(o, t)
        losses.append(float(l.detach()))
        return l
    loader = [(xs[i], ts[i]) for i in range(3)]
    stats = engine_finetune.train_one_epoch(m, crit, loader, opt, torch.device(DEV), 0, scaler, 1.0, None, None, Args)
    assert stats is not None
    # CPU trajectory
    name_of = {id(p): n for n, p in m.named_parameters()}
    Pc = {k: v.clone().requires_grad_(True) for k, v in P0.items()}
    cgroups = [{"lr_scale": gr["lr_scale"], "weight_decay": gr["weight_decay"], "params": [Pc[name_of[id(p)]] for p in gr["params"]]}
               for gr in groups]
    copt = torch.optim.AdamW(cgroups, lr=Args.lr)
    closses = []
    for i in range(3):
        lr_sched.adjust_learning_rate(copt, i / 3, Args)
        out, _ = R.forward(Pc, xs[i], cfg, flash=True)
        loss = torch.nn.functional.cross_entropy(out, ts[i])
        closses.append(float(loss))
        copt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(Pc.values()), 1.0)
        copt.step()
    np.testing.assert_allclose(losses, closses, rtol=3e-2)
    max_step = Args.lr * 3
    sd = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    for n, ref in Pc.items():
        ref, mine, init = ref.detach().flatten(), sd[n].flatten(), P0[n].flatten()
        if n.endswith("attn.qkv.bias"):      # d loss / d k-bias == 0 exactly (softmax is shift-invariant): that third steps along
            D = cfg.embed_dim                 # rounding noise in both runs (test_gpu_finetune.py skips attn.k.bias for the same reason)
            keep = torch.cat([torch.arange(D), torch.arange(2 * D, 3 * D)])
            ref, mine, init = ref[keep], mine[keep], init[keep]
        du_ref, du = (ref - init).double(), (mine - init).double()
        assert float((mine - ref).abs().max()) <= 2.5 * max_step, (n, float((mine - ref).abs().max()))
        if float(du_ref.norm()) > 1e-9:
            cos = float((du * du_ref).sum() / (du.norm() * du_ref.norm() + 1e-30))
            assert cos >= 0.98, (n, cos)


def test_vitl_24_slices_forward_pin():
    """ViT-L at 224 x 224, one volume of 24 slices (N = 197 at full width): the token streams of three slices against the CPU
    oracle, and the pooled head on the GPU's own tokens against an fp64 composition."""
    cfg = V.ViT2DConfig(img_size=224, patch_size=16, in_chans=3, num_classes=3, embed_dim=1024, depth=24, num_heads=16, global_pool=True)
    P = R.init(cfg, seed=93)
    x = torch.randn(1, 24, 3, 224, 224, generator=torch.Generator().manual_seed(94))
    m = models_vit_3dhead.flash_attn_vit_large_patch16_3DSliceHead(img_size=224, num_classes=3, global_pool=True)
    m.load_state_dict(P, strict=True)
    m = m.to(DEV).eval()
    with torch.no_grad():
        tok = m._tokens(x.view(24, 3, 224, 224).to(DEV))
        out = m(x.to(DEV))
    idx = [0, 11, 23]
    ref_tok = R.slice_tokens(P, x[:, idx], cfg, flash=True)
    for j, i in enumerate(idx):
        assert rel(tok[i], ref_tok[j]) <= 2e-2, (i, rel(tok[i], ref_tok[j]))
    Pd = {k: v.double() for k, v in P.items()}
    f = R.slice_pool(tok.double().cpu(), Pd, cfg, 24)
    f = torch.nn.functional.linear(f, Pd["fc_aggregate_cls.weight"], Pd["fc_aggregate_cls.bias"])
    f = torch.nn.functional.layer_norm(f, (1024,), Pd["aggregate_cls_norm.weight"], Pd["aggregate_cls_norm.bias"], 1e-6)
    ref = torch.nn.functional.linear(f, Pd["head.weight"], Pd["head.bias"])
    assert rel(out, ref) <= 1e-2
