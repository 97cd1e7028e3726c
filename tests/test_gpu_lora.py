"""Low-rank adapters on the fused Block, model level -- `pytest -m gpu` on an MI355X.

Small 2-D ViTs (models_vit.VisionTransformer on TimmBlocks: width 64 and 128, two heads = head_dim 32 and 64, depth 2, 10 and 65
tokens, batch 3 and 2, ranks 4 and 16) and single Blocks of the three layouts.  What is bit-identical is asserted with torch.equal:
an adapted model against the plain model that holds merge_and_unload's weights (same operands, same launches), the three recompute
levels, two runs from one seed.  The adapter gradients are held to the CPU oracle (oracle/vit_ref.py in fp32 autograd, the weights
entering as W + s B A) with the error of the existing full weight-gradient path as the yardstick."""
import os
from functools import partial

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import checkpoint, engine_finetune, lora, lr_decay, misc, models_vit, models_vit_st, ops, video_vit
    from octcubem_amd import optim as foptim
    from octcubem_amd.arena import get_arena
from oracle import vit_ref as V
from tests.conftest import parity

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN = partial(torch.nn.LayerNorm, eps=1e-6)
CASES = [(64, 48, 3, 4), (128, 128, 2, 16)]          # (width, image side -> (side / 16)^2 + 1 tokens, batch, rank)
TIMM_KEYS = {"qkv": "attn.qkv.weight", "proj": "attn.proj.weight", "fc1": "mlp.fc1.weight", "fc2": "mlp.fc2.weight"}


def rel(a, b):
    a, b = a.detach().double().flatten().cpu(), b.detach().double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def randomize(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n_, p_ in module.named_parameters():
            if ".lora." in f".{n_}":
                continue
            p_.copy_(torch.randn(p_.shape, generator=g) * (0.05 if p_.dim() > 1 else 0.02) + (1.0 if "norm" in n_ and n_.endswith("weight") else 0.0))
    return module


def random_b(module, seed, std=0.1):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n_, p_ in module.named_parameters():
            if n_.endswith("_B") and ".lora." in f".{n_}":
                p_.copy_((torch.randn(p_.shape, generator=g) * std).to(p_.device))
    return module


def make_vit(C, img, seed=5):
    m = models_vit.VisionTransformer(img_size=img, patch_size=16, in_chans=3, num_classes=8, embed_dim=C, depth=2, num_heads=2, mlp_ratio=4,
                                     qkv_bias=True, norm_layer=LN, global_pool=True)
    return randomize(m, seed)


def make_st(C, img, seed=5):
    """the spatio-temporal fine-tune ViT (q / k / v layout): 6 frames in 2 temporal patches, (img / 16)^2 spatial ones, a cls token"""
    m = models_vit_st.VisionTransformer(num_frames=6, t_patch_size=3, img_size=img, patch_size=16, in_chans=1, num_classes=8, embed_dim=C,
                                        depth=2, num_heads=2, mlp_ratio=4, norm_layer=LN, sep_pos_embed=True, cls_embed=True,
                                        global_pool=True, dropout=0.0)
    return randomize(m, seed)


def adapted_vit(C, img, rank, seed=5, sd=None, make=None):
    m = (make or make_vit)(C, img, seed).to(DEV)
    lora.attach(m, rank=rank, alpha=2 * rank)
    if sd is None:
        random_b(m, seed + 1)
    else:
        m.load_state_dict(sd, strict=True)
    return m


def folded_twin(C, img, rank, sd, make=None):
    """a plain model holding merge_and_unload's weights of the adapted model whose state dict is ``sd``"""
    tmp = adapted_vit(C, img, rank, sd=sd, make=make)
    lora.merge_and_unload(tmp)
    assert not any(".lora." in k for k in tmp.state_dict())
    twin = (make or make_vit)(C, img).to(DEV)
    twin.load_state_dict(tmp.state_dict(), strict=True)
    return twin


def batch(C, img, B, seed=9):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, img, img, generator=g).to(DEV), torch.randint(0, 8, (B,), generator=g).to(DEV)


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("after_first_forward", [False, True])
@pytest.mark.parametrize("C,img,B,rank", CASES)
def test_attached_model_starts_as_the_base_model(C, img, B, rank, after_first_forward):
    x, _ = batch(C, img, B)
    base = make_vit(C, img).to(DEV).eval()
    with torch.no_grad():
        ref = base(x)
    m = make_vit(C, img).to(DEV).eval()
    if after_first_forward:
        with torch.no_grad():
            assert torch.equal(m(x), ref)
    new = lora.attach(m, rank=rank)
    assert len(new) == 2 * 2 * 4 and all(p.requires_grad for p in new)
    assert all(float(p.detach().abs().max()) == 0.0 for n_, p in m.named_parameters() if n_.endswith("_B"))
    with torch.no_grad():
        assert torch.equal(m(x), ref)
    assert all(get_arena(m).owns(p) for p in new), "the adapters live in the model's arena"


# ------------------------------------------------------------------------------------------------ 2, 3
@pytest.mark.parametrize("C,img,B,rank", CASES)
def test_adapted_model_against_its_folded_twin_and_the_oracle(C, img, B, rank):
    x, tgt = batch(C, img, B)
    m = adapted_vit(C, img, rank).train()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        m(x)                                                  # binds the arena
    arena = get_arena(m)
    arena.grad.fill_(7.0)
    xg = x.clone().requires_grad_(True)
    logits = m(xg)
    loss = torch.nn.functional.cross_entropy(logits, tgt)
    loss.backward()
    torch.cuda.synchronize()
    # no base gradient inside the adapted Blocks, their slices of the gradient arena untouched; the head has one
    for n_, p in m.named_parameters():
        if n_.startswith("blocks.") and ".lora." not in n_:
            assert p.grad is None and not p.requires_grad, n_
            assert bool((arena.grad_view(p) == 7.0).all()), n_
    assert m.head.weight.grad is not None and not bool((m.head.weight.grad == 7.0).all())
    ad_grads = {n_: (p.grad - 7.0).cpu() for n_, p in m.named_parameters() if ".lora." in n_}
    assert all(float(g.abs().max()) > 0 for g in ad_grads.values())
    # ---- the plain model with the folded weights: same operands, same launches
    twin = folded_twin(C, img, rank, sd).train()
    xt = x.clone().requires_grad_(True)
    logits_t = twin(xt)
    loss_t = torch.nn.functional.cross_entropy(logits_t, tgt)
    loss_t.backward()
    torch.cuda.synchronize()
    assert torch.equal(logits, logits_t) and torch.equal(loss, loss_t) and torch.equal(xg.grad, xt.grad)
    # ---- the CPU oracle in fp32 autograd, the adapted weights entering as W + s B A
    cfg = V.ViT2DConfig(img_size=img, patch_size=16, in_chans=3, num_classes=8, embed_dim=C, depth=2, num_heads=2, global_pool=True)
    P = {k: v.cpu().clone() for k, v in sd.items() if ".lora." not in k}
    s = 2.0                                                   # alpha = 2 rank
    leaves, merged = {}, {}
    for i in range(2):
        for t, key in TIMM_KEYS.items():
            A = sd[f"blocks.{i}.lora.{t}_A"].cpu().clone().requires_grad_(True)
            Bm = sd[f"blocks.{i}.lora.{t}_B"].cpu().clone().requires_grad_(True)
            leaves[f"blocks.{i}.lora.{t}_A"], leaves[f"blocks.{i}.lora.{t}_B"] = A, Bm
            w = P[f"blocks.{i}.{key}"] + s * (Bm @ A)
            w.retain_grad()
            P[f"blocks.{i}.{key}"] = merged[(i, t)] = w
    loss_o = torch.nn.functional.cross_entropy(V.vit2d_forward(P, x.cpu(), cfg), tgt.cpu())
    loss_o.backward()
    lines = [f"# width {C}, {(img // 16) ** 2 + 1} tokens, batch {B}, rank {rank}: relative L2 against the fp32 CPU oracle",
             "# tensor                      adapter kernels   full weight gradient, projected   bound (2 x)"]
    fails = []
    for i in range(2):
        for t, key in TIMM_KEYS.items():
            dW = dict(twin.named_parameters())[f"blocks.{i}.{key}"].grad.cpu().double()
            A, Bm = leaves[f"blocks.{i}.lora.{t}_A"], leaves[f"blocks.{i}.lora.{t}_B"]
            full = {"A": s * (Bm.detach().double().t() @ dW), "B": s * (dW @ A.detach().double().t())}
            for which, leaf in (("A", A), ("B", Bm)):
                name = f"blocks.{i}.lora.{t}_{which}"
                e_lora, e_full = rel(ad_grads[name], leaf.grad), rel(full[which], leaf.grad)
                lines.append(f"{name:28s} {e_lora:.3e}         {e_full:.3e}                         {2 * e_full:.3e}")
                print(lines[-1])
                try:
                    parity(f"lora/C{C}_r{rank}/{name}", e_lora, 2 * e_full)
                except AssertionError as e:
                    fails.append(str(e))
    try:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        mode = "w" if (C, rank) == CASES[0][::3] else "a"
        with open(os.path.join(ROOT, "profiles", "lora_parity.txt"), mode) as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass                                                  # a read-only checkout: the figures are in the parity ledger
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ 4
def make_block(kind, C, dp, seed=3):
    if kind == "block":
        blk = video_vit.Block(C, 2, 4.0, qkv_bias=True, norm_layer=LN, drop_path=dp)
    elif kind == "timm":
        blk = video_vit.TimmBlock(C, 2, 4.0, qkv_bias=True, norm_layer=LN, drop_path=dp)
    else:
        blk = video_vit.create_block(C, 2, 4.0, True, 0.0, 0.0, drop_path1=dp, drop_path2=dp, norm_layer=LN, act_layer=torch.nn.GELU,
                                     use_flash_attn=True, fused_bias_fc=False, fused_mlp=False, fused_dropout_add_ln=False)
    return randomize(blk, seed).to(DEV).train()


def run_block(blk, kind, mode, x, ws):
    """two accumulated backwards at ``mode`` from zeroed gradients and a reset seed -> (outputs, input gradient, parameter gradients)"""
    blk.recompute = mode
    with torch.no_grad():
        blk(x) if kind != "flash" else blk(x, None)
    get_arena(blk).zero_grad()
    torch.manual_seed(77)
    xg = x.clone().requires_grad_(True)
    outs = []
    for w in ws:
        if kind != "flash":
            o = blk(xg)
            loss = (o * w[0]).sum()
            outs.append(o.detach().clone())
        else:
            h, r = blk(xg, x * 0.5)
            loss = (h * w[0]).sum() + (r * w[1]).sum()
            outs += [h.detach().clone(), r.detach().clone()]
        loss.backward()
    torch.cuda.synchronize()
    return outs, xg.grad.clone(), {n_: p_.grad.clone() for n_, p_ in blk.named_parameters() if p_.grad is not None}


@pytest.mark.parametrize("dp", [0.0, 0.5])
@pytest.mark.parametrize("C,N,rank", [(64, 9, 4), (128, 65, 16)])
@pytest.mark.parametrize("kind", ["block", "timm", "flash"])
def test_recompute_levels_and_layouts(kind, C, N, rank, dp):
    blk = make_block(kind, C, dp)
    lora.attach(blk, rank=rank, alpha=2 * rank)
    random_b(blk, 11)
    g = torch.Generator().manual_seed(C + N)
    x = torch.randn(2, N, C, generator=g).to(DEV)
    ws = [(torch.randn(2, N, C, generator=g).to(DEV), torch.randn(2, N, C, generator=g).to(DEV)) for _ in range(2)]
    base_o, base_dx, base_g = run_block(blk, kind, "none", x, ws)
    assert set(base_g) == {n_ for n_, _ in blk.named_parameters() if n_.startswith("lora.")} and len(base_g) == 8
    if dp == 0.0:
        assert all(float(v.abs().max()) > 0 for v in base_g.values())
    for mode in ("light", "full"):
        o, dx, gr = run_block(blk, kind, mode, x, ws)
        assert all(torch.equal(a, b) for a, b in zip(o, base_o)) and torch.equal(dx, base_dx), mode
        assert set(gr) == set(base_g) and all(torch.equal(gr[n_], base_g[n_]) for n_ in base_g), mode
    with ops.weight_grads(False):                             # saliency-style backward: the same input gradient, no adapter gradient
        o, dx, gr = run_block(blk, kind, "none", x, ws)
    assert torch.equal(dx, base_dx) and all(float(v.abs().max()) == 0.0 for v in gr.values())
    # the folded twin of this layout
    tmp = make_block(kind, C, dp)
    lora.attach(tmp, rank=rank, alpha=2 * rank)
    tmp.load_state_dict(blk.state_dict(), strict=True)
    keys_before = set(make_block(kind, C, dp).state_dict())
    lora.merge_and_unload(tmp)
    assert set(tmp.state_dict()) == keys_before and all(p.requires_grad for p in tmp.parameters())
    twin = make_block(kind, C, dp)
    twin.load_state_dict(tmp.state_dict(), strict=True)
    o, dx, _ = run_block(twin, kind, "none", x, ws)
    assert all(torch.equal(a, b) for a, b in zip(o, base_o)) and torch.equal(dx, base_dx)


# ------------------------------------------------------------------------------------------------ 5, 6
class Args:
    accum_iter = 1; lr = 1e-2; min_lr = 1e-4; warmup_epochs = 0; epochs = 2; task_mode = "multi_cls"


ST_CASES = [(64, 32, 3, 4), (128, 64, 2, 16)]          # 9 and 33 tokens


def st_batch(img, B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 1, 6, img, img, generator=g).to(DEV), torch.randint(0, 8, (B,), generator=g).to(DEV)


def train_three_steps(C, img, B, rank):
    torch.manual_seed(1234)                                   # attach draws the adapters' A from the global generator
    m = adapted_vit(C, img, rank, make=make_st)
    lora.mark_only_lora_trainable(m)
    base_before = {k: v.detach().clone() for k, v in m.state_dict().items() if k.startswith("blocks.") and ".lora." not in k}
    opt = foptim.FusedAdamW(lr_decay.param_groups_lrd(m, 0.05, m.no_weight_decay(), 0.75), lr=Args.lr)
    scaler = misc.NativeScalerWithGradNormCount()
    loader = [st_batch(img, B, 20 + i) for i in range(3)]
    losses = []

    def crit(o, t):
        l = torch.nn.functional.cross_entropy(o, t)
        losses.append(float(l))
        return l
    stats = engine_finetune.train_one_epoch(m, crit, loader, opt, torch.device(DEV), 0, scaler, 1.0, None, None, Args)
    assert stats is not None
    torch.cuda.synchronize()
    return m, base_before, losses


@pytest.mark.parametrize("C,img,B,rank", ST_CASES)
def test_three_optimizer_steps_and_the_task_checkpoint(C, img, B, rank):
    m, base_before, losses = train_three_steps(C, img, B, rank)
    m2, _, losses2 = train_three_steps(C, img, B, rank)
    sd, sd2 = m.state_dict(), m2.state_dict()
    assert losses == losses2 and all(torch.equal(sd[k], sd2[k]) for k in sd), "two runs from one seed differ"
    assert all(torch.equal(sd[k], v) for k, v in base_before.items()), "a base weight of an adapted Block moved"
    torch.manual_seed(1234)
    init = adapted_vit(C, img, rank, make=make_st).state_dict()
    assert all(not torch.equal(sd[k], init[k]) for k in sd if ".lora." in k or k.startswith("head.")), "the adapters and the head were trained"
    assert losses[0] != losses[1]
    # the stale-merge test: the eval forward after raw-pointer optimizer steps against a freshly folded copy
    x, _ = st_batch(img, B, 40)
    m.eval()
    with torch.no_grad():
        got = m(x)
        ref = folded_twin(C, img, rank, {k: v.detach().clone() for k, v in sd.items()}, make=make_st).eval()(x)
    assert torch.equal(got, ref)
    # the per-task checkpoint: adapters + head + fc_norm on top of the pretrained weights
    task = lora.lora_state_dict(m)
    assert set(task) == {k for k in sd if ".lora." in k or k.split(".")[0] in ("head", "fc_norm", "norm")}
    nbytes = sum(v.numel() * v.element_size() for v in task.values())
    assert nbytes < sum(v.numel() * v.element_size() for v in sd.values()) / 3
    pretrained = {k: v for k, v in make_st(C, img).state_dict().items()}
    fresh = make_st(C, img, seed=99).to(DEV)
    lora.attach(fresh, rank=rank, alpha=2 * rank)
    a_init = {k: v.detach().clone() for k, v in fresh.state_dict().items() if ".lora." in k}
    missing, unexpected = checkpoint.load_pretrained(fresh, pretrained, strict=True)
    assert not missing and not unexpected
    assert all(torch.equal(fresh.state_dict()[k], v) for k, v in a_init.items()), "load_pretrained moved an adapter"
    with pytest.raises(RuntimeError, match="missing adapter keys"):
        lora.load_lora_state_dict(fresh, {k: v for k, v in task.items() if not k.endswith("fc2_B")})
    lora.load_lora_state_dict(fresh, task)
    fresh.eval()
    with torch.no_grad():
        assert torch.equal(fresh(x), got)
