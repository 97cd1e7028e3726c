"""GPU: the COEM epoch loop (coem.train_one_epoch / train_one_epoch_3modalities) on tiny towers -- accum_freq 1 against train_step,
the cached-feature accumulation against one step on the whole batch and against the CPU oracle, the reducers' traffic per optimizer
step, the three-modality loss of every micro-step, and the scheduler / clamp."""
import math
import types
from functools import partial

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import coem, models_vit, models_vit_st
    from octcubem_amd import optim as foptim
from oracle import vit_ref as V

DEV = "cuda"


def rel(a, b):
    a = torch.as_tensor(a).detach().double().flatten().cpu(); b = torch.as_tensor(b).detach().double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def towers(seed2=52):
    """towers() of tests/test_gpu_coem.py, restated (``seed2``: the seed of the 2-D tower, for a second en-face tower)"""
    c3 = V.ViTSTConfig(num_frames=6, t_patch_size=3, img_size=64, patch_size=16, in_chans=1, num_classes=64, embed_dim=128, depth=2,
                       num_heads=2, global_pool=True)
    c2 = V.ViT2DConfig(img_size=64, patch_size=16, in_chans=3, num_classes=64, embed_dim=128, depth=2, num_heads=2, global_pool=True)
    P3 = V.init_from_shapes(V.vit_st_param_shapes(c3), seed=51)
    P2 = V.init_from_shapes(V.vit2d_param_shapes(c2), seed=seed2)
    kw = dict(mlp_ratio=4, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    m3 = models_vit_st.VisionTransformer(num_frames=6, t_patch_size=3, img_size=64, patch_size=16, in_chans=1, num_classes=64, embed_dim=128,
                                         depth=2, num_heads=2, sep_pos_embed=True, cls_embed=True, global_pool=True, dropout=0.0, **kw)
    m2 = models_vit.VisionTransformer(img_size=64, patch_size=16, in_chans=3, num_classes=64, embed_dim=128, depth=2, num_heads=2,
                                      qkv_bias=True, global_pool=True, **kw)
    m3.load_state_dict(P3, strict=True); m2.load_state_dict(P2, strict=True)
    return c3, c2, P3, P2, m3.to(DEV), m2.to(DEV)


def batches(n, bs, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(bs, 1, 6, 64, 64, generator=g), torch.randn(bs, 3, 64, 64, generator=g)) for _ in range(n)]


class Loader(list):
    pass


def as_data(items, bs):
    loader = Loader(items)
    loader.num_batches, loader.num_samples = len(items), len(items) * bs
    return {"train": types.SimpleNamespace(dataloader=loader, set_epoch=lambda e: None)}


def loop_args(**kw):
    base = dict(device=DEV, accum_freq=1, rank=0, world_size=1, batch_size=4, local_loss=False, gather_with_grad=False, horovod=False,
                correct_label=0, precision="amp", skip_scheduler=True, grad_clip_norm=None, log_every_n_steps=100, wandb=False,
                multimodal_type="default")
    base.update(kw)
    return types.SimpleNamespace(**base)


def make(lr):
    c3, c2, P3, P2, m3, m2 = towers()
    model = coem.CustomTextCLIP(m3, m2).to(DEV).train()
    opts = [foptim.FusedAdamW(m3.parameters(), lr=lr), foptim.FusedAdamW(m2.parameters(), lr=lr), torch.optim.SGD([model.logit_scale], lr=lr)]
    return (c3, c2, P3, P2), model, opts


def test_accum_1_is_three_train_steps():
    data = batches(3, 4, seed=11)
    _, model_a, opts_a = make(1e-3)
    rec = coem.train_one_epoch(model_a, as_data(data, 4), 0, opts_a, None, None, loop_args(), fused=False)
    _, model_b, opts_b = make(1e-3)
    want = [coem.train_step(model_b, coem.ClipLoss(), v.to(DEV), t.to(DEV), opts_b) for v, t in data]
    torch.cuda.synchronize()
    assert rec["steps"] == 3
    for got, w in zip(rec["losses"], want):
        assert abs(float(got) - float(w)) <= 1e-6 * abs(float(w))
    for ta, tb in ((model_a.visual, model_b.visual), (model_a.text, model_b.text)):
        a, b = ta.arena.flat, tb.arena.flat
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-7
    assert abs(float(model_a.logit_scale) - float(model_b.logit_scale)) <= 1e-6


@pytest.mark.parametrize("fused", [False, True])
def test_accum_2_is_one_step_on_the_whole_batch(fused):
    data = batches(2, 4, seed=12)
    (c3, c2, P3, P2), model, opts = make(0.0)
    rec = coem.train_one_epoch(model, as_data(data, 4), 0, opts, None, None, loop_args(accum_freq=2), fused=fused)
    torch.cuda.synchronize()
    assert rec["steps"] == 1 and len(rec["micro_losses"][0]) == 2
    grads = {id(t): {k: p.grad.clone() for k, p in t.named_parameters() if p.grad is not None} for t in (model.visual, model.text)}
    gl = float(model.logit_scale.grad)
    vol, ir = torch.cat([d[0] for d in data]), torch.cat([d[1] for d in data])
    # the CPU oracle on the 8 pairs is the judge
    Q3 = {k: v.clone().requires_grad_(True) for k, v in P3.items()}
    Q2 = {k: v.clone().requires_grad_(True) for k, v in P2.items()}
    lsr = torch.tensor(math.log(1 / 0.07), requires_grad=True)
    f3, _ = V.vit_st_forward(Q3, vol, c3)
    f3 = torch.nn.functional.normalize(f3, dim=-1)
    f2 = torch.nn.functional.normalize(V.vit2d_forward(Q2, ir, c2), dim=-1)
    lr = V.clip_loss(f3, f2, lsr.exp())
    lr.backward()
    for ml in rec["micro_losses"][0]:                            # every micro-step's loss is the full-batch loss
        assert abs(float(ml) - float(lr)) <= 5e-3 * float(lr), (float(ml), float(lr))
    print("logit_scale.grad", gl, "oracle (x 2)", 2 * float(lsr.grad))
    assert abs(gl - 2 * float(lsr.grad)) <= 5e-2 * abs(2 * float(lsr.grad)) + 1e-4
    for mod, Q in ((model.visual, Q3), (model.text, Q2)):
        tot = math.sqrt(sum(float(v.grad.double().norm()) ** 2 for v in Q.values() if v.grad is not None))
        for k, g in grads[id(mod)].items():
            gr = Q[k].grad
            if gr is None or float(gr.norm()) < 1e-3 * tot or k.endswith("attn.k.bias"):
                continue
            assert rel(g, gr) <= 6e-2, (k, rel(g, gr))
    # ... and one batch-of-8 train_step gives the same tower arenas and half the temperature gradient
    l8 = coem.train_step(model, coem.ClipLoss(), vol.to(DEV), ir.to(DEV), opts)
    torch.cuda.synchronize()
    assert abs(float(rec["losses"][0]) - float(l8)) <= 5e-3 * float(l8)
    assert abs(gl - 2 * float(model.logit_scale.grad)) <= 5e-2 * abs(gl) + 1e-4
    for mod in (model.visual, model.text):
        tot = math.sqrt(sum(float(p.grad.double().norm()) ** 2 for p in mod.parameters() if p.grad is not None))
        worst = max(rel(grads[id(mod)][k], p.grad) for k, p in mod.named_parameters()
                    if p.grad is not None and float(p.grad.norm()) >= 1e-3 * tot and not k.endswith("attn.k.bias"))
        print("worst per-tensor rel L2, accumulated against whole batch:", worst)
        assert worst <= 6e-2


def test_reducers_exchange_one_arena_per_optimizer_step():
    from octcubem_amd import comm as ocomm
    data = batches(4, 4, seed=13)
    _, model, opts = make(0.0)
    local = coem.train_one_epoch(model, as_data(data, 4), 0, opts, None, None, loop_args(accum_freq=2), fused=False)
    torch.cuda.synchronize()
    g3, g2, gl = model.visual.arena.grad.clone(), model.text.arena.grad.clone(), model.logit_scale.grad.clone()
    comm1 = ocomm.NativeComm(ocomm.NativeComm.unique_id(), 0, 1, 0)
    try:
        reds = coem.make_reducers(model, comm=comm1, force=True, n_chunks=3)
        rec = coem.train_one_epoch(model, as_data(data, 4), 0, opts, None, None, loop_args(accum_freq=2), reducers=reds, fused=False)
        torch.cuda.synchronize()
        assert rec["steps"] == local["steps"] == 2
        for a, b in zip(rec["losses"], local["losses"]):
            assert abs(float(a) - float(b)) <= 1e-6 * abs(float(b))
        for a, b in ((model.visual.arena.grad, g3), (model.text.arena.grad, g2)):
            assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-7
        assert torch.equal(model.logit_scale.grad, gl)
        # two optimizer steps of two micro-steps each: one arena per step through each reducer, not accum_freq arenas
        assert reds[0].stats["bytes_total"] == 2 * 4 * model.visual.arena.total
        assert reds[1].stats["bytes_total"] == 2 * 4 * model.text.arena.total
    finally:
        comm1.destroy()


class ThreeTowerCLIP(torch.nn.Module):
    def __init__(self, visual, ir, faf):
        super().__init__()
        self.visual, self.text, self.text2 = visual, ir, faf
        self.logit_scale = torch.nn.Parameter(torch.ones([]) * math.log(1 / 0.07))
        self.logit_scale1 = torch.nn.Parameter(torch.ones([]) * math.log(20.0))
        self.logit_scale2 = torch.nn.Parameter(torch.ones([]) * math.log(5.5))

    def forward(self, image, ir, faf):
        f = lambda t, x: torch.nn.functional.normalize(t(x).float(), dim=-1)
        return (f(self.visual, image), f(self.text, ir), f(self.text2, faf), self.logit_scale.exp(), self.logit_scale1.exp(),
                self.logit_scale2.exp())


@pytest.mark.parametrize("fused", [False, True])
def test_three_modality_micro_step_losses(fused):
    _, _, _, _, m3, m_ir = towers()
    _, _, _, _, _, m_faf = towers(seed2=57)
    model = ThreeTowerCLIP(m3, m_ir, m_faf).to(DEV).train()
    opts = [foptim.FusedAdamW(t.parameters(), lr=0.0) for t in (m3, m_ir, m_faf)]
    opts.append(torch.optim.SGD([model.logit_scale, model.logit_scale1, model.logit_scale2], lr=0.0))
    g = torch.Generator().manual_seed(14)
    flags = [[[1, 1, 1], [1, 1, 1], [1, 0, 1]], [[1, 1, 1], [1, 1, 1], [1, 1, 1]]]          # [batch][modality][sample]: one sample without FAF
    items = []
    for b in range(2):
        x = {"oct": torch.rand(3, 1, 6, 64, 64, generator=g), "ir": torch.randn(3, 3, 64, 64, generator=g),
             "f2_faf": torch.randn(3, 3, 64, 64, generator=g)}
        items.append((x, (["n"] * 3, [0] * 3, [torch.tensor(f) for f in flags[b]], None)))
    rec = coem.train_one_epoch_3modalities(model, as_data(items, 3), 0, opts, None, None,
                                           loop_args(accum_freq=2, batch_size=3, multimodal_type="oct_faf_ir"), fused=fused)
    torch.cuda.synchronize()
    assert rec["steps"] == 1 and len(rec["micro_losses"][0]) == 2
    # by hand: learning rates are 0 and the towers are deterministic, so the fresh features of a micro-step are the cached ones and
    # the spliced matrices are the concatenation over the group, whatever the position
    with torch.no_grad():
        outs = [model(*(it[0][k].to(DEV) for k in ("oct", "ir", "f2_faf"))) for it in items]
        feats = [torch.cat([o[k] for o in outs]) for k in range(3)]
        w_ir = torch.tensor(flags[0][1] + flags[1][1], dtype=torch.float32, device=DEV)
        w_faf = torch.tensor(flags[0][2] + flags[1][2], dtype=torch.float32, device=DEV)
        assert w_faf.tolist() == [1, 0, 1, 1, 1, 1]
        want = coem.ThreeModalityClipLoss(fused=fused)(*feats, *outs[0][3:], w_ir, w_faf)
        full = coem.ThreeModalityClipLoss()(*feats, *outs[0][3:], torch.ones_like(w_ir), torch.ones_like(w_faf))
    assert abs(float(want) - float(full)) > 1e-3 * float(full)            # the missing modality matters
    for ml in rec["micro_losses"][0]:
        print("micro-step loss", float(ml), "by hand", float(want))
        assert abs(float(ml) - float(want)) <= 1e-6 * float(want)
    assert model.logit_scale1.grad is not None and model.text2.arena.grad.abs().max() > 0


def test_scheduler_moves_every_optimizer_and_the_clamp_holds():
    data = batches(3, 4, seed=15)
    _, model, opts = make(1e-3)
    with torch.no_grad():
        model.logit_scale.fill_(10.0)
    sched = coem.cosine_lr(opts, 5e-4, 2, 9)
    seen = []
    writer = types.SimpleNamespace(add_scalar=lambda name, val, step: seen.append((name, step)))
    coem.train_one_epoch(model, as_data(data, 4), 1, opts, None, sched, loop_args(skip_scheduler=False, log_every_n_steps=1, grad_clip_norm=1.0),
                         tb_writer=writer)
    last = 3 * 1 + 2                                           # num_batches_per_epoch * epoch + i
    want = 0.5 * (1 + math.cos(math.pi * (last - 2) / (9 - 2))) * 5e-4
    for o in opts:
        for gr in o.param_groups:
            assert abs(gr["lr"] - want) <= 1e-15
    assert float(model.logit_scale) <= math.log(100) + 1e-6
    names = {n for n, _ in seen}
    assert {"train/loss", "train/scale", "train/lr", "train/samples_per_second", "train/data_time", "train/batch_time"} <= names
