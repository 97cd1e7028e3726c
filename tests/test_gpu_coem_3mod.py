"""GPU: the three-modality COEM model family on tiny towers (64 x 64, embed_dim 128, depth 2, out_dim 64: the towers of
tests/test_gpu_coem_loop.py) -- the two-modality en-face tower (models_vit_2mod) against the CPU oracle, ``forward_pair`` against two
``forward`` calls, CustomTextCLIP3Mod inside coem.train_one_epoch_3modalities, the classification models' fused join against the unfused
head, and the regression fine-tune loop and its evaluation (coem_finetune).
Tolerances: those of tests/test_gpu_coem.py on the same towers -- features rel-L2 <= 1e-2, tower gradients rel-L2 <= 6e-2."""
import json
import math
import os
import types
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import coem, coem_finetune as FT, models_vit_2mod, models_vit_st, ops
    from octcubem_amd import optim as foptim
from oracle import vit_ref as V
from tests import join_ref as R

DEV = "cuda"
FEAT_TOL, GRAD_TOL = 1e-2, 6e-2
E, OUT = 128, 64


def rel(a, b):
    a = torch.as_tensor(a).detach().double().flatten().cpu(); b = torch.as_tensor(b).detach().double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def tower2_params():
    """the 2-D oracle's parameters with ``head`` as embed_dim -> embed_dim, plus the two modality heads"""
    c2 = V.ViT2DConfig(img_size=64, patch_size=16, in_chans=3, num_classes=E, embed_dim=E, depth=2, num_heads=2, global_pool=True)
    P2 = V.init_from_shapes(V.vit2d_param_shapes(c2), seed=52)
    g = torch.Generator().manual_seed(58)
    for i in range(2):
        P2[f"mod_head_{i}.weight"] = torch.randn(OUT, E, generator=g) * 0.05
        P2[f"mod_head_{i}.bias"] = torch.randn(OUT, generator=g) * 0.02
    return c2, P2


def tower2(P2):
    t = models_vit_2mod.VisionTransformer(image_size=64, out_dim=OUT, embed_dim=E, depth=2, num_heads=2, mlp_ratio=4,
                                          norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), flash_compat=False)
    assert set(t.state_dict()) == set(P2)
    t.load_state_dict(P2, strict=True)
    return t.to(DEV)


def tower3():
    c3 = V.ViTSTConfig(num_frames=6, t_patch_size=3, img_size=64, patch_size=16, in_chans=1, num_classes=OUT, embed_dim=E, depth=2,
                       num_heads=2, global_pool=True)
    P3 = V.init_from_shapes(V.vit_st_param_shapes(c3), seed=51)
    m3 = models_vit_st.VisionTransformer(num_frames=6, t_patch_size=3, img_size=64, patch_size=16, in_chans=1, num_classes=OUT, embed_dim=E,
                                         depth=2, num_heads=2, sep_pos_embed=True, cls_embed=True, global_pool=True, dropout=0.0,
                                         mlp_ratio=4, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    m3.load_state_dict(P3, strict=True)
    return m3.to(DEV)


def oracle_2mod(Q, x, c2, k):
    h = torch.nn.functional.gelu(V.vit2d_forward(Q, x, c2))            # the oracle's head is this tower's ``head``
    return torch.nn.functional.linear(h, Q[f"mod_head_{k}.weight"], Q[f"mod_head_{k}.bias"])


def grads_close(mod, Q, tol=GRAD_TOL, skip=()):
    tot = math.sqrt(sum(float(v.grad.double().norm()) ** 2 for v in Q.values() if v.grad is not None))
    worst = 0.0
    for k, p in mod.named_parameters():
        gr = Q[k].grad
        if gr is None or float(gr.norm()) < 1e-3 * tot or k.startswith(skip):
            continue
        worst = max(worst, rel(p.grad, gr))
        assert rel(p.grad, gr) <= tol, (k, rel(p.grad, gr))
    return worst


@pytest.fixture(scope="module")
def images():
    g = torch.Generator().manual_seed(3)
    return torch.randn(3, 3, 64, 64, generator=g), torch.randn(3, 3, 64, 64, generator=g), torch.randn(3, OUT, generator=g)


@pytest.fixture(scope="module")
def oracle(images):
    """per modality: the oracle's output and the gradients of sum(out * w) -- computed once, shared, never changed"""
    x0, x1, w = images
    c2, P2 = tower2_params()
    res = []
    for k, x in ((0, x0), (1, x1)):
        Q = {n: v.clone().requires_grad_(True) for n, v in P2.items()}
        out = oracle_2mod(Q, x, c2, k)
        (out * w).sum().backward()
        res.append((out.detach(), Q))
    return res


@pytest.mark.parametrize("k", [0, 1])
def test_2mod_tower_matches_the_oracle(images, oracle, k):
    _, P2 = tower2_params()
    t = tower2(P2).train()
    out = t(images[k].to(DEV), modality=k)
    assert out.dtype == torch.float32 and tuple(out.shape) == (3, OUT)
    (out * images[2].to(DEV)).sum().backward()
    want, Q = oracle[k]
    print("modality", k, "output rel-L2", rel(out, want))
    assert rel(out, want) <= FEAT_TOL
    print("worst gradient rel-L2", grads_close(t, Q))
    other = getattr(t, f"mod_head_{1 - k}")
    assert not bool(other.weight.grad.any())                            # the other modality's head took no part
    with pytest.raises(ValueError):
        t(images[0].to(DEV), modality=2)


def test_forward_pair_equals_two_forwards(images, oracle):
    x0, x1, w = (a.to(DEV) for a in images)
    _, P2 = tower2_params()
    t = tower2(P2).eval()
    with torch.no_grad():
        y0, y1 = t.forward_pair(x0, x1)
        z0, z1 = t(x0, modality=0), t(x1, modality=1)
    for y, z, (want, _) in ((y0, z0, oracle[0]), (y1, z1, oracle[1])):
        print("pair / single against the oracle", rel(y, want), rel(z, want), "against each other", rel(y, z))
        assert rel(y, want) <= FEAT_TOL and rel(z, want) <= FEAT_TOL and rel(y, z) <= 2 * FEAT_TOL
    # train(), drop_path_rate = 0: one backward at 2 B against the sum of two backwards at B
    a = tower2(P2).train()
    y0, y1 = a.forward_pair(x0, x1)
    ((y0 * w).sum() + (y1 * w).sum()).backward()
    b = tower2(P2).train()
    (b(x0, modality=0) * w).sum().backward()
    (b(x1, modality=1) * w).sum().backward()
    ga, gb = dict(a.named_parameters()), dict(b.named_parameters())
    tot = math.sqrt(sum(float(p.grad.double().norm()) ** 2 for p in gb.values()))
    worst = max(rel(ga[k].grad, p.grad) for k, p in gb.items() if float(p.grad.norm()) >= 1e-3 * tot)
    print("worst per-tensor rel L2, one 2B backward against two B backwards:", worst)
    assert worst <= GRAD_TOL
    # ... and both equal the oracle's summed gradient
    Qsum = {k: types.SimpleNamespace(grad=oracle[0][1][k].grad + oracle[1][1][k].grad if oracle[0][1][k].grad is not None
                                     and oracle[1][1][k].grad is not None else (oracle[0][1][k].grad if oracle[0][1][k].grad is not None
                                                                                else oracle[1][1][k].grad)) for k in oracle[0][1]}
    grads_close(a, Qsum)


class Loader(list):
    pass


def as_data(items, bs, key="train", dataset=None):
    loader = Loader(items)
    loader.num_batches, loader.num_samples, loader.dataset = len(items), len(items) * bs, dataset
    return {key: types.SimpleNamespace(dataloader=loader, set_epoch=lambda e: None)}


def loop_args(**kw):
    base = dict(device=DEV, accum_freq=1, rank=0, world_size=1, batch_size=3, local_loss=False, gather_with_grad=False, horovod=False,
                correct_label=0, precision="amp", skip_scheduler=True, grad_clip_norm=None, log_every_n_steps=1, wandb=False,
                multimodal_type="oct_faf_ir", single_modality=None, fold=-1, val_frequency=1, epochs=1, save_logs=False,
                cls_dataset_type="BCVA_and_GAA")
    base.update(kw)
    return types.SimpleNamespace(**base)


def batch_items(n, bs, seed, flags=None, num_classes=None):
    g = torch.Generator().manual_seed(seed)
    items = []
    for b in range(n):
        x = {"oct": torch.rand(bs, 1, 6, 64, 64, generator=g), "ir": torch.randn(bs, 3, 64, 64, generator=g),
             "f2_faf": torch.randn(bs, 3, 64, 64, generator=g)}
        if num_classes:
            x["label"] = torch.randn(bs, num_classes, generator=g)
        mods = [torch.tensor(f) for f in flags[b]] if flags else [torch.ones(bs)] * 3
        items.append((x, (["n"] * bs, mods, (None, torch.arange(bs) + 10 * b))))
    return items


@pytest.mark.parametrize("fused", [False, True])
def test_3mod_model_in_the_three_modality_loop(fused):
    """tests/test_gpu_coem_loop.py::test_three_modality_micro_step_losses with the real model in place of its three-tower stand-in"""
    _, P2 = tower2_params()
    m3, t2 = tower3(), tower2(P2)
    model = coem.CustomTextCLIP3Mod(m3, t2).to(DEV).train()
    with torch.no_grad():
        model.logit_scale1.fill_(math.log(20.0)); model.logit_scale2.fill_(math.log(5.5))
    opts = [foptim.FusedAdamW(t.parameters(), lr=0.0) for t in (m3, t2)]
    opts.append(torch.optim.SGD([model.logit_scale, model.logit_scale1, model.logit_scale2], lr=0.0))
    flags = [[[1, 1, 1], [1, 1, 1], [1, 0, 1]], [[1, 1, 1], [1, 1, 1], [1, 1, 1]]]          # one sample without FAF
    items = batch_items(2, 3, 14, flags)
    items = [(x, (nm, [0] * 3, mods, None)) for x, (nm, mods, _) in items]                    # the contrastive loader's layout
    rec = coem.train_one_epoch_3modalities(model, as_data(items, 3), 0, opts, None, None, loop_args(accum_freq=2), fused=fused)
    torch.cuda.synchronize()
    assert rec["steps"] == 1 and len(rec["micro_losses"][0]) == 2
    with torch.no_grad():
        outs = [model(*(it[0][k].to(DEV) for k in ("oct", "ir", "f2_faf"))) for it in items]
        assert len(outs[0]) == 6
        feats = [torch.cat([o[k] for o in outs]) for k in range(3)]
        w_ir = torch.tensor(flags[0][1] + flags[1][1], dtype=torch.float32, device=DEV)
        w_faf = torch.tensor(flags[0][2] + flags[1][2], dtype=torch.float32, device=DEV)
        want = coem.ThreeModalityClipLoss(fused=fused)(*feats, *outs[0][3:], w_ir, w_faf)
        full = coem.ThreeModalityClipLoss()(*feats, *outs[0][3:], torch.ones_like(w_ir), torch.ones_like(w_faf))
    assert abs(float(want) - float(full)) > 1e-3 * float(full)
    for ml in rec["micro_losses"][0]:
        print("micro-step loss", float(ml), "by hand", float(want))
        assert abs(float(ml) - float(want)) <= 1e-6 * float(want)
    assert model.logit_scale1.grad is not None and model.logit_scale2.grad is not None
    assert float(model.text.arena.grad.abs().max()) > 0 and float(model.visual.arena.grad.abs().max()) > 0
    # single_modality: the 6-tuple with None for what is left out, and a number (not a method) for the third temperature
    with torch.no_grad():
        x = items[0][0]
        o = model(x["oct"].to(DEV), x["ir"].to(DEV), x["f2_faf"].to(DEV), single_modality="text2")
    assert o[0] is None and o[1] is None and torch.is_tensor(o[5]) and abs(float(o[5]) - 5.5) < 1e-4
    assert rel(o[2], outs[0][2]) <= 2 * FEAT_TOL                        # one pass at B against the pair's pass at 2 B


def cls_model(num_classes, three=True, seed=7):
    _, P2 = tower2_params()
    m3, t2 = tower3(), tower2(P2)
    torch.manual_seed(seed)
    if three:
        return coem.CustomTextCLIP3ModClassification(m3, t2, num_classes).to(DEV)
    return coem.CustomTextCLIPClassification(m3, t2, num_classes).to(DEV)


def head_bound(head, feats, mask):
    """|logits(fused) - logits(unfused)| <=: both LayerNorm outputs lie within the join bound of the exact y, so they are at most twice that
    apart; through fc1 (|W1| row sums), the 16-bit roundings of the pre-activation and the activation (GELU's slope is <= 1.13), fc2, and
    one 16-bit rounding of the logits on the GEMM route; f32 accumulation of K terms in any order on top of each product sum"""
    f = [None if x is None else x.detach().cpu().numpy() for x in feats]
    ref, bound = R.reference(f, mask, head.input_norm.weight.detach().cpu().numpy(), head.input_norm.bias.detach().cpu().numpy(),
                             eps=head.input_norm.eps, lp_is_f16=ops.LP_IS_F16)
    u_lp, _ = R.lp_roundoff(ops.LP_IS_F16)
    lp = lambda w: R.to_lp(w.detach().cpu().numpy(), ops.LP_IS_F16).astype(np.float64)      # the GEMMs read the 16-bit copy of a weight
    W1, b1 = lp(head.fc1.weight), head.fc1.bias.detach().double().cpu().numpy()
    W2 = lp(head.fc2.weight) if head.fc2.out_features % 8 == 0 else head.fc2.weight.detach().double().cpu().numpy()
    b2 = head.fc2.bias.detach().double().cpu().numpy()
    aW1, aW2 = np.abs(W1), np.abs(W2)
    y, dy = ref["y"], 2 * bound["y"]
    pre = y @ W1.T + b1
    d_pre = dy @ aW1.T + 2 * (W1.shape[1] + 2) * R.U * ((np.abs(y) + dy) @ aW1.T + np.abs(b1)) + 2 * u_lp * np.abs(pre)
    act = 0.5 * pre * (1 + np.vectorize(math.erf)(pre / math.sqrt(2)))
    d_act = 1.13 * d_pre + 2 * u_lp * (np.abs(act) + 1.13 * d_pre) + 4e-5 * np.abs(pre)           # + the polynomial GELU against erf (common.hpp)
    logits = act @ W2.T + b2
    return (d_act @ aW2.T + 2 * (W2.shape[1] + 2) * R.U * ((np.abs(act) + d_act) @ aW2.T + np.abs(b2)) + 2 * u_lp * np.abs(logits)
            + R.FLOOR), logits


@pytest.mark.parametrize("num_classes", [2, 5, 8])
def test_classification_model_fused_join_against_the_unfused_head(num_classes):
    model = cls_model(num_classes).eval()
    x = batch_items(1, 3, 16)[0][0]
    vol, ir, faf = (x[k].to(DEV) for k in ("oct", "ir", "f2_faf"))
    F = torch.nn.functional
    with torch.no_grad():
        raw = model._raw_features(vol, ir, faf)
        for single, mask in ((None, 7), ("image", 1), ("text1", 2), ("text2", 4)):
            out = model(vol, ir, faf, single_modality=single)
            assert len(out) == 4 and tuple(out[0].shape) == (3, num_classes) and out[0].dtype == torch.float32
            logits, n = model.forward_with_features(vol, ir, faf, single_modality=single)
            assert torch.equal(logits, out[0])
            feats = [r if (mask >> k) & 1 else None for k, r in enumerate(raw)]
            for k in range(3):                                           # the slots, directly on n_out
                if (mask >> k) & 1:
                    assert rel(n[k], F.normalize(raw[k], dim=-1)) <= (2 * FEAT_TOL if single and k else 1e-6)
                else:
                    assert not bool(n[k].any())
            if single in ("text1", "text2"):      # one pass at B here, the pair's pass at 2 B above: the GEMM plan differs, so do the features
                feats = list(model._raw_features(vol, ir, faf, single_modality=single))
            unfused = model.classification_head(torch.cat([F.normalize(f, dim=-1) if f is not None else torch.zeros_like(raw[0])
                                                           for f in feats], dim=-1))
            if single in ("text1", "text2"):
                logits, _ = model.classification_head.forward_joined(feats, mask)
            bound, exact = head_bound(model.classification_head, feats, mask)
            err = np.abs(logits.double().cpu().numpy() - unfused.double().cpu().numpy())
            print(num_classes, single, "worst |fused - unfused| / bound =", float((err / bound).max()), "logits rms", float(np.sqrt((exact ** 2).mean())))
            assert (err <= bound).all(), (single, float((err / bound).max()))
            assert (np.abs(logits.double().cpu().numpy() - exact) <= bound).all()
    two = cls_model(num_classes, three=False).eval()
    with torch.no_grad():
        lg, ls = two(vol, faf)
        assert tuple(lg.shape) == (3, num_classes) and abs(float(ls) - 1 / 0.07) < 1e-3
        only = two(vol, faf, single_modality="image")[0]
        fi = two.encode_image(vol)
        assert torch.equal(only, two.classification_head.forward_joined((fi, None), 1)[0]) and not torch.equal(only, lg)


def finetune_setup(lr):
    model = cls_model(5).train()
    opts = [foptim.FusedAdamW(model.visual.parameters(), lr=lr), foptim.FusedAdamW(model.text.parameters(), lr=lr),
            foptim.FusedAdamW(model.classification_head.parameters(), lr=lr),
            torch.optim.SGD([model.logit_scale, model.logit_scale1, model.logit_scale2], lr=lr)]
    return model, opts


def test_finetune_epoch_is_two_hand_rolled_steps():
    items = batch_items(2, 3, 17, num_classes=5)
    args = loop_args(multimodal_type="oct3d_paired_faf_ir_cls")
    model_a, opts_a = finetune_setup(1e-3)
    seen = []
    writer = types.SimpleNamespace(add_scalar=lambda name, val, step: seen.append((name, val, step)))
    rec = FT.train_one_epoch(model_a, as_data(items, 3), 0, opts_a, None, None, args, tb_writer=writer)
    model_b, opts_b = finetune_setup(1e-3)
    want, logits = [], []
    for x, _ in items:
        for o in opts_b:
            o.zero_grad()
        lg, *_ = model_b(x["oct"].to(DEV), x["ir"].to(DEV), x["f2_faf"].to(DEV))
        loss = FT.regression_loss(lg, x["label"].to(DEV))
        loss.backward()
        for o in opts_b:
            o.step()
        coem.clamp_logit_scale(model_b)
        want.append(loss.detach()); logits.append(lg.detach())
    torch.cuda.synchronize()
    assert rec["steps"] == 2
    for got, w in zip(rec["losses"], want):
        print("loss", float(got), "hand-rolled", float(w))
        assert abs(float(got) - float(w)) <= 1e-6 * abs(float(w))
    assert float(want[0]) != float(want[1])
    for ta, tb in ((model_a.visual, model_b.visual), (model_a.text, model_b.text), (model_a.classification_head, model_b.classification_head)):
        a, b = ta.arena.flat, tb.arena.flat
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-7
    assert float(model_a.classification_head.arena.grad.abs().max()) > 0 and float(model_a.text.arena.grad.abs().max()) > 0
    # the end-of-epoch metrics: numpy on the collected logits
    lo = rec["logits"].double().cpu().numpy(); la = torch.cat([x["label"] for x, _ in items]).double().numpy()
    assert lo.shape == (6, 5) and np.allclose(rec["labels"].cpu().numpy(), la)
    for j in range(5):
        r = np.corrcoef(la[:, j], lo[:, j])[0, 1]
        assert abs(rec[f"pearsonr_{j}"] - r) <= 1e-9 and abs(rec[f"R2_{j}"] - r * r) <= 1e-9 and abs(rec[f"r2_{j}"] - r * r) <= 1e-9
        assert abs(rec[f"mse_{j}"] - np.mean((la[:, j] - lo[:, j]) ** 2)) <= 1e-9
        assert abs(rec[f"mae_{j}"] - np.mean(np.abs(la[:, j] - lo[:, j]))) <= 1e-9
    names = {n for n, _, _ in seen}
    assert {"train/loss", "train/scale", "train/lr"} | {f"train/{k}_{j}" for k in FT.METRIC_KEYS for j in range(5)} <= names
    # the two-tower model on the chosen en-face image
    two = cls_model(5, three=False).train()
    opts = [foptim.FusedAdamW(t.parameters(), lr=0.0) for t in (two.visual, two.text, two.classification_head)]
    r2 = FT.train_one_epoch(two, as_data(items, 3), 0, opts, None, None, loop_args(multimodal_type="oct3d_paired_faf_cls", fold=2), tb_writer=writer)
    with torch.no_grad():
        lg = two(items[0][0]["oct"].to(DEV), items[0][0]["f2_faf"].to(DEV))[0]
    assert abs(float(r2["losses"][0]) - float(FT.regression_loss(lg, items[0][0]["label"].to(DEV)))) <= 1e-6 * float(r2["losses"][0])
    assert any(n.startswith("train_fold_2/") for n, _, _ in seen)
    with pytest.raises(NotImplementedError):
        FT.train_one_epoch(two, as_data(items, 3), 0, opts, None, None, loop_args(multimodal_type="oct_faf_ir"))


def test_finetune_steps_between_log_points_read_nothing_back(monkeypatch):
    """Three batches at the default log_every_n_steps = 100: step 0 and the last step write the log line (two scalars read back each),
    the step between them -- forward, loss, backward, optimizers, clamp -- reads nothing back, and the collected logits and labels come
    to the host once, after the last step."""
    items = batch_items(3, 3, 19, num_classes=5)
    model, opts = finetune_setup(0.0)
    syncs = {"item": 0, "cpu": 0}
    item, cpu = torch.Tensor.item, torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (syncs.__setitem__("item", syncs["item"] + 1), item(self))[1])
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (syncs.__setitem__("cpu", syncs["cpu"] + 1), cpu(self, *a, **k))[1])
    at_fetch = []

    class Counting(Loader):
        def __iter__(self):
            for it in list.__iter__(self):
                at_fetch.append(dict(syncs))
                yield it
    data = as_data(items, 3)
    counting = Counting(items)
    counting.num_batches, counting.num_samples = 3, 9
    data["train"].dataloader = counting
    rec = FT.train_one_epoch(model, data, 0, opts, None, None, loop_args(multimodal_type="oct3d_paired_faf_ir_cls", log_every_n_steps=100))
    monkeypatch.undo()
    print("host reads when each batch was fetched", at_fetch, "at the end", syncs)
    assert rec["steps"] == 3
    assert at_fetch == [{"item": 0, "cpu": 0}, {"item": 2, "cpu": 0}, {"item": 2, "cpu": 0}]
    assert syncs == {"item": 4, "cpu": 2}, syncs


def test_finetune_epoch_with_reducers_exchanges_three_arenas():
    """coem.make_reducers gives the classification head a reducer of its own; with a ONE-RANK RCCL communicator (force=True) the epoch
    with reducers must equal the local one, and every byte of the three gradient arenas must have gone through the communicator once
    per optimizer step -- the head's too, whose fc2 (5 classes) takes the F.linear route and never notifies a reducer."""
    from octcubem_amd import comm as ocomm
    items = batch_items(2, 3, 20, num_classes=5)
    args = loop_args(multimodal_type="oct3d_paired_faf_ir_cls")
    model, opts = finetune_setup(0.0)
    local = FT.train_one_epoch(model, as_data(items, 3), 0, opts, None, None, args)
    torch.cuda.synchronize()
    arenas = (model.visual.arena, model.text.arena, model.classification_head.arena)
    want = [a.grad.clone() for a in arenas]
    scales = [p.grad.clone() for p in (model.logit_scale, model.logit_scale1, model.logit_scale2) if p.grad is not None]
    comm1 = ocomm.NativeComm(ocomm.NativeComm.unique_id(), 0, 1, 0)
    try:
        reds = coem.make_reducers(model, comm=comm1, force=True, n_chunks=3)
        assert len(reds) == 3
        rec = FT.train_one_epoch(model, as_data(items, 3), 0, opts, None, None, args, reducers=reds)
        torch.cuda.synchronize()
        assert rec["steps"] == local["steps"] == 2
        for a, b in zip(rec["losses"], local["losses"]):
            assert abs(float(a) - float(b)) <= 1e-6 * abs(float(b))
        for a, w in zip(arenas, want):
            assert float(w.abs().max()) > 0 and float((a.grad - w).abs().max()) <= 1e-5 * float(w.abs().max()) + 1e-7
        assert float(model.classification_head.fc2.weight.grad.abs().max()) > 0
        for r, a in zip(reds, arenas):
            assert r.stats["bytes_total"] == 2 * 4 * a.total, (r.stats["bytes_total"], a.total)
        got = [p.grad for p in (model.logit_scale, model.logit_scale1, model.logit_scale2) if p.grad is not None]
        assert len(got) == len(scales) and all(torch.equal(g, w) for g, w in zip(got, scales))
    finally:
        comm1.destroy()


def test_evaluate_metrics_predictions_and_files(tmp_path):
    items = batch_items(2, 3, 18, num_classes=5)
    mean, std = [1.0, 50.0, 2.0, -3.0, 0.5], [2.0, 10.0, 0.5, 4.0, 1.5]
    ds = types.SimpleNamespace(preset_label_mean=None, preset_label_std=None, label_mean=mean, label_std=std)
    model = cls_model(5)
    args = loop_args(multimodal_type="oct3d_paired_faf_ir_cls", save_logs=True, checkpoint_path=str(tmp_path), fold=1)
    seen = []
    writer = types.SimpleNamespace(add_scalar=lambda name, val, step: seen.append(name))
    metrics, pred = FT.evaluate(model, as_data(items, 3, "val", ds), 1, args, tb_writer=writer, return_prediction=True)
    assert not model.training
    with torch.no_grad():
        lgs = [model(x["oct"].to(DEV), x["ir"].to(DEV), x["f2_faf"].to(DEV))[0] for x, _ in items]
        losses = [float(FT.regression_loss(lg, x["label"].to(DEV))) for lg, (x, _) in zip(lgs, items)]
    lo = torch.cat(lgs).double().cpu().numpy(); la = torch.cat([x["label"] for x, _ in items]).double().numpy()
    assert metrics["num_samples"] == 6 and metrics["epoch"] == 1 and abs(metrics["val_loss"] - sum(losses) / 2) <= 1e-6 * sum(losses)
    for j in range(5):
        r = np.corrcoef(la[:, j], lo[:, j])[0, 1]
        assert abs(metrics[f"pearsonr_{j}"] - r) <= 1e-9 and abs(metrics[f"r2_{j}"] - r * r) <= 1e-9
        assert abs(metrics[f"mse_{j}"] - np.mean((la[:, j] - lo[:, j]) ** 2)) <= 1e-9
    m32, s32 = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    assert np.array_equal(pred["original_labels"], la.astype(np.float32) * s32 + m32)
    assert np.array_equal(pred["original_logits"], lo.astype(np.float32) * s32 + m32)
    assert pred["original_true_idx"].tolist() == [0, 1, 2, 10, 11, 12]
    line = json.loads(open(os.path.join(tmp_path, "results-val-0_fold_1.jsonl")).read().strip())
    assert line == json.loads(json.dumps(metrics))
    folder = os.path.join(tmp_path, "log_val", "val_dataset_0", "fold_1", "epoch_0")
    assert sorted(os.listdir(folder)) == sorted(f"{n}.json" for n in FT.PLOT_NAMES)
    doc = json.load(open(os.path.join(folder, "BCVABASE.json")))
    assert doc["label"] == "BCVABASE" and (doc["min_val"], doc["max_val"]) == (40, 80) and doc["actual_epoch"] == 0 and doc["fold"] == 1
    assert np.allclose(doc["y_pred"], pred["original_logits"][:, 1]) and doc["true_idx"] == [0, 1, 2, 10, 11, 12]
    assert np.allclose(doc["poly_coef"], np.polyfit(pred["original_labels"][:, 1].astype(np.float64), pred["original_logits"][:, 1].astype(np.float64), 1))
    assert "val-0/val_fold_1/val_loss" in seen
    # the dataset's preset moments win; not due / not the main process: {}
    ds2 = types.SimpleNamespace(preset_label_mean=[0.0] * 5, preset_label_std=[1.0] * 5, label_mean=mean, label_std=std)
    _, p2 = FT.evaluate(model, as_data(items, 3, "test", ds2), 1, loop_args(multimodal_type="oct3d_paired_faf_ir_cls"), setting="test",
                        dinfo_idx=1, return_prediction=True)
    assert np.array_equal(p2["original_logits"], lo.astype(np.float32))
    assert FT.evaluate(model, as_data(items, 3, "val", ds), 1, loop_args(multimodal_type="oct3d_paired_faf_ir_cls", rank=1)) == {}
    assert FT.evaluate(model, as_data(items, 3, "val", ds), 3, loop_args(multimodal_type="oct3d_paired_faf_ir_cls", val_frequency=2, epochs=9)) == {}
