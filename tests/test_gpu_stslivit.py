"""GPU: OCTCube with the SLIViT slice head (octcubem_amd/models_vit_st_flash_attn_slivit.py) at tests/stslivit_ref.SMALL against the
committed golden (tests/golden/stslivit_small.npz: the reference's own model class in fp32, tools/gen_golden_stslivit.py).

Tolerance of every quantity: 2 x the golden's ``rounding_err`` of that quantity for the library's operand type -- the REFERENCE's own
error when its operands are rounded where the library rounds them (the factor: the rounding model fixes neither the accumulation order
nor the GELU formula's error) -- and never more than what tests/test_gpu_model.py holds the bfloat16 library to (9.5e-3 on predictions,
3e-2 on gradients): the convention of tests/test_gpu_slivit.py.  A gradient norm is held to the rounding error of its whole gradient.
Parameters without a gradient (``norm.*``) must have none or exact zeros; a gradient that is mathematically zero (``attn.k.bias``: below
1e-6 of the total norm in the golden) is fp32 noise on both sides and only its size is comparable (<= 1e-4 of the total), as in
tests/test_gpu_model.py.  Measured figures are printed before anything is asserted."""
import os
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import engine_finetune, misc, ops, optim as foptim
    from octcubem_amd import models_vit_st_flash_attn_slivit as M
from tests import stslivit_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stslivit_small.npz")
DEV = "cuda"
PRED_CAP, GRAD_CAP = 9.5e-3, 3e-2          # tests/test_gpu_model.py's bounds for the bfloat16 library


def build(P=None, **kw):
    c = S.SMALL
    args = dict(num_frames=c["num_frames"], t_patch_size=c["t_patch_size"], img_size=c["img_size"], patch_size=c["patch_size"],
                in_chans=c["in_chans"], num_classes=c["num_classes"], embed_dim=c["embed_dim"], depth=c["depth"], num_heads=c["num_heads"],
                mlp_ratio=4, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), sep_pos_embed=True, cls_embed=True, global_pool=True,
                slivit_depth_num=c["slivit_depth_num"])
    args.update(kw)
    m = M.VisionTransformer(**args)
    P = S.init_params() if P is None else P
    if args.get("use_flash_attn"):
        res = m.load_state_dict_to_backbone(dict(P), strict=True)
    else:
        res = m.load_state_dict(P, strict=True)                     # strict, from the reference's key set
    assert not res.missing_keys and not res.unexpected_keys
    return m.to(DEV), P


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm())


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


@pytest.fixture(scope="module")
def step():
    """one forward + backward of the SMALL model on the golden's weights and inputs"""
    m, P = build()
    x, target = S.make_inputs()
    xd = x.to(DEV)
    m.train()
    with torch.no_grad():
        m(xd)                                # binds the arena
    m.arena.zero_grad()
    logits, emb = m(xd, return_embeddings=True)
    loss = F.mse_loss(logits.float(), target.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: (None if p.grad is None else p.grad.detach().float().cpu().clone()) for k, p in m.named_parameters()}
    return m, P, xd, target.to(DEV), emb, logits.detach().float().cpu(), float(loss.detach()), grads


def test_small_model_against_the_golden(step):
    m, P, _, _, emb, logits, loss, grads = step
    g = np.load(GOLDEN)
    dt = "float16" if ops.LP_IS_F16 else "bfloat16"
    e = lambda name: float(g[f"rounding_err/{dt}/{name}"])
    keys = [str(k) for k in g["keys"]]
    assert sorted(keys) == sorted(grads.keys()) == sorted(P.keys())
    assert tuple(emb.shape) == tuple(g["embedding"].shape) and emb.dtype == torch.float32 and logits.shape == tuple(g["logits"].shape)
    rows = [("embedding", _rel(emb, g["embedding"]), min(2 * e("embedding"), PRED_CAP)),
            ("logits", _rel(logits, g["logits"]), min(2 * e("logits"), PRED_CAP)),
            ("loss", abs(loss - float(g["loss"])) / abs(float(g["loss"])), min(2 * e("loss"), PRED_CAP))]
    gerr = g[f"rounding_err/{dt}/grad"]
    total = float(np.sqrt((g["grad_norm"].astype(np.float64) ** 2).sum()))
    zero_like = []
    for i, k in enumerate(keys):
        want = float(g["grad_norm"][i])
        if want == 0.0:                                              # ``norm.*``: no gradient in the reference
            assert k in S.NO_GRAD and (grads[k] is None or float(grads[k].abs().max()) == 0.0), k
        elif want < 1e-6 * total:
            zero_like.append((k, float(grads[k].double().norm()) / total))
        else:
            rows.append(("norm " + k, abs(float(grads[k].double().norm()) - want) / want, min(2 * float(gerr[i]), GRAD_CAP)))
    for k in (str(k) for k in g["sample_keys"]):
        rows.append(("sample " + k, _rel(S.subsample(grads[k]), g["grad_sample/" + k]), min(2 * e("sample/" + k), GRAD_CAP)))
    worst = sorted(rows, key=lambda r: -r[1] / r[2])
    print(f"[stslivit {dt}] " + "; ".join(f"{n} {v:.2e} (<= {b:.2e})" for n, v, b in rows[:3]))
    print(f"[stslivit {dt}] worst against their bounds: " + "; ".join(f"{n} {v:.2e} (<= {b:.2e})" for n, v, b in worst[:8]))
    print(f"[stslivit {dt}] mathematically zero gradients, size / total: " + "; ".join(f"{k} {v:.1e}" for k, v in zero_like))
    bad = [(n, v, b) for n, v, b in rows if not v <= b]
    assert not bad, "; ".join(f"{n}: {v:.3e} > {b:.3e}" for n, v, b in bad)
    assert zero_like and all(v <= 1e-4 for _, v in zero_like), zero_like


def test_global_pool_false_raises():
    m, _ = build(global_pool=False)
    with pytest.raises(ValueError, match="Class token can not be implemented for Slivit head"):
        m(S.make_inputs()[0].to(DEV))
    assert len(m(S.make_inputs()[0].to(DEV), hidden_states=True)) == S.SMALL["depth"]     # as in the reference: returned before the check


def test_return_embeddings_is_a_view_of_the_stream(step):
    m, P, xd, *_ = step
    g = np.load(GOLDEN)
    dt = "float16" if ops.LP_IS_F16 else "bfloat16"
    with torch.no_grad():
        logits, emb = m(xd, return_embeddings=True)
        stream = m(xd, hidden_states=True)[-1]
    N, T, C, L = S.SMALL["batch"], 3, 64, 9
    assert emb.shape == (N, T, C, L) and emb.stride() == ((1 + T * L) * C, L * C, 1, C) and emb._base is not None     # no copy was made
    assert torch.equal(bits(emb), bits(stream[:, 1:].reshape(N, T, L, C).transpose(2, 3)))
    assert _rel(emb, g["embedding"]) <= min(2 * float(g[f"rounding_err/{dt}/embedding"]), PRED_CAP)
    assert torch.equal(bits(m(xd)), bits(logits))


def test_fused_and_aten_slice_embedding_agree(step):
    """the head's own ``forward_head`` on the embedding view: the same weights through the materialised transpose, F.layer_norm and the
    same GEMMs"""
    m, P, xd, target, _, logits, loss, grads = step
    g = np.load(GOLDEN)
    dt = "float16" if ops.LP_IS_F16 else "bfloat16"
    m.arena.zero_grad()
    _, emb = m(xd, return_embeddings=True)
    out = m.SLIViT_head.forward_head(emb)
    F.mse_loss(out.float(), target).backward()
    got = {k: p.grad.detach().float().cpu().clone() for k, p in m.named_parameters() if p.grad is not None}
    tol = min(2 * float(g[f"rounding_err/{dt}/logits"]), PRED_CAP)
    print(f"[stslivit {dt}] fused vs ATen slice embedding: logits {_rel(out.detach().float().cpu(), logits):.2e} (<= {tol:.2e})")
    assert _rel(out.detach().float().cpu(), logits) <= tol
    for k in ("SLIViT_head.to_patch_embedding.1.weight", "SLIViT_head.to_patch_embedding.1.bias", "SLIViT_head.to_patch_embedding.2.weight",
              "patch_embed.proj.weight"):
        i = [str(q) for q in g["keys"]].index(k)
        assert _rel(got[k], grads[k]) <= min(2 * float(g[f"rounding_err/{dt}/grad"][i]), GRAD_CAP), k


def test_flash_blocks_drop_the_last_residual():
    """use_flash_attn=True hands on the last block's MLP branch alone: the non-flash model with ``flash_compat`` (the same semantics on
    the other block class), and the restatement without the last residual, to the restatement's own rounding error"""
    x, _ = S.make_inputs()
    xd = x.to(DEV)
    flash, P = build(use_flash_attn=True)
    compat, _ = build(flash_compat=True)
    plain, _ = build()
    with torch.no_grad():
        a, ea = flash(xd, return_embeddings=True)
        b, eb = compat(xd, return_embeddings=True)
        c = plain(xd)
    dtp = torch.float16 if ops.LP_IS_F16 else torch.bfloat16
    e0, l0 = S.forward(P, x, last_residual=False)
    e1, l1 = S.forward(P, x, dt=dtp, last_residual=False)
    tol_l, tol_e = min(2 * _rel(l1, l0), PRED_CAP), min(2 * _rel(e1, e0), PRED_CAP)
    print(f"[stslivit flash] vs restatement: logits {_rel(a, l0):.2e} (<= {tol_l:.2e}), embedding {_rel(ea, e0):.2e} (<= {tol_e:.2e}); "
          f"vs flash_compat: {_rel(a, b):.2e}; vs the standard residual: {_rel(a, c):.2e}")
    assert _rel(a, l0) <= tol_l and _rel(ea, e0) <= tol_e
    assert _rel(a, b) <= tol_l and _rel(ea, eb) <= tol_e
    assert _rel(ea, S.forward(P, x)[0]) > 10 * tol_e               # and it is not the standard residual


def test_weight_grads_off_leaves_the_arena_untouched(step):
    m, P, xd, target, *_ = step
    outs = []
    for on in (True, False):
        m.arena.zero_grad()
        x = xd.clone().requires_grad_(True)
        loss = F.mse_loss(m(x).float(), target)
        with ops.weight_grads(on):
            loss.backward()
        outs.append((x.grad.clone(), m.arena.grad.clone()))
    assert int((bits(outs[0][1]) != 0).sum()) > 0 and int((bits(outs[1][1]) != 0).sum()) == 0
    assert float(outs[0][0].abs().max()) > 0 and torch.equal(bits(outs[0][0]), bits(outs[1][0]))      # the same input gradient either way


def test_autocast_changes_nothing(step):
    m, P, xd, target, _, logits, *_ = step
    res = []
    for amp in (False, True):
        m.arena.zero_grad()
        with torch.autocast("cuda", enabled=amp):
            out, emb = m(xd, return_embeddings=True)
        F.mse_loss(out.float(), target).backward()
        res.append((out.detach().clone(), emb.detach().clone(), m.arena.grad.clone()))
    assert res[1][0].dtype == torch.float32 and res[1][1].dtype == torch.float32
    for a, b in zip(res[0], res[1]):
        assert torch.equal(bits(a), bits(b))
    assert torch.equal(res[0][0].float().cpu(), logits)


def test_recompute_modes_are_bit_identical(step):
    from tests.test_gpu_recompute import assert_modes_agree
    m, P, xd, target, *_ = step

    def one(model, k):
        out = model(xd * (1.0 + 0.25 * k))
        return F.mse_loss(out.float(), target), out

    assert_modes_agree(m, one)


class Args:
    # AdamW's first steps move every weight by the learning rate; the sum of |gradient| here is 1.2e5, so 1e-4 would promise a drop of
    # 12 on a loss of 2.7 and overshoots (the restatement's loss after one sign step: 1e-4 -> 7.47, 1e-5 -> 1.66, 1e-6 -> 2.55)
    accum_iter = 1; lr = 1e-5; min_lr = 1e-7; warmup_epochs = 0; epochs = 4; task_mode = "regression"
    patient_dataset_type = "3D_st_flash_attn_slivit"


def test_finetune_steps_lower_the_loss(tmp_path):
    torch.manual_seed(0)
    m, _ = build()
    x, target = S.make_inputs()
    loader = [(x, target), (x, target)]
    crit = torch.nn.MSELoss()
    losses = []

    def rec(o, t):
        l = crit(o.float(), t)
        losses.append(float(l.detach()))
        return l

    opt = foptim.FusedAdamW(m.parameters(), lr=Args.lr)
    stats = engine_finetune.train_one_epoch(m, rec, loader, opt, torch.device(DEV), 1, misc.NativeScalerWithGradNormCount(), 1.0, None, None,
                                            Args)
    assert stats is not None and np.isfinite(stats["loss"]) and len(losses) == 2
    m.eval()
    with torch.no_grad():
        after = float(crit(m(x.to(DEV)).float(), target.to(DEV)))
    print(f"[stslivit finetune] losses {losses[0]:.4f} -> {losses[1]:.4f} -> {after:.4f}")
    if not ops.LP_IS_F16:                                           # (on half operands the first steps settle the loss scale)
        assert losses[1] < losses[0] and after < losses[0]
    res = engine_finetune.evaluate_task_report(loader, m, DEV, str(tmp_path), 0, "val", 1, criterion=crit, task_mode="regression", args=Args)
    assert np.isfinite(res["mse"]) and np.isfinite(res["loss"])
