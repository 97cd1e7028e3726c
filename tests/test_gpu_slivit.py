"""GPU: the SLIViT baseline (octcubem_amd/model_slivit_baseline.py) at tests/slivit_ref.SMALL against the committed golden
(tests/golden/slivit_small.npz: HF's ConvNextModel + the restated ViT in fp32, tools/gen_golden_slivit.py).

Tolerance of every quantity: 2 x the golden's ``rounding_err`` of that quantity for the library's operand type -- the REFERENCE's own
error when its GEMM operands are rounded where the library rounds them (the factor: the rounding model fixes neither the accumulation
order nor the GELU formula's error) -- and never more than what tests/test_gpu_model.py holds the bfloat16 library to (9.5e-3 on
predictions, 3e-2 on gradients).  A gradient norm is held to the rounding error of its whole gradient (| ||a|| - ||b|| | <= ||a - b||).
Measured figures are printed before anything is asserted.

Then: strict loading from the reference's key layout and the ``pretrained_weights`` mapping on the device, the weight-gradient switch,
autocast invariance, and the fine-tune loop with and without the ``convnext_slivit`` reshape."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import engine_finetune, misc, ops, optim as foptim
    from octcubem_amd import model_slivit_baseline as M
from tests import slivit_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "slivit_small.npz")
DEV = "cuda"
PRED_CAP, GRAD_CAP = 9.5e-3, 3e-2          # tests/test_gpu_model.py's bounds for the bfloat16 library


def build(P=None, seed=0):
    c = R.SMALL
    m = M.SLIViT(feature_extractor=M.ConvNextFeatureExtractor(depths=c["depths"], hidden_sizes=c["hidden_sizes"]), vit_dim=c["vit_dim"],
                 vit_depth=c["vit_depth"], heads=c["heads"], mlp_dim=c["mlp_dim"], num_of_patches=c["num_patches"],
                 patch_height=c["patch_height"], patch_width=c["patch_width"], num_classes=c["num_classes"], dim_head=c["dim_head"])
    P = R.init_params(c, seed=seed) if P is None else P
    res = m.load_state_dict(P, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return m.to(DEV), P


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())


def _subsample(t, n=256):
    f = t.reshape(-1)
    return f[::max(1, f.numel() // n)][:n]


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


@pytest.fixture(scope="module")
def step():
    """one forward + backward of the SMALL model on the golden's weights and inputs"""
    m, P = build()
    img, target = R.make_inputs(R.SMALL, seed=1)
    imgd = img.to(DEV)
    with torch.no_grad():
        feat = m.feature_extractor(imgd)
    m.arena.zero_grad()
    logits = m(imgd)
    loss = F.mse_loss(logits.float(), target.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().float().cpu().clone() for k, p in m.named_parameters()}
    return m, P, imgd, feat.detach().cpu(), logits.detach().float().cpu(), float(loss.detach()), grads


def test_small_model_against_the_golden(step):
    m, P, _, feat, logits, loss, grads = step
    g = np.load(GOLDEN)
    dt = "float16" if ops.LP_IS_F16 else "bfloat16"
    e = lambda name: float(g[f"rounding_err/{dt}/{name}"])
    keys = [str(k) for k in g["keys"]]
    assert keys == list(grads.keys()) == list(P.keys())
    assert feat.shape == tuple(g["feat"].shape) and feat.dtype == torch.float32 and logits.shape == tuple(g["logits"].shape)
    rows = [("feat", _rel(feat, g["feat"]), min(2 * e("feat"), PRED_CAP)),
            ("logits", _rel(logits, g["logits"]), min(2 * e("logits"), PRED_CAP)),
            ("loss", abs(loss - float(g["loss"])) / abs(float(g["loss"])), min(2 * e("loss"), PRED_CAP))]
    gerr = g[f"rounding_err/{dt}/grad"]
    for i, k in enumerate(keys):
        want = float(g["grad_norm"][i])
        rows.append(("norm " + k, abs(float(grads[k].double().norm()) - want) / want, min(2 * float(gerr[i]), GRAD_CAP)))
    for k in (str(k) for k in g["sample_keys"]):
        rows.append(("sample " + k, _rel(_subsample(grads[k]), g["grad_sample/" + k]), min(2 * e("sample/" + k), GRAD_CAP)))
    worst = sorted(rows, key=lambda r: -r[1] / r[2])
    print(f"[slivit {dt}] " + "; ".join(f"{n} {v:.2e} (<= {b:.2e})" for n, v, b in rows[:3]))
    print(f"[slivit {dt}] worst against their bounds: " + "; ".join(f"{n} {v:.2e} (<= {b:.2e})" for n, v, b in worst[:8]))
    bad = [(n, v, b) for n, v, b in rows if not v <= b]
    assert not bad, "; ".join(f"{n}: {v:.3e} > {b:.3e}" for n, v, b in bad)


def test_pretrained_weights_mapping_on_the_device(step, tmp_path):
    m, P, imgd, feat, *_ = step
    ck = {("model.convnext.embeddings." if k[len(R.FE)] == "0" else "model.convnext.encoder.") + k[len(R.FE) + 2:]: v
          for k, v in P.items() if k.startswith(R.FE)}
    ck["model.convnext.layernorm.weight"], ck["model.classifier.bias"] = torch.ones(128), torch.zeros(4)
    path = str(tmp_path / "chf.pth")
    torch.save(ck, path)
    fe = M.get_feature_extractor(4, path, depths=R.SMALL["depths"], hidden_sizes=R.SMALL["hidden_sizes"]).to(DEV)
    with torch.no_grad():
        assert torch.equal(bits(fe(imgd)), bits(feat.to(DEV)))        # the stand-alone extractor, from the mapped file: the same bits
    with pytest.raises(AssertionError):
        fe(imgd[:, :, :48])                                            # H not a multiple of 32


def test_weight_grads_off_leaves_the_arena_untouched(step):
    m, P, imgd, *_ = step
    target = R.make_inputs(R.SMALL, seed=1)[1].to(DEV)
    outs = []
    for on in (True, False):
        m.arena.zero_grad()
        x = imgd.clone().requires_grad_(True)
        loss = F.mse_loss(m(x).float(), target)
        with ops.weight_grads(on):
            loss.backward()
        outs.append((x.grad.clone(), m.arena.grad.clone()))
    assert int((bits(outs[0][1]) != 0).sum()) > 0 and int((bits(outs[1][1]) != 0).sum()) == 0
    assert float(outs[0][0].abs().max()) > 0 and torch.equal(bits(outs[0][0]), bits(outs[1][0]))      # the same input gradient either way
    assert all(p.grad is not None and p.grad.data_ptr() == m.arena.grad_view(p).data_ptr() for p in m.parameters())


def test_autocast_changes_nothing(step):
    m, P, imgd, feat, logits, *_ = step
    target = R.make_inputs(R.SMALL, seed=1)[1].to(DEV)
    res = []
    for amp in (False, True):
        m.arena.zero_grad()
        with torch.autocast("cuda", enabled=amp):
            out = m(imgd)
            f = m.feature_extractor(imgd)
        F.mse_loss(out.float(), target).backward()
        res.append((out.detach().clone(), f.detach().clone(), m.arena.grad.clone()))
    assert res[1][0].dtype == torch.float32 and res[1][1].dtype == torch.float32
    for a, b in zip(res[0][:2], res[1][:2]):
        assert torch.equal(bits(a), bits(b))
    # the gradients: the same launches on the same operands (a split weight gradient adds its slices in the order they finish)
    assert _rel(res[1][2], res[0][2]) <= 1e-5
    assert torch.equal(res[0][0].float().cpu(), logits)


class Args:
    accum_iter = 1; lr = 1e-4; min_lr = 1e-6; warmup_epochs = 1; epochs = 4; task_mode = "regression"
    patient_dataset_type = "convnext_slivit"


def test_finetune_loop_with_and_without_the_reshape(tmp_path):
    g = torch.Generator().manual_seed(11)
    vols = [torch.randn((2, 3, 3, 64, 64), generator=g) for _ in range(2)]       # [B, C, T, H, W] -> [B, T, H, W * C] = [2, 3, 64, 192]
    tgts = [torch.randn((2, 3), generator=g) for _ in range(2)]
    flat = [v.permute(0, 2, 3, 4, 1).reshape(2, 3, 64, 192) for v in vols]
    crit = torch.nn.MSELoss()
    seen = {}

    def run(loader, args):
        torch.manual_seed(0)
        m, _ = build(seed=2)
        opt = foptim.FusedAdamW(m.parameters(), lr=args.lr)
        losses = []

        def rec(o, t):
            l = crit(o.float(), t)
            losses.append(l.detach().clone())
            return l
        before = m.arena.flat.clone()
        stats = engine_finetune.train_one_epoch(m, rec, loader, opt, torch.device(DEV), 1, misc.NativeScalerWithGradNormCount(), 1.0, None,
                                                None, args)
        assert stats is not None and np.isfinite(stats["loss"]) and len(losses) == 2
        if not ops.LP_IS_F16:                                             # (on half operands the first steps settle the loss scale)
            assert not torch.equal(before, m.arena.flat)                  # the optimizer stepped
        return m, torch.stack(losses)

    class Other(Args):
        patient_dataset_type = "3D"

    m, with_reshape = run(list(zip(vols, tgts)), Args)
    _, without = run(list(zip(flat, tgts)), Other)
    # the reshape is the loop's only difference: the same first loss to the bit, the second (after an optimizer step on weight gradients
    # whose split-K slices add in the order they finish) to fp32 summation noise
    assert torch.equal(bits(with_reshape[0]), bits(without[0])) and _rel(with_reshape, without) <= 1e-5
    # a loop without the setting hands its samples to the model as they come: the first loss is the model's own on that batch
    ref_m, _ = build(seed=2)
    ref_m.train(True)
    assert torch.equal(bits(crit(ref_m(flat[0].to(DEV)).float(), tgts[0].to(DEV))), bits(without[0]))
    no_attr = types.SimpleNamespace(accum_iter=1, lr=1e-4, min_lr=1e-6, warmup_epochs=1, epochs=4, task_mode="regression")
    _, plain = run(list(zip(flat, tgts)), no_attr)
    assert torch.equal(bits(plain[0]), bits(without[0])) and _rel(plain, without) <= 1e-5
    # evaluation, regression mode, on the trained model: the report of column 0
    res = engine_finetune.evaluate_task_report(list(zip(vols, tgts)), m, DEV, str(tmp_path), 0, "val", 3, criterion=crit,
                                               task_mode="regression", args=Args)
    want = engine_finetune.evaluate_task_report(list(zip(flat, tgts)), m, DEV, str(tmp_path), 0, "val", 3, criterion=crit,
                                                task_mode="regression", args=Other)
    assert res == want and np.isfinite(res["mse"]) and np.isfinite(res["loss"])          # the same forward launches on the same rows
    ev = engine_finetune.evaluate(list(zip(vols, tgts)), m, DEV, criterion=crit, args=Args)
    assert ev["logits"].shape == (4, 3) and abs(ev["loss"] - res["loss"]) <= 1e-6 * abs(res["loss"])
