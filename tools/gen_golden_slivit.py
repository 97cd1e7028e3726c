#!/usr/bin/env python
"""Writes tests/golden/slivit_small.npz: the SLIViT baseline at tests/slivit_ref.SMALL in fp32 on the CPU.

The ConvNeXt half is ``transformers``' real ``ConvNextModel`` built from a config (nothing is downloaded) with the seeded weights of
slivit_ref.init_params loaded into its ``embeddings`` / ``encoder``; the ViT half is slivit_ref.head_forward (vit-pytorch is not
installed), autograd running through both.  Stored, all fp32: the feature map, the logits, the MSE loss against the seeded target, the
gradient norm of every parameter, sub-sampled gradients of SAMPLE_KEYS, the state-dict key list -- and ``rounding_err/<dtype>/...``:
the relative error of slivit_ref's ROUNDING-MODEL run (operands rounded to bfloat16 / float16 where the library rounds) against
slivit_ref's fp32 run, per stored quantity: ``feat``, ``logits`` (relative L2), ``loss`` (relative), ``grad/<key>`` (relative L2 of
the whole gradient -- it bounds the error of that gradient's norm) and ``sample/<key>`` (relative L2 over the stored samples).
tests/test_gpu_slivit.py takes its tolerances from these: the reference's own error under operand rounding, never the library's.

    python tools/gen_golden_slivit.py            (needs transformers; tests/test_cpu_slivit.py checks the file without it)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import slivit_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "slivit_small.npz")
SAMPLES = 256


def sample_keys(cfg):
    """one parameter of every kind the model has, first and last layers of both halves"""
    fe, last = R.FE, f"1.stages.3.layers.{cfg['depths'][3] - 1}."
    return [fe + "0.patch_embeddings.weight", fe + "0.layernorm.weight", fe + "1.stages.0.layers.0.dwconv.weight",
            fe + "1.stages.0.layers.0.dwconv.bias", fe + "1.stages.0.layers.0.layer_scale_parameter", fe + "1.stages.0.layers.0.pwconv1.weight",
            fe + "1.stages.1.downsampling_layer.1.weight", fe + "1.stages.2.layers.1.pwconv2.weight", fe + last + "dwconv.weight",
            fe + last + "layer_scale_parameter", fe + last + "layernorm.bias", "to_patch_embedding.1.weight", "to_patch_embedding.2.weight",
            "pos_embedding", "cls_token", "transformer.layers.0.0.to_qkv.weight", "transformer.layers.0.0.to_out.0.bias",
            "transformer.layers.1.1.net.1.weight", "transformer.layers.1.1.net.4.weight", "transformer.norm.weight", "mlp_head.weight"]


def subsample(t, n=SAMPLES):
    f = t.reshape(-1)
    step = max(1, f.numel() // n)
    return f[::step][:n]


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def hf_forward_backward(P, img, target, cfg):
    from transformers import ConvNextConfig, ConvNextModel
    hf = ConvNextModel(ConvNextConfig(depths=list(cfg["depths"]), hidden_sizes=list(cfg["hidden_sizes"])))
    sd = {}
    for k, v in P.items():
        if k.startswith(R.FE + "0."):
            sd["embeddings." + k[len(R.FE) + 2:]] = v
        elif k.startswith(R.FE + "1."):
            sd["encoder." + k[len(R.FE) + 2:]] = v
    missing, unexpected = hf.load_state_dict(sd, strict=False)
    assert not unexpected and all(m.startswith("layernorm.") for m in missing), (missing, unexpected)     # the pooled LayerNorm: dropped
    hf.eval()
    head = {k: v.detach().clone().requires_grad_(True) for k, v in P.items() if not k.startswith(R.FE)}
    feat = hf.encoder(hf.embeddings(img)).last_hidden_state
    logits = R.head_forward(head, feat, cfg, None)
    loss = torch.nn.functional.mse_loss(logits, target)
    loss.backward()
    G = {k: v.grad for k, v in head.items()}
    for n, p in hf.named_parameters():
        if n.startswith("embeddings."):
            G[R.FE + "0." + n[len("embeddings."):]] = p.grad
        elif n.startswith("encoder."):
            G[R.FE + "1." + n[len("encoder."):]] = p.grad
    hf_keys = [("0." + k[len("embeddings."):]) if k.startswith("embeddings.") else ("1." + k[len("encoder."):])
               for k in hf.state_dict().keys() if k.startswith(("embeddings.", "encoder."))]
    return feat.detach(), logits.detach(), loss.detach(), G, hf_keys


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)                 # one summation order whatever the machine
    cfg = R.SMALL
    P = R.init_params(cfg, seed=0)
    img, target = R.make_inputs(cfg, seed=1)
    feat, logits, loss, G, hf_keys = hf_forward_backward(P, img, target, cfg)
    skeys = sample_keys(cfg)
    out = {"feat": feat.numpy(), "logits": logits.numpy(), "loss": np.float32(loss), "keys": np.array(list(P.keys())),
           "extractor_keys": np.array(hf_keys), "sample_keys": np.array(skeys),
           "grad_norm": np.array([float(G[k].double().norm()) for k in P.keys()], dtype=np.float32)}
    for k in skeys:
        out["grad_sample/" + k] = subsample(G[k]).numpy()
    f0, l0, s0, G0 = R.forward_backward(P, img, target, cfg, None)
    for name, dt in (("bfloat16", torch.bfloat16), ("float16", torch.float16)):
        f1, l1, s1, G1 = R.forward_backward(P, img, target, cfg, dt)
        pre = f"rounding_err/{name}/"
        out[pre + "feat"] = np.float32(rel(f1, f0))
        out[pre + "logits"] = np.float32(rel(l1, l0))
        out[pre + "loss"] = np.float32(abs(float(s1) - float(s0)) / abs(float(s0)))
        out[pre + "grad"] = np.array([rel(G1[k], G0[k]) for k in P.keys()], dtype=np.float32)
        for k in skeys:
            out[pre + "sample/" + k] = np.float32(rel(subsample(G1[k]), subsample(G0[k])))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes; loss {float(loss):.6f}; rounding_err logits bf16 "
          f"{float(out['rounding_err/bfloat16/logits']):.2e} f16 {float(out['rounding_err/float16/logits']):.2e}; "
          f"ref vs HF feat {rel(f0, feat):.2e} logits {rel(l0, logits):.2e}")


if __name__ == "__main__":
    main()
