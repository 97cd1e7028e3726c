#!/usr/bin/env python3
"""Golden vectors for the RETFound-all slice-pooled ViT (CPU, build container only; needs the reference source tree).

    python tools/gen_golden_slicehead.py  ->  tests/golden/slicehead_small.npz

Runs the reference's own non-flash OCTCube/models_vit_3dhead.py ``VisionTransformerWith3DPoolingHead`` (over its
OCTCube/models_vit.py subclass) on the restated timm 0.3.2 base class of oracle.gen_golden.install_shims, as
oracle/gen_golden_vit2d.py does for the 2-D ViT.  Reduced configuration (tests/slicehead_ref.SMALL): embed 128, 2 heads of 64,
depth 2, 64 x 64 images (T = 17), 4 slices, batch 2, 3 classes; both global-pool and cls modes.  Weights are regenerated from
a seed (oracle.vit_ref.init_from_shapes), not stored.  Stored: input, target, features, logits, cross-entropy loss, the
gradients of tests/slicehead_ref.GRAD_KEYS, the reference's state_dict key list and the missing keys of its load_state_dict from a
RETFound-layout (timm ViT, ``norm.*``, no head) checkpoint -- the set main_finetune_downstream_*.py:516-518 asserts.
The flash variant cannot run here (flash-attn is shimmed to raise); its oracle is the same composition with the last block's
MLP branch alone (tests/slicehead_ref.forward(flash=True))."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
REF = os.environ.get("OCTCUBE_REFERENCE", "/root/reference")


def main():
    from functools import partial
    from oracle.gen_golden import install_shims
    from oracle import vit_ref as V
    from tests import slicehead_ref as R
    install_shims()
    torch.manual_seed(0)
    # the reference imports its base class as OCTCube.models_vit; the package's __init__ pulls in the SLIViT baseline
    # (transformers, torchvision), so the package is registered here by its path alone
    import types
    pkg = types.ModuleType("OCTCube"); pkg.__path__ = [os.path.join(REF, "OCTCube")]
    sys.modules["OCTCube"] = pkg
    from OCTCube import models_vit_3dhead as ref
    save = {}
    cfg0 = R.config(True)
    x, tgt = R.inputs(cfg0)
    save["x"] = x.numpy(); save["target"] = tgt.numpy()
    for gp in (True, False):
        cfg = R.config(gp)
        m = ref.VisionTransformerWith3DPoolingHead(global_pool=gp, img_size=cfg.img_size, patch_size=cfg.patch_size, in_chans=cfg.in_chans,
                                                   num_classes=cfg.num_classes, embed_dim=cfg.embed_dim, depth=cfg.depth,
                                                   num_heads=cfg.num_heads, mlp_ratio=4, qkv_bias=True,
                                                   norm_layer=partial(nn.LayerNorm, eps=1e-6))
        P = R.init(cfg)
        keys = list(m.state_dict())
        assert set(keys) == set(P), set(keys) ^ set(P)
        m.load_state_dict(P, strict=True)
        m.eval()
        feats = m.forward_features(x)
        out = m.head(feats)
        assert torch.equal(out, m(x))
        loss = torch.nn.functional.cross_entropy(out, tgt)
        m.zero_grad(); loss.backward()
        tag = "gp1" if gp else "gp0"
        save[f"{tag}/cfg"] = json.dumps(cfg.__dict__)
        save[f"{tag}/features"] = feats.detach().numpy(); save[f"{tag}/out"] = out.detach().numpy(); save[f"{tag}/loss"] = loss.detach().numpy()
        grads = dict(m.named_parameters())
        for k in R.grad_keys(cfg):
            save[f"{tag}/grad/{k}"] = R.sub(grads[k].grad).numpy()
            save[f"{tag}/gnorm/{k}"] = float(grads[k].grad.double().norm())
        save[f"{tag}/keys"] = json.dumps(keys)
        # a RETFound-layout checkpoint: the timm ViT's keys (fused attn.qkv, ``norm``), the head removed by the driver
        ck = {k: torch.zeros(s) for k, s in V.vit2d_param_shapes(R.config(False)).items() if not k.startswith("head.")}
        msg = m.load_state_dict(ck, strict=False)
        save[f"{tag}/ckpt_missing"] = json.dumps(sorted(msg.missing_keys))
        save[f"{tag}/ckpt_unexpected"] = json.dumps(sorted(msg.unexpected_keys))
    save["param_seed"] = R.PARAM_SEED
    outp = os.path.join(ROOT, "tests", "golden", "slicehead_small.npz")
    np.savez_compressed(outp, **save)
    print("wrote", outp, os.path.getsize(outp), "bytes")


if __name__ == "__main__":
    main()
