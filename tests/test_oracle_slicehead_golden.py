"""CPU: the slice-head oracle composition (tests/slicehead_ref.py) reproduces the fixture the reference's own
OCTCube/models_vit_3dhead.py produced (tests/golden/slicehead_small.npz, tools/gen_golden_slicehead.py): features, logits, loss and
the stored gradients to 1e-5 -- which pins the oracle the GPU tests of the RETFound-all model compare against."""
import json
import os

import numpy as np
import pytest
import torch

from tests import slicehead_ref as R
from oracle import vit_ref as V


def rel(a, b):
    a = torch.as_tensor(a).detach().double().flatten(); b = torch.as_tensor(b).detach().double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("tag", ["gp1", "gp0"])
def test_oracle_reproduces_reference_slicehead(golden_dir, tag):
    z = np.load(os.path.join(golden_dir, "slicehead_small.npz"))
    cfg = V.ViT2DConfig(**json.loads(str(z[f"{tag}/cfg"])))
    P = R.init(cfg, seed=int(z["param_seed"]))
    x, tgt = R.inputs(cfg)
    assert torch.equal(x, torch.from_numpy(z["x"])) and torch.equal(tgt, torch.from_numpy(z["target"]))
    for t in P.values():
        t.requires_grad_(True)
    out, feats = R.forward(P, x, cfg)
    assert rel(feats, z[f"{tag}/features"]) <= 1e-5
    assert rel(out, z[f"{tag}/out"]) <= 1e-5
    loss = torch.nn.functional.cross_entropy(out, tgt)
    assert abs(float(loss.detach()) - float(z[f"{tag}/loss"])) <= 1e-5 * float(z[f"{tag}/loss"])
    loss.backward()
    for k in R.grad_keys(cfg):
        assert rel(R.sub(P[k].grad), z[f"{tag}/grad/{k}"]) <= 1e-5, k
        assert abs(float(P[k].grad.double().norm()) - float(z[f"{tag}/gnorm/{k}"])) <= 1e-5 * float(z[f"{tag}/gnorm/{k}"]) + 1e-12, k
