#!/usr/bin/env python3
"""Generate tests/golden/recon_small.npz from the REAL reference (build container only; the reference never travels to a GPU box).

    python tools/gen_golden_recon.py

What runs from the reference's own source: ``untransform_image`` (Pre-training/custom_util/misc.py:727-728) and the model's
``unpatchify`` (Pre-training/models_mae_joint_res_flash_attn.py:316-334); the lines between them are get_visible_images' (:1233-1274:
mask expanded to pixels, index_select of the frames, the two blends), whose matplotlib part cannot run here.  The reference's
un-vendored imports are shimmed as oracle/gen_golden.py does, plus psutil / matplotlib, which only its logging and plotting touch.

Cases (tests/test_gpu_recon.py (a) and (b); the inputs come from tests/recon_ref.make_inputs and are stored in the file):
  a   B=2, T=6, H=W=32, p=16, u=3, every frame predicted
  b   the same pred / mask on a T=9 volume of which pred_t_dim=6 frames are predicted: linspace(0, 8, 6).long() = [0, 1, 3, 4, 6, 8]
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
REF = "/root/reference/Pre-training"


def load_reference():
    from oracle.gen_golden import install_shims
    install_shims()
    for name in ("psutil", "matplotlib", "matplotlib.pyplot"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    if "matplotlib.pyplot" in sys.modules and not hasattr(sys.modules["matplotlib"], "pyplot"):
        sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.path.insert(0, REF)
    import custom_util.misc as rmisc
    import models_mae_joint_res_flash_attn as rmodel
    return rmisc, rmodel


def reference_panels(rmisc, rmodel, pred, imgs, mask, pred_t_dim, u, p):
    N, _, T, H, W = imgs.shape
    L = pred.shape[1]
    t, h, w = L // ((H // p) * (W // p)), H // p, W // p
    actual_t_dim = t * u
    me = types.SimpleNamespace(in_chans=1, patch_info=(N, T, H, W, p, u, t, h, w))       # what patchify leaves behind (:312)
    with contextlib.redirect_stdout(io.StringIO()):                                      # unpatchify prints its shapes
        volumes = rmodel.MaskedAutoencoderViT.unpatchify(me, pred, high_res=False, actual_t_dim=actual_t_dim)
        masks = mask.unsqueeze(-1).repeat(1, 1, pred.shape[-1])
        masks = rmodel.MaskedAutoencoderViT.unpatchify(me, masks, high_res=False, actual_t_dim=actual_t_dim)
    samples = torch.index_select(imgs, 2, torch.linspace(0, imgs.shape[2] - 1, pred_t_dim).long())
    out = []
    for i in range(N):
        vol_i = rmisc.untransform_image(volumes[i].squeeze())
        m = masks[i].squeeze()
        x = rmisc.untransform_image(samples[i].squeeze())
        im_masked = x * (1 - m)
        im_paste = x * (1 - m) + vol_i * m
        out.append(torch.stack([x.float(), im_masked, vol_i.float(), im_paste]))
    out = torch.stack(out)
    assert torch.equal(out, out.round()) and int(out.min()) >= 0 and int(out.max()) <= 255
    return out.to(torch.uint8).numpy()


def main():
    from tests import recon_ref as R
    rmisc, rmodel = load_reference()
    assert rmisc.IMG_MEAN == R.IMG_MEAN and rmisc.IMG_STD == R.IMG_STD
    imgs9, pred, mask = R.make_inputs(seed=20, B=2, T=9, H=32, W=32, p=16, u=3, Tp=6)
    imgs6 = imgs9[:, :, :6].contiguous()
    exp_a = reference_panels(rmisc, rmodel, pred, imgs6, mask, 6, 3, 16)
    exp_b = reference_panels(rmisc, rmodel, pred, imgs9, mask, 6, 3, 16)
    path = os.path.join(ROOT, "tests", "golden", "recon_small.npz")
    np.savez_compressed(path, imgs9=imgs9.numpy(), pred=pred.numpy(), mask=mask.numpy(), u=3, p=16,
                        frame_idx_b=torch.linspace(0, 8, 6).long().numpy().astype(np.int32), panels_a=exp_a, panels_b=exp_b)
    print(path, os.path.getsize(path), "bytes; grey range", exp_a.min(), exp_a.max())


if __name__ == "__main__":
    main()
