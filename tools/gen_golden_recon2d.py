#!/usr/bin/env python3
"""Generate tests/golden/recon2d_small.npz from the REAL reference (build container only; the reference never travels to a GPU box).

    python tools/gen_golden_recon2d.py

What runs from the reference's own source:
  find_and_convert_large_white_region   Pre-training/custom_util/misc.py:1438-1484, on every image of tests/recon2d_ref.wb_case
  untransform_image_no_normalization    :730-731
  unpatchify                            OCTCube/models_mae.py:110-122 (the 2-D MAE, three channels) and
                                        Pre-training/models_mae_joint_res_flash_attn.py:316-334 (the joint model's B-scan triplets)
The lines between them are get_visible_images_2d's (:1186-1198: the mask expanded to elements, the two blends), whose matplotlib part
cannot run here.  The reference's un-vendored imports are shimmed as tools/gen_golden_recon.py does.

Cases (tests/test_gpu_recon2d.py; the inputs come from tests/recon2d_ref and are stored in the file):
  rgb       B = 2 RGB images of 32 x 32, p = 16: panels [2, 4, 32, 32, 3]
  triplet   the same numbers read as 2 triplets of three 32 x 32 B-scans, u = 3: panels [2, 4, 3, 32, 32]
  wb_*      the blanking images of recon2d_ref.WB_CASES: the input, the returned image and the returned region
"""
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from tools.gen_golden_recon import load_reference  # noqa: E402

OC_MODEL = "/root/reference/OCTCube/models_mae.py"


def load_2d_model():
    """OCTCube/models_mae.py under a name of its own (Pre-training has a module of the same name)."""
    oc = os.path.dirname(OC_MODEL)
    for m_ in [k for k in list(sys.modules) if k == "util" or k.startswith("util.")]:
        del sys.modules[m_]
    sys.path.insert(0, oc)
    spec = importlib.util.spec_from_file_location("ref_octcube_models_mae", OC_MODEL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sys.path.remove(oc)
    return mod


def blend(rmisc, frames, masks, samples):
    """get_visible_images_2d :1186-1198 per image, on what unpatchify returned"""
    out = []
    for i in range(frames.shape[0]):
        frame_i = rmisc.untransform_image_no_normalization(frames[i].squeeze())
        m = masks[i].squeeze()
        x = rmisc.untransform_image_no_normalization(samples[i].squeeze())
        im_masked = x * (1 - m)
        im_paste = x * (1 - m) + frame_i * m
        out.append(torch.stack([x.float(), im_masked, frame_i.float(), im_paste]))
    out = torch.stack(out)
    assert torch.equal(out, out.round()) and int(out.min()) >= 0 and int(out.max()) <= 255
    return out.to(torch.uint8)


def main():
    from tests import recon2d_ref as R
    rmisc, rjoint = load_reference()
    r2d = load_2d_model()
    out = {}
    # ---- panels
    imgs, pred, mask, u, p, _, _ = R.case("rgb")
    out.update(imgs=imgs.numpy(), pred=pred.numpy(), mask=mask.numpy())
    me = types.SimpleNamespace(patch_embed=types.SimpleNamespace(patch_size=(p, p)))
    frames = r2d.MaskedAutoencoderViT.unpatchify(me, pred)                                     # [N, 3, H, W]
    masks = r2d.MaskedAutoencoderViT.unpatchify(me, mask.unsqueeze(-1).repeat(1, 1, pred.shape[-1]))
    rgb = blend(rmisc, frames, masks, imgs[:, :, 0])                                           # [N, 4, 3, H, W]
    out["panels_rgb"] = rgb.permute(0, 1, 3, 4, 2).contiguous().numpy()                        # channels last
    imgs3, pred, mask, u, p, _, _ = R.case("triplet")
    N, _, T, H, W = imgs3.shape
    me = types.SimpleNamespace(in_chans=1, patch_info=(N, T, H, W, p, u, T // u, H // p, W // p))
    with contextlib.redirect_stdout(io.StringIO()):                                            # unpatchify prints its shapes
        frames = rjoint.MaskedAutoencoderViT.unpatchify(me, pred, high_res=False)
        masks = rjoint.MaskedAutoencoderViT.unpatchify(me, mask.unsqueeze(-1).repeat(1, 1, pred.shape[-1]), high_res=False)
    out["panels_triplet"] = blend(rmisc, frames, masks, imgs3).numpy()                         # [N, 4, 3, H, W]
    # ---- blanking
    for name in R.WB_CASES:
        image = R.wb_case(name)
        got, region = rmisc.find_and_convert_large_white_region(image.clone(), "tensor")
        assert got.shape == image.shape and region.shape == image.shape and region.dtype == torch.bool
        out[f"wb_{name}_in"], out[f"wb_{name}_out"], out[f"wb_{name}_region"] = image.numpy(), got.numpy(), region.numpy()
        print(f"{name}: {tuple(image.shape)}, {int(region.sum())} marked, threshold {float(R.threshold(image)):.9g}")
    path = os.path.join(ROOT, "tests", "golden", "recon2d_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
