"""Torch restatement of the reference's reconstruction dump (Pre-training/custom_util/misc.py:1225-1299 get_visible_images): unpatchify
of the prediction and of the mask expanded to pixels (models_mae_joint_res_flash_attn.py:316-334), index_select of the frames the
prediction stands for, untransform_image (:727-728) of both, the two blends.  Plain tensor ops on whatever device the inputs live on;
tests/golden/recon_small.npz holds what the reference's own functions give on the same inputs (tools/gen_golden_recon.py).

``panels``         the chain as the reference runs it (fp32, every op rounded on its own): int32 [N, 4, Tp, H, W]
``panels_denorm``  the ``denorm`` variant in fp64: the prediction mapped back from per-patch standardised units first; returns the
                   panels and the fp64 values of panel 2 before clip and truncation (how far each is from an integer decides whether a
                   fp32 computation must reproduce the grey level exactly)"""
import torch

IMG_MEAN = 45.79 / 255
IMG_STD = 76.03 / 255


def untransform_image(image):
    return torch.clip((image.float() * IMG_STD + IMG_MEAN) * 255, 0, 255).int()


def unpatchify(x, T, H, W, p, u):
    """[N, L, u*p*p] -> [N, 1, T, H, W], L = (T/u)(H/p)(W/p)"""
    N = x.shape[0]
    t, h, w = T // u, H // p, W // p
    x = x.reshape(shape=(N, t, h, w, u, p, p, 1))
    x = torch.einsum("nthwupqc->nctuhpwq", x)
    return x.reshape(shape=(N, 1, T, H, W))


def patchify(imgs, p, u):
    """[N, 1, T, H, W] -> [N, L, u*p*p]"""
    N, _, T, H, W = imgs.shape
    t, h, w = T // u, H // p, W // p
    x = imgs.reshape(shape=(N, 1, t, u, h, p, w, p))
    x = torch.einsum("nctuhpwq->nthwupqc", x)
    return x.reshape(shape=(N, t * h * w, p * p * u))


def pred_frames(pred, imgs, u, p):
    H, W = imgs.shape[-2:]
    return pred.shape[1] // ((H // p) * (W // p)) * u


def select_frames(imgs, frame_idx, Tp):
    if frame_idx is None:
        return imgs[:, :, :Tp]
    return torch.index_select(imgs, 2, frame_idx.long().to(imgs.device))


def _blend(x, vol, m):
    im_masked = x * (1 - m)
    im_paste = x * (1 - m) + vol * m
    return torch.stack([x.float(), im_masked, vol.float(), im_paste], dim=1).int()      # whole numbers in fp32: exact


def panels(pred, imgs, mask, frame_idx, u, p):
    H, W = imgs.shape[-2:]
    Tp = pred_frames(pred, imgs, u, p)
    vol = untransform_image(unpatchify(pred, Tp, H, W, p, u)[:, 0])
    m = unpatchify(mask.unsqueeze(-1).repeat(1, 1, pred.shape[-1]), Tp, H, W, p, u)[:, 0]
    x = untransform_image(select_frames(imgs, frame_idx, Tp)[:, 0])
    return _blend(x, vol, m)


def panels_denorm(pred, imgs, mask, frame_idx, u, p):
    H, W = imgs.shape[-2:]
    Tp = pred_frames(pred, imgs, u, p)
    sel = select_frames(imgs, frame_idx, Tp)
    target = patchify(sel.double(), p, u)
    mean = target.mean(dim=-1, keepdim=True)
    var = target.var(dim=-1, keepdim=True)                       # unbiased, as the norm_pix branch of the loss
    pd = pred.double() * (var + 1.0e-6) ** 0.5 + mean
    s = float(torch.tensor(IMG_STD, dtype=torch.float32))        # the fp32 constants of the chain, in fp64 arithmetic
    mm = float(torch.tensor(IMG_MEAN, dtype=torch.float32))
    raw = (unpatchify(pd, Tp, H, W, p, u)[:, 0] * s + mm) * 255
    vol = torch.clip(raw, 0, 255).int()
    m = unpatchify(mask.unsqueeze(-1).repeat(1, 1, pred.shape[-1]), Tp, H, W, p, u)[:, 0]
    x = untransform_image(sel[:, 0])
    return _blend(x, vol, m), raw


# ---------------------------------------------------------------------------------------------- inputs of the tests and of the fixture
def edge_values():
    """For every grey level k the fp32 inputs around the one the chain maps to exactly k, two steps to either side: where the truncation
    flips, i.e. where one rounding more or less in (v * s + m) * 255 shows as another grey level.  1280 values."""
    import numpy as np
    k = np.arange(256, dtype=np.float64)
    v = ((k / 255 - IMG_MEAN) / IMG_STD).astype(np.float32)
    out = [v]
    lo, hi = v.copy(), v.copy()
    for _ in range(2):
        lo = np.nextafter(lo, np.float32(-np.inf)); hi = np.nextafter(hi, np.float32(np.inf))
        out += [lo.copy(), hi.copy()]
    return torch.from_numpy(np.stack(out, axis=1).reshape(-1).copy())


def make_inputs(seed, B, T, H, W, p, u, Tp, mask_ratio=0.75, edges=True):
    """imgs [B, 1, T, H, W] and pred [B, L, u*p*p] spread a little past both clip ends of the grey scale (values that half precision
    holds exactly, so that a fixture of them compresses), the first values of both replaced by ``edge_values``; mask [B, L] of 0 / 1."""
    g = torch.Generator().manual_seed(seed)
    L = (Tp // u) * (H // p) * (W // p)
    imgs = (torch.rand(B, 1, T, H, W, generator=g) * 3.6 - 0.7).half().float()
    pred = (torch.rand(B, L, u * p * p, generator=g) * 3.6 - 0.7).half().float()
    if edges:
        e = edge_values()
        n = min(e.numel(), imgs[0].numel(), pred[0].numel())
        imgs.view(-1)[:n] = e[:n]
        pred.view(-1)[:n] = e[torch.randperm(e.numel(), generator=g)][:n]
    mask = (torch.rand(B, L, generator=g) < mask_ratio).float()
    return imgs, pred, mask


def load_fixture(golden_dir):
    import os
    import numpy as np
    z = np.load(os.path.join(golden_dir, "recon_small.npz"))
    return {k: (torch.from_numpy(z[k]) if z[k].ndim else int(z[k])) for k in z.files}


# name -> (imgs, pred, mask, frame_idx, u, p): the direct-kernel cases of tests/test_gpu_recon.py; (a) and (b) are the fixture's inputs
def case(name, golden_dir):
    if name in ("a", "b"):
        z = load_fixture(golden_dir)
        if name == "a":
            return z["imgs9"][:, :, :6].contiguous(), z["pred"], z["mask"], None, z["u"], z["p"]
        return z["imgs9"], z["pred"], z["mask"], z["frame_idx_b"], z["u"], z["p"]
    if name == "c":      # T = 3: one token layer, the 512^2 B-scan branch by shape
        return (*make_inputs(31, B=2, T=3, H=64, W=64, p=16, u=3, Tp=3), None, 3, 16)
    if name == "d":      # PD = 16: 4 float4 groups for 64 lanes; a 2 x 3 grid
        return (*make_inputs(32, B=3, T=5, H=8, W=12, p=4, u=1, Tp=5), None, 1, 4)
    if name == "e":      # 3 tokens: the fourth wave of the only workgroup has no token
        return (*make_inputs(33, B=1, T=9, H=16, W=16, p=16, u=3, Tp=9), None, 3, 16)
    raise KeyError(name)


def denorm_case(name, golden_dir):
    """Case (a) / (d) with the prediction in per-patch standardised units (about zero mean, unit spread)."""
    imgs, pred, mask, fi, u, p = case(name, golden_dir)
    return imgs, (pred - 1.1) / 1.04, mask, fi, u, p


def exact_class(raw, tol=1.0e-3):
    """Voxels whose fp64 value before clip and truncation is farther than ``tol`` from an integer: a fp32 chain (error: a few ulp of
    255, about 1e-4) must give exactly the fp64 grey level there."""
    return (raw - raw.round()).abs() > tol
