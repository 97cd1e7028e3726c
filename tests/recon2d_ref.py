"""Restatements of the 2-D half of the reference's validation pass, and the inputs of its tests.

``panels_nc``         get_visible_images_2d's chain (Pre-training/custom_util/misc.py:1134-1223) as plain tensor ops for C channels:
                      unpatchify of the prediction and of the mask expanded to elements, the grey level of both, the two blends.
                      int32 [N, 4, Tp, H, W, C].  The level is ``(int) clip(((v * scale) + shift) * 255, 0, 255)`` in fp32, every op
                      rounded on its own; scale 1 / shift 0 is untransform_image_no_normalization (:730-731) bit for bit (a product
                      with 1 and a sum with 0 round nothing).
``panels_nc_denorm``  the ``denorm`` variant in fp64 and the values of panel 2 before clip and truncation (tests/recon_ref.py's rule).
``white_border``      find_and_convert_large_white_region(image, 'tensor') (:1438-1484) restated per row from its first / last white
                      column, with the reference's own double comparisons and its torch expression for the threshold.

tests/golden/recon2d_small.npz holds what the reference's own functions give on the same inputs (tools/gen_golden_recon2d.py)."""
import os

import numpy as np
import torch

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ---------------------------------------------------------------------------------------------- panels
def level(v, scale=1.0, shift=0.0):
    """v [..., C] (channels last) or any shape with scalar scale / shift"""
    s = torch.as_tensor(scale, dtype=torch.float32)
    m = torch.as_tensor(shift, dtype=torch.float32)
    return torch.clip(((v.float() * s) + m) * 255, 0, 255).int()


def unpatchify(x, T, H, W, p, u, C):
    """[N, L, u*p*p*C] in the order (a < u, py, px, c < C) -> [N, T, H, W, C].  C = 1: models_mae.unpatchify; u = T = 1:
    models_mae_2d.unpatchify ('nhwpqc->nchpwq')."""
    N = x.shape[0]
    t, h, w = T // u, H // p, W // p
    x = x.reshape(N, t, h, w, u, p, p, C)
    x = torch.einsum("nthwupqc->ntuhpwqc", x)
    return x.reshape(N, T, H, W, C)


def patchify(imgs, p, u):
    """[N, C, T, H, W] -> [N, L, u*p*p*C] in the same order"""
    N, C, T, H, W = imgs.shape
    t, h, w = T // u, H // p, W // p
    x = imgs.reshape(N, C, t, u, h, p, w, p)
    x = torch.einsum("nctuhpwq->nthwupqc", x)
    return x.reshape(N, t * h * w, u * p * p * C)


def pred_frames(pred, imgs, u, p):
    H, W = imgs.shape[-2:]
    return pred.shape[1] // ((H // p) * (W // p)) * u


def _blend(x, vol, m):
    im_masked = x * (1 - m)
    im_paste = x * (1 - m) + vol * m
    return torch.stack([x.float(), im_masked, vol.float(), im_paste], dim=1).int()      # whole numbers in fp32: exact


def panels_nc(pred, imgs, mask, u, p, scale=1.0, shift=0.0):
    """pred [N, L, PD], imgs [N, C, T, H, W], mask [N, L] -> int32 [N, 4, Tp, H, W, C]; scale / shift: a scalar or C values"""
    N, C, T, H, W = imgs.shape
    Tp = pred_frames(pred, imgs, u, p)
    vol = level(unpatchify(pred, Tp, H, W, p, u, C), scale, shift)
    m = unpatchify(mask.unsqueeze(-1).repeat(1, 1, pred.shape[-1]), Tp, H, W, p, u, C)
    x = level(imgs[:, :, :Tp].permute(0, 2, 3, 4, 1), scale, shift)
    return _blend(x, vol, m)


def panels_nc_denorm(pred, imgs, mask, u, p, scale=1.0, shift=0.0):
    N, C, T, H, W = imgs.shape
    Tp = pred_frames(pred, imgs, u, p)
    target = patchify(imgs[:, :, :Tp].double(), p, u)
    mean = target.mean(dim=-1, keepdim=True)
    var = target.var(dim=-1, keepdim=True)                       # unbiased, over all PD elements, as the norm_pix branch of the loss
    pd = pred.double() * (var + 1.0e-6) ** 0.5 + mean
    s = torch.as_tensor(scale, dtype=torch.float32).double()     # the fp32 constants of the chain, in fp64 arithmetic
    mm = torch.as_tensor(shift, dtype=torch.float32).double()
    raw = (unpatchify(pd, Tp, H, W, p, u, C) * s + mm) * 255
    vol = torch.clip(raw, 0, 255).int()
    m = unpatchify(mask.unsqueeze(-1).repeat(1, 1, pred.shape[-1]), Tp, H, W, p, u, C)
    x = level(imgs[:, :, :Tp].permute(0, 2, 3, 4, 1), scale, shift)
    return _blend(x, vol, m), raw


def exact_class(raw, tol=1.0e-3):
    return (raw - raw.round()).abs() > tol


def edge_values(scale=1.0, shift=0.0):
    """For every level k the fp32 inputs around the one the chain maps to exactly k, two steps to either side.  1280 values."""
    k = np.arange(256, dtype=np.float64)
    v = ((k / 255 - shift) / scale).astype(np.float32)
    out = [v]
    lo, hi = v.copy(), v.copy()
    for _ in range(2):
        lo = np.nextafter(lo, np.float32(-np.inf)); hi = np.nextafter(hi, np.float32(np.inf))
        out += [lo.copy(), hi.copy()]
    return torch.from_numpy(np.stack(out, axis=1).reshape(-1).copy())


def make_inputs(seed, B, C, T, H, W, p, u, mask_ratio=0.75, lo=-0.2, hi=1.2, edges=None):
    """imgs [B, C, T, H, W] and pred [B, L, u*p*p*C] spread a little past both clip ends of the scale (values that half precision holds
    exactly, so that a fixture of them compresses), the first values of both replaced by ``edges``; mask [B, L] of 0 / 1."""
    g = torch.Generator().manual_seed(seed)
    L = (T // u) * (H // p) * (W // p)
    imgs = (torch.rand(B, C, T, H, W, generator=g) * (hi - lo) + lo).half().float()
    pred = (torch.rand(B, L, u * p * p * C, generator=g) * (hi - lo) + lo).half().float()
    if edges is not None:
        n = min(edges.numel(), imgs[0].numel(), pred[0].numel())
        imgs.view(-1)[:n] = edges[:n]
        pred.view(-1)[:n] = edges[torch.randperm(edges.numel(), generator=g)][:n]
    mask = (torch.rand(B, L, generator=g) < mask_ratio).float()
    return imgs, pred, mask


def load_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "recon2d_small.npz"))
    return {k: z[k] for k in z.files}


# name -> (imgs [B, C, T, H, W], pred, mask, u, p, scale, shift): the direct cases of tests/test_gpu_recon2d.py
def case(name, golden_dir=None):
    if name in ("rgb", "triplet"):
        # the fixture's numbers: ONE pair of tensors read as 2 RGB images of 32 x 32 and as 2 triplets of three 32 x 32 B-scans
        if golden_dir is None:
            imgs, pred, mask = make_inputs(40, B=2, C=3, T=1, H=32, W=32, p=16, u=1, edges=edge_values())
        else:
            z = load_fixture(golden_dir)
            imgs, pred, mask = (torch.from_numpy(z[k]) for k in ("imgs", "pred", "mask"))
        if name == "rgb":
            return imgs, pred, mask, 1, 16, 1.0, 0.0
        return imgs.reshape(2, 1, 3, 32, 32), pred, mask, 3, 16, 1.0, 0.0
    if name == "rgb_small":      # PD = 48: 12 float4 groups for 64 lanes; a 2 x 3 grid
        return (*make_inputs(41, B=3, C=3, T=1, H=8, W=12, p=4, u=1, edges=edge_values()), 1, 4, 1.0, 0.0)
    if name == "imagenet":       # Normalize-d inputs: about (v - mean) / std
        imgs, pred, mask = make_inputs(42, B=2, C=3, T=1, H=32, W=32, p=16, u=1, lo=-2.4, hi=2.9)
        e = torch.stack([edge_values(IMAGENET_STD[c], IMAGENET_MEAN[c]) for c in range(3)], dim=1)       # [1280, 3]: channel c's edges
        pred[0, 0] = e[:256].reshape(-1)               # one patch: 256 pixels, channels innermost
        pred[1, 1] = e[256:512].reshape(-1)
        imgs[0, :, 0] = e[:1024].t().reshape(3, 32, 32)
        return imgs, pred, mask, 1, 16, IMAGENET_STD, IMAGENET_MEAN
    if name == "grey_oct":       # C = 1 with the OCT mean / std: the levels of recon.hip's grey()
        return (*make_inputs(43, B=2, C=1, T=3, H=32, W=32, p=16, u=3, lo=-0.7, hi=2.9,
                             edges=edge_values(76.03 / 255, 45.79 / 255)), 3, 16, 76.03 / 255, 45.79 / 255)
    if name == "clip":           # far past both ends
        imgs, pred, mask = make_inputs(44, B=2, C=3, T=1, H=32, W=32, p=16, u=1, lo=-3.0, hi=4.0)
        return imgs, pred, mask, 1, 16, 1.0, 0.0
    if name == "cap":            # 65 x 16 x 16 = 16 640 tokens on 16 384 waves
        return (*make_inputs(45, B=65, C=3, T=1, H=64, W=64, p=4, u=1), 1, 4, 1.0, 0.0)
    raise KeyError(name)


def denorm_case(name):
    """A case with the prediction in per-patch standardised units (about zero mean, unit spread)."""
    imgs, pred, mask, u, p, scale, shift = case(name)
    return imgs, (pred - 0.5) / 0.4, mask, u, p, scale, shift


# ---------------------------------------------------------------------------------------------- border blanking
def white_border_limits(W):
    cols = range(W + 1)
    return (next(i for i in cols if i > 0.01 * W), next(i for i in cols if i > 0.05 * W),
            next(i for i in cols if not (i < W - 0.01 * W)), next(i for i in cols if not (i < W - 0.05 * W)))


def threshold(image):
    """The reference's own expression: a Python double times a 0-dim fp32 tensor is an fp32 product, then an fp32 difference."""
    max_val, min_val = torch.max(image), torch.min(image)
    return max_val - (255 - 240) / 255 * (max_val - min_val)


def white_border(image):
    """[T, H, W] or [H, W] -> (blanked image, region bool), both of the input's shape"""
    image = image.float()
    thresh = threshold(image)
    g = (image[0] if image.dim() == 3 else image).clone()
    white = (g > thresh).numpy()
    H, W = white.shape
    region = np.zeros((H, W), dtype=bool)
    for y in range(H):
        cols = np.flatnonzero(white[y])
        if cols.size == 0:
            continue
        f, l = int(cols[0]), int(cols[-1])
        if not (f > 0.01 * W):
            nw = np.flatnonzero(~white[y, f:])
            e = f + int(nw[0]) if nw.size else W
            region[y, f:e] = True
            if e < W and e > 0.05 * W:
                region[y, e:min(e + 5, W)] = True
        if not (l < W - 0.01 * W):
            nw = np.flatnonzero(~white[y, :l + 1])
            s = int(nw[-1]) if nw.size else None
            region[y, (0 if s is None else s + 1):l + 1] = True
            if s is not None and s < W - 0.05 * W and s <= 4:          # [s : s - 5] with a negative stop: up to W + s - 5
                region[y, s:W + s - 5] = True
    region = torch.from_numpy(region)
    g[region] = 0
    if image.dim() == 3:
        return g.unsqueeze(0).repeat(image.shape[0], 1, 1), region.unsqueeze(0).repeat(image.shape[0], 1, 1)
    return g, region


def _background(T, H, W):
    t, y, x = np.meshgrid(np.arange(T), np.arange(H), np.arange(W), indexing="ij")
    return (((x * 7 + y * 13 + t * 29) % 32) / 64.0).astype(np.float32)          # 0 .. 0.484, exact in half precision


def _paint(img, rows):
    """rows: {y: [(first, last, value), ...]} painted into frame 0"""
    for y, runs in rows.items():
        for a, b, v in runs:
            img[0, y, a:b + 1] = v
    return img


def threshold_extremes():
    """A (max, min) pair for which the threshold depends on HOW it is rounded: the separately rounded product and difference (the
    reference) differ from a fused multiply-add and from the same expression with the factor kept in double."""
    k32 = np.float32(15 / 255)
    mx = np.float32(0.0625)          # close to the product, so that the difference is exact and shows the product's rounding
    for i in range(2048, 4000):
        mn = np.float32(-i / 4096.0)
        gap = np.float32(mx - mn)
        sep = np.float32(mx - np.float32(k32 * gap))
        fused = np.float32(np.float64(mx) - np.float64(k32) * np.float64(gap))
        dbl = np.float32(np.float64(mx) - (15 / 255) * np.float64(gap))
        if sep != fused and sep != dbl:
            return float(mx), float(mn)
    raise AssertionError("no such pair")


WB_CASES = ("w128", "w64", "w100", "w512", "b2_second", "const", "nan", "thresh")


def wb_case(name):
    """The images of the blanking tests: [T, H, W] (or [H, W] for w100)."""
    if name in ("w128", "b2_second", "nan"):
        img = _paint(_background(3, 16, 128), {
            1: [(120, 127, 1.0)],                      # right band that stops at 119: [119 : 114] is empty
            2: [(124, 127, 1.0)],                      # ... at 123: not below 121.6
            3: [(0, 2, 1.0), (4, 127, 0.97)],          # full row, hole at 3: the negative stop, [3, 126)
            4: [(0, 4, 1.0), (6, 127, 1.0)],           # full row, hole at 5: empty slice, the hole stays
            5: [(1, 19, 0.99)],                        # first white at 1 (<= 1.28): followed, ends at 20 > 6.4: 20 .. 24 too
            6: [(2, 10, 1.0)],                         # first white at 2: not followed
            7: [(110, 126, 1.0)],                      # last white at 126 (< 126.72): not followed
            9: [(50, 60, 1.0)],                        # away from both edges
            10: [(0, 6, 1.0)],                         # ends at 7 > 6.4: 7 .. 11 too
            11: [(0, 5, 1.0)],                         # ends at 6 <= 6.4: no extension
            12: [(0, 127, 1.0)],                       # all white: e = W, s = none
            13: [(0, 0, 1.0), (127, 127, 1.0)],        # one pixel at either edge
            15: [(0, 3, 1.0), (30, 40, 1.0), (125, 127, 1.0)],
        })
        if name == "b2_second":                        # other extremes: max 0.75, min 0.25
            img = (img * 0.5 + 0.25).astype(np.float32)
        if name == "nan":
            img[0, 8, 77] = np.nan
        return torch.from_numpy(img)
    if name == "w64":                                  # 63 < 63.36: a right band is never followed
        return torch.from_numpy(_paint(_background(1, 8, 64), {y: [(56, 63, 1.0)] for y in (2, 3, 4, 5)}))
    if name == "w100":                                 # limits on integers: 1.0, 5.0, 99.0, 95.0; 25 lanes of a wave; a [H, W] input
        img = _paint(_background(1, 8, 100), {
            0: [(1, 10, 1.0)],                         # 1 > 1.0 is false: followed; ends at 11: 11 .. 15 too
            1: [(2, 10, 1.0)],                         # not followed
            2: [(0, 4, 1.0)],                          # ends at 5, 5 > 5.0 is false
            3: [(0, 5, 1.0)],                          # ends at 6: 6 .. 10 too
            4: [(90, 99, 1.0)],                        # 99 < 99.0 is false: followed
            5: [(90, 98, 1.0)],                        # not followed
            6: [(0, 1, 1.0), (3, 99, 1.0)],            # hole at 2: [2, 97)
            7: [(96, 99, 1.0)],                        # stops at 95, 95 < 95.0 is false
        })
        return torch.from_numpy(img[0])
    if name == "w512":                                 # limits 5.12, 25.6, 506.88, 486.4
        return torch.from_numpy(_paint(_background(1, 8, 512), {
            0: [(5, 30, 1.0)],                         # followed, extended
            1: [(6, 30, 1.0)],                         # not followed
            2: [(0, 24, 1.0)],                         # ends at 25: no extension
            3: [(0, 25, 1.0)],                         # ends at 26: 26 .. 30 too
            4: [(490, 507, 1.0)],                      # followed
            5: [(490, 506, 1.0)],                      # not followed
            6: [(0, 3, 1.0), (5, 511, 1.0)],           # hole at 4: [4, 511)
            7: [(487, 511, 1.0), (480, 485, 1.0)],     # stops at 486 (< 486.4, but the slice [486 : 481] is empty)
        }))
    if name == "const":
        return torch.full((3, 8, 64), 0.7)
    if name == "thresh":
        mx, mn = threshold_extremes()
        img = np.full((1, 4, 128), np.float32(0.5 * (mx + mn)), dtype=np.float32)
        img[0, 3, 60], img[0, 3, 61] = mx, mn
        th = np.float32(threshold(torch.from_numpy(img)))
        up = np.nextafter(th, np.float32(np.inf))
        img[0, 0, 0], img[0, 0, 1] = up, th            # white, then not: [0, 1) is marked
        img[0, 1, 0], img[0, 1, 1] = th, up            # not white, then white at 1 (<= 1.28): [1, 2) is marked
        img[0, 2, 0:3] = th                            # equal to the threshold: not white
        assert np.float32(threshold(torch.from_numpy(img))) == th
        return torch.from_numpy(img)
    raise KeyError(name)
