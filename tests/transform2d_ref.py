"""numpy restatement of Pillow's 8-bit bicubic resize (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc,
ImagingResampleHorizontal_8bpc / Vertical_8bpc) as torchvision's Resize / resized_crop call it for a PIL image with interpolation=3,
plus the float chain ToTensor -> Normalize.  float64 and int64 only, every operation rounded on its own (numpy never fuses a
multiply with an add), no torch in the resize.  tests/golden/image2d_small.npz (tools/gen_golden_image2d.py, written WITH Pillow) pins
it to Pillow bit for bit; the GPU tests compare the kernel with it.

Per axis (in = the crop's extent, the crop is taken first):  scale = in / out, support = 2 max(scale, 1), and for output index xx
  center = (xx + 0.5) scale;  xmin = max(int(center - support + 0.5), 0);  xmax = min(int(center + support + 0.5), in) - xmin
  w[x] = bicubic((x + xmin - center + 0.5) / max(scale, 1)), summed in tap order;  kk[x] = int(w[x] / sum * 2^22 +- 0.5)
A pass: clamp((2^21 + sum pixel kk) >> 22, 0, 255); horizontal first, rounded to uint8, then vertical over those values."""
import zlib

import numpy as np

PRECISION_BITS = 22
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def axis_coeffs(in_size: int, out_size: int):
    """(bounds int [out, 2] = (xmin, xmax), kk int64 [out, ksize]) of one axis."""
    scale = float(in_size) / float(out_size)
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = 2 * int(np.ceil(support)) + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), dtype=np.int64)
    kk = np.zeros((out_size, ksize), dtype=np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            k = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + k * (1 << PRECISION_BITS)) if k < 0 else int(0.5 + k * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _matrix(in_size, out_size):
    bounds, kk = axis_coeffs(in_size, out_size)
    m = np.zeros((out_size, in_size), dtype=np.int64)
    for xx, (xmin, xmax) in enumerate(bounds):
        m[xx, xmin:xmin + xmax] = kk[xx, :xmax]
    return m


def _clip8(acc, stats, key):
    v = (acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS          # numpy's >> on int64 is arithmetic, as C's on int
    if stats is not None:
        stats[key + "_below"] = stats.get(key + "_below", 0) + int((v < 0).sum())
        stats[key + "_above"] = stats.get(key + "_above", 0) + int((v > 255).sum())
    return np.clip(v, 0, 255).astype(np.uint8)


def resize(img: np.ndarray, size, crop=None, stats=None) -> np.ndarray:
    """uint8 [H, W] or [H, W, 3] -> uint8 [OH, OW(, 3)].  crop = (top, left, h, w): torchvision's resized_crop (crop, then resize).
    stats: a dict that receives how many sums of each pass left [0, 255] ("h_below", "h_above", "v_below", "v_above")."""
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    if crop is not None:
        t, l, h, w = crop
        img = img[t:t + h, l:l + w]
    OH, OW = size
    x = img.astype(np.int64)
    mh = _matrix(img.shape[1], OW)
    x = _clip8(np.tensordot(x, mh, axes=([1], [1])) if x.ndim == 2 else np.einsum("hwc,ow->hoc", x, mh), stats, "h").astype(np.int64)
    mv = _matrix(img.shape[0], OH)
    return _clip8(np.tensordot(mv, x, axes=([1], [0])), stats, "v")


def row_span(in_size: int, out_size: int, tile: int) -> int:
    """The longest run of input rows [xmin(first), xmin(last) + xmax(last)) over the tiles of `tile` output rows."""
    b, _ = axis_coeffs(in_size, out_size)
    return max(int(b[min(y0 + tile, out_size) - 1].sum() - b[y0, 0]) for y0 in range(0, out_size, tile))


def lut(mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """ToTensor -> Normalize on every grey level, with the reference's own ops: float32 [3, 256]."""
    import torch
    if not isinstance(mean, (tuple, list)):
        mean, std = (mean,) * 3, (std,) * 3
    g = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    return torch.stack([(g - mean[c]) / std[c] for c in range(3)])


def to_tensor_normalize(u8: np.ndarray, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """The float chain on a resized image: convert("RGB") -> ToTensor (HWC uint8 -> CHW float32 / 255) -> Normalize
    (tensor.sub_(mean[:, None, None]).div_(std[:, None, None])), as torchvision runs it: float32 [3, OH, OW]."""
    import torch
    if not isinstance(mean, (tuple, list)):
        mean, std = (mean,) * 3, (std,) * 3
    x = torch.from_numpy(np.ascontiguousarray(u8))
    if x.dim() == 2:
        x = x[:, :, None].expand(-1, -1, 3)
    x = x.permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    m = torch.tensor(mean, dtype=torch.float32)[:, None, None]
    s = torch.tensor(std, dtype=torch.float32)[:, None, None]
    return x.sub_(m).div_(s)


# ---- the cases of tests/golden/image2d_small.npz and of the GPU tests -------------------------------------------------------------------
# name -> (kind, seed, input shape, crop or None, (OH, OW)).  Inputs come from numpy's seeded PCG64 (a stable stream); the golden file
# stores each input's CRC-32 beside Pillow's output, so a changed stream is a loud failure, not a silent one.
def _cases():
    c = {}
    c["binary_37x53_to_64x32"] = ("binary", 1, (37, 53), None, (64, 32))
    c["binary_61x100_to_50x70"] = ("binary", 2, (61, 100), None, (50, 70))
    c["noise_70x90_to_8x8"] = ("noise", 3, (70, 90), None, (8, 8))
    c["noise_124x256_to_128x128"] = ("noise", 4, (124, 256), None, (128, 128))
    c["noise_64x64_to_64x48"] = ("noise", 5, (64, 64), None, (64, 48))
    c["noise_5x7_to_16x16"] = ("noise", 6, (5, 7), None, (16, 16))
    c["noise_1x1_to_3x2"] = ("noise", 7, (1, 1), None, (3, 2))
    c["noise_2x3_to_1x1"] = ("noise", 8, (2, 3), None, (1, 1))
    for cname, crop in (("inner", (23, 17, 237, 133)), ("first", (0, 0, 1, 1)), ("last", (299, 199, 1, 1)), ("whole", None)):
        for size in ((224, 224), (31, 33)):
            c[f"noise_300x200_{cname}_to_{size[0]}x{size[1]}"] = ("noise", 9, (300, 200), crop, size)
    c["rgb_37x53_to_64x32"] = ("noise", 10, (37, 53, 3), None, (64, 32))
    c["rgb_37x53_crop_to_64x32"] = ("noise", 10, (37, 53, 3), (5, 9, 20, 31), (64, 32))
    for i in range(3):
        c[f"stack{i}_37x53_to_64x32"] = ("noise", 20 + i, (37, 53), None, (64, 32))
        c[f"rgbstack{i}_37x53_to_64x32"] = ("noise", 30 + i, (37, 53, 3), None, (64, 32))
    return c


CASES = _cases()


def case_input(name: str) -> np.ndarray:
    kind, seed, shape, _, _ = CASES[name]
    g = np.random.Generator(np.random.PCG64(seed))
    a = g.integers(0, 256, size=shape, dtype=np.uint8)
    return np.where(a < 128, 0, 255).astype(np.uint8) if kind == "binary" else a


def crc(a: np.ndarray) -> int:
    return zlib.crc32(np.ascontiguousarray(a).tobytes())
