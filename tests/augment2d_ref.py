"""numpy restatement of the Pillow operations behind the reference's RandAugment (OCTCube/util/rand_augment.py: NAME_TO_OP), on uint8
[H, W, 3] images.  float64 / float32 / int64 only, every operation rounded on its own (numpy never fuses a multiply with an add).
tests/golden/augment2d_small.npz (tools/gen_golden_augment2d.py, written WITH Pillow through the reference's own file) pins it to Pillow
bit for bit; the GPU tests compare csrc/augment2d.hip with it.

  convert("L")        L = (R 19595 + G 38470 + B 7471 + 0x8000) >> 16
  Image.blend         in1 + alpha (in2 - in1) in C float; truncated for alpha in [0, 1], clipped to [0, 255] and truncated outside
  ImageEnhance        blend(degenerate, image, factor); degenerate = black (Brightness), the grey int(mean(L) + 0.5) (Contrast), L
                      replicated (Color), the 3 x 3 SMOOTH filter (Sharpness)
  ImageFilter.SMOOTH  float weights (1 1 1 / 1 5 1 / 1 1 1) / 13 summed row by row FROM THE ROW BELOW UPWARDS onto 0.5, clipped and
                      truncated; the one-pixel border is copied
  ImageOps            autocontrast, equalize, posterize, solarize, invert: 256-entry tables per channel
  Image.transform     AFFINE with a filter (Geometry.c: ImagingGenericTransform, affine_transform, bilinear / bicubic_filter32RGB)
  Image.rotate        its matrix, rounded to 15 places, about (w / 2, h / 2); an angle of 0 is a copy
"""
import math
import zlib

import numpy as np

BILINEAR, BICUBIC = 2, 3            # Pillow's Image.Resampling numbers
FILL = (128, 128, 128)
GEOMETRIC = ("Rotate", "ShearX", "ShearY", "TranslateX", "TranslateY", "TranslateXRel", "TranslateYRel")
NEEDS_STATS = ("AutoContrast", "Equalize", "Contrast", "ContrastIncreasing")


# ---- statistics --------------------------------------------------------------------------------------------------------------------------
def to_l(img: np.ndarray) -> np.ndarray:
    x = img.astype(np.int64)
    return ((x[..., 0] * 19595 + x[..., 1] * 38470 + x[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def stats(img: np.ndarray) -> np.ndarray:
    """uint32 [4, 256]: the histograms of R, G, B and L."""
    planes = [img[..., 0], img[..., 1], img[..., 2], to_l(img)]
    return np.stack([np.bincount(p.reshape(-1), minlength=256) for p in planes]).astype(np.uint32)


# ---- the blend ---------------------------------------------------------------------------------------------------------------------------
def blend(in1: np.ndarray, in2: np.ndarray, alpha) -> np.ndarray:
    """ImagingBlend (Blend.c) on uint8 arrays with alpha as a C float."""
    a = np.float32(alpha)
    if a == np.float32(1.0):
        return in2.copy()
    if a == np.float32(0.0):
        return in1.copy()
    d = (in2.astype(np.int32) - in1.astype(np.int32)).astype(np.float32)
    t = in1.astype(np.float32) + a * d
    if np.float32(0.0) <= a <= np.float32(1.0):
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


# factors inside [0, 1], on both sides of 1 (the clipping branch), next to 1, and the two copy shortcuts
BLEND_FACTORS = (0.1, 0.37, 0.5, 0.999, 1.0, 1.0000001, 1.001, 1.45, 1.9, 0.0, 0.9999999, -0.25, 2.5)


def blend_pairs():
    """(in1, in2): uint8 [256, 256] holding every pair of bytes once."""
    in1, in2 = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    return np.ascontiguousarray(in1), np.ascontiguousarray(in2)


# ---- tables ------------------------------------------------------------------------------------------------------------------------------
_LEVELS = np.arange(256, dtype=np.uint8)


def _same(t):
    return np.stack([t, t, t]).astype(np.uint8)


def lut_invert():
    return _same(255 - _LEVELS)


def lut_posterize(bits: int):
    if bits >= 8:
        return _same(_LEVELS)
    return _same(_LEVELS & np.uint8((~(2 ** (8 - bits) - 1)) & 0xFF))


def lut_solarize(thresh: int):
    i = _LEVELS.astype(np.int64)
    return _same(np.where(i < thresh, i, 255 - i))


def lut_solarize_add(add: int, thresh: int = 128):
    i = _LEVELS.astype(np.int64)
    return _same(np.where(i < thresh, np.minimum(255, i + add), i))


def lut_brightness(factor):
    return _same(blend(np.zeros(256, np.uint8), _LEVELS, factor))


def contrast_mean(hist_l) -> int:
    s = 0.0
    for j in range(256):
        s += j * int(hist_l[j])
    return int(s / int(np.sum(hist_l, dtype=np.int64)) + 0.5)


def lut_contrast(factor, hist):
    return _same(blend(np.full(256, contrast_mean(hist[3]), np.uint8), _LEVELS, factor))


def lut_autocontrast(hist):
    out = []
    for c in range(3):
        nz = np.nonzero(hist[c])[0]
        lo, hi = int(nz[0]), int(nz[-1])
        if hi <= lo:
            out.append(_LEVELS.copy())
            continue
        scale = 255.0 / (hi - lo)
        offset = -lo * scale
        out.append(np.array([min(max(int(ix * scale + offset), 0), 255) for ix in range(256)], np.uint8))
    return np.stack(out)


def lut_equalize(hist):
    out = []
    for c in range(3):
        h = [int(v) for v in hist[c]]
        histo = [v for v in h if v]
        step = (sum(histo) - histo[-1]) // 255 if len(histo) > 1 else 0
        if not step:
            out.append(_LEVELS.copy())
            continue
        n, t = step // 2, []
        for i in range(256):
            t.append(min(n // step, 255))       # the table's entries are clipped to a byte where Pillow reads the list
            n += h[i]
        out.append(np.array(t, np.uint8))
    return np.stack(out)


def apply_lut(img, table):
    return np.stack([table[c][img[..., c]] for c in range(3)], axis=-1)


# ---- colour and sharpness ------------------------------------------------------------------------------------------------------------------
def color(img, factor):
    l = to_l(img)
    return blend(np.stack([l, l, l], axis=-1), img, factor)


def smooth(img):
    """ImageFilter.SMOOTH: Filter.c's 3 x 3 path."""
    H, W = img.shape[:2]
    out = img.copy()
    if H < 3 or W < 3:
        return out
    k1, k5 = np.float32(1.0) / np.float32(13.0), np.float32(5.0) / np.float32(13.0)
    x = img.astype(np.float32)

    def row(r, kc):         # pixel[-1] k0 + pixel[0] k1 + pixel[+1] k2 of rows r of the interior columns
        return x[r, 0:W - 2] * k1 + x[r, 1:W - 1] * kc + x[r, 2:W] * k1
    ss = np.float32(0.5) + row(slice(2, H), k1)
    ss = ss + row(slice(1, H - 1), k5)
    ss = ss + row(slice(0, H - 2), k1)
    out[1:H - 1, 1:W - 1] = np.where(ss <= 0, 0, np.where(ss >= 255, 255, ss.astype(np.int32))).astype(np.uint8)
    return out


def sharpness(img, factor):
    return blend(smooth(img), img, factor)


# ---- the affine transform ------------------------------------------------------------------------------------------------------------------
def rotate_matrix(W: int, H: int, degrees: float):
    """Image.rotate's matrix; None where it takes the copy shortcut (an angle of 0 modulo 360)."""
    angle = degrees % 360.0
    if angle == 0:
        return None
    assert angle not in (90, 180, 270), "Image.rotate transposes here; RandAugment's +-30 degrees never does"
    cx, cy = W / 2, H / 2
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    x, y = -cx, -cy
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def op_matrix(name: str, arg: float, W: int, H: int):
    if name == "Rotate":
        return rotate_matrix(W, H, arg)
    if name == "ShearX":
        return (1, arg, 0, 0, 1, 0)
    if name == "ShearY":
        return (1, 0, 0, arg, 1, 0)
    if name in ("TranslateX", "TranslateXRel"):
        return (1, 0, arg * W if name.endswith("Rel") else arg, 0, 1, 0)
    if name in ("TranslateY", "TranslateYRel"):
        return (1, 0, 0, 0, 1, arg * H if name.endswith("Rel") else arg)
    raise KeyError(name)


def _floor(v):
    return np.where(v < 0.0, np.floor(v), np.trunc(v)).astype(np.int64)


def affine(img, m, interp, fill=FILL):
    H, W = img.shape[:2]
    m = [float(v) for v in m]
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64) + 0.5, np.arange(W, dtype=np.float64) + 0.5, indexing="ij")
    xin = m[0] * xs + m[1] * ys + m[2]
    yin = m[3] * xs + m[4] * ys + m[5]
    inside = ~((xin < 0.0) | (xin >= W) | (yin < 0.0) | (yin >= H))
    xin, yin = xin - 0.5, yin - 0.5
    x, y = _floor(xin), _floor(yin)
    dx, dy = (xin - x)[..., None], (yin - y)[..., None]
    src = img.astype(np.float64)

    def px(yy, xx):
        return src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
    if interp == BILINEAR:
        def line(yy):
            a, b = px(yy, x), px(yy, x + 1)
            return a + (b - a) * dx
        v1, v2 = line(y), line(y + 1)
        v = v1 + (v2 - v1) * dy
        res = v.astype(np.int64)            # (UINT8)v: no overshoot to clip
    elif interp == BICUBIC:
        def cubic(v1, v2, v3, v4, d):
            p1 = v2
            p2 = -v1 + v3
            p3 = 2 * (v1 - v2) + v3 - v4
            p4 = -v1 + v2 - v3 + v4
            return p1 + d * (p2 + d * (p3 + d * p4))

        def line(yy):
            return cubic(px(yy, x - 1), px(yy, x), px(yy, x + 1), px(yy, x + 2), dx)
        v = cubic(line(y - 1), line(y), line(y + 1), line(y + 2), dy)
        res = np.where(v <= 0.0, 0, np.where(v >= 255.0, 255, v.astype(np.int64)))
    else:
        raise ValueError(interp)
    out = np.empty_like(img)
    out[...] = np.array(fill, np.uint8)
    out[inside] = res[inside].astype(np.uint8)
    return out


# ---- one op by the reference's name ----------------------------------------------------------------------------------------------------------
def apply(img: np.ndarray, name: str, args=(), interp=BICUBIC, fill=FILL) -> np.ndarray:
    """What NAME_TO_OP[name](Image.fromarray(img), *args, resample=interp, fillcolor=fill) returns."""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    H, W = img.shape[:2]
    base = name[:-len("Increasing")] if name.endswith("Increasing") else name
    if name in GEOMETRIC:
        m = op_matrix(name, args[0], W, H)
        return img.copy() if m is None else affine(img, m, interp, fill)
    if base == "AutoContrast":
        return apply_lut(img, lut_autocontrast(stats(img)))
    if base == "Equalize":
        return apply_lut(img, lut_equalize(stats(img)))
    if base == "Invert":
        return apply_lut(img, lut_invert())
    if base in ("Posterize", "PosterizeOriginal"):
        return apply_lut(img, lut_posterize(args[0]))
    if base == "Solarize":
        return apply_lut(img, lut_solarize(args[0]))
    if base == "SolarizeAdd":
        return apply_lut(img, lut_solarize_add(args[0]))
    if base == "Brightness":
        return apply_lut(img, lut_brightness(args[0]))
    if base == "Contrast":
        return apply_lut(img, lut_contrast(args[0], stats(img)))
    if base == "Color":
        return color(img, args[0])
    if base == "Sharpness":
        return sharpness(img, args[0])
    raise KeyError(name)


def apply_chain(img, decisions, fill=FILL):
    """decisions: the drawn list of one image, [(name, args, interp), ...]."""
    for name, args, interp in decisions:
        img = apply(img, name, args, interp, fill)
    return img


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
INPUT_KINDS = ("noise", "lowcontrast", "constant", "binary", "ramp")


def make_input(kind: str, seed: int, H: int, W: int) -> np.ndarray:
    """Seeded inputs that make the rules bite: uniform noise alone leaves AutoContrast an identity (every channel holds 0 and 255)."""
    g = np.random.Generator(np.random.PCG64(seed))
    if kind == "noise":
        return g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "lowcontrast":           # values in [40, 200], another range per channel
        lo = np.array([40, 55, 70])
        hi = np.array([200, 180, 160])
        return (lo + g.integers(0, 1 << 30, (H, W, 3)) % (hi - lo + 1)).astype(np.uint8)
    if kind == "constant":
        return np.broadcast_to(g.integers(0, 256, 3, dtype=np.uint8), (H, W, 3)).copy()
    if kind == "binary":                # bicubic overshoots into both clips
        return np.where(g.integers(0, 256, (H, W, 3)) < 128, 0, 255).astype(np.uint8)
    if kind == "ramp":
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        return np.stack([(xx * 255) // max(W - 1, 1), (yy * 255) // max(H - 1, 1), ((xx + yy) * 3) % 256], axis=-1).astype(np.uint8)
    raise KeyError(kind)


def crc(a: np.ndarray) -> int:
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


# ---- the cases of tests/golden/augment2d_small.npz ------------------------------------------------------------------------------------------
# The boundary arguments of every op (the ranges rand-m*-inc* can draw from) and values inside them.
SWEEP_ARGS = {
    "AutoContrast": [()], "Equalize": [()], "Invert": [()],
    "Rotate": [(0.0,), (30.0,), (-30.0,), (7.3,), (-0.001,)],
    "ShearX": [(0.3,), (-0.3,), (0.111,)], "ShearY": [(0.3,), (-0.3,), (-0.07,)],
    "TranslateXRel": [(0.0,), (0.45,), (-0.45,), (0.2137,)], "TranslateYRel": [(0.0,), (0.45,), (-0.45,), (-0.3001,)],
    "TranslateX": [(0.0,), (100.0,), (-3.7,)], "TranslateY": [(0.0,), (-100.0,), (5.25,)],
    "Posterize": [(b,) for b in (0, 1, 2, 3, 4, 8)],
    "Solarize": [(t,) for t in (0, 1, 128, 255, 256)],
    "SolarizeAdd": [(a,) for a in (0, 57, 110)],
    "Color": [(f,) for f in (0.1, 0.55, 1.0, 1.45, 1.9)], "Contrast": [(f,) for f in (0.1, 0.55, 1.0, 1.45, 1.9)],
    "Brightness": [(f,) for f in (0.1, 0.55, 1.0, 1.45, 1.9)], "Sharpness": [(f,) for f in (0.1, 0.55, 1.0, 1.45, 1.9)],
}
SWEEP_INPUTS = [("noise", 37, 53), ("lowcontrast", 37, 53), ("constant", 5, 9), ("noise", 8, 8), ("binary", 37, 53), ("ramp", 64, 64),
                ("noise", 1, 1), ("lowcontrast", 2, 7), ("binary", 3, 3), ("lowcontrast", 65, 130)]
# full outputs: one case per op and interpolation, on the input that makes the op's rule bite
FULL_CASES = {}
for _n in SWEEP_ARGS:
    _kind = "binary" if _n in GEOMETRIC else "lowcontrast"
    for _i in ((BILINEAR, BICUBIC) if _n in GEOMETRIC else (BICUBIC,)):
        FULL_CASES[f"{_n}_{_i}"] = (_n, SWEEP_ARGS[_n][1 if len(SWEEP_ARGS[_n]) > 1 else 0], _i, (_kind, 24, 20))


def sweep_cases():
    """(key, name, args, interp, (kind, H, W)) of every swept combination."""
    for ii, (kind, H, W) in enumerate(SWEEP_INPUTS):
        for name, arglist in SWEEP_ARGS.items():
            for ai, args in enumerate(arglist):
                for interp in ((BILINEAR, BICUBIC) if name in GEOMETRIC else (BICUBIC,)):
                    yield f"{name}_{ai}_{interp}_in{ii}", name, args, interp, (kind, H, W)


def case_input(spec, seed=11) -> np.ndarray:
    kind, H, W = spec
    return make_input(kind, seed + 131 * H + W, H, W)


# ---- the recorded decision streams: RandAugment configurations and RandomErasing arguments, seeds 0 ... 63 -----------------------------------
# name -> (config string, hparams factory); four images in a row per seed (random.seed(s), numpy.random.seed(s))
RA_CONFIGS = {
    "timm224": ("rand-m9-mstd0.5-inc1", lambda: dict(translate_const=int(224 * 0.45), img_mean=(124, 116, 104), interpolation=BICUBIC)),
    "random_interp_w0": ("rand-m7-n3-mstd1-w0", lambda: dict(translate_const=100, img_mean=(128, 128, 128))),
    "plain": ("rand-n4", lambda: dict(translate_const=250, img_mean=(0, 0, 0))),
}
RA_IMAGES = 4
# max_area 1.6 makes boxes that do not fit, so the retries are part of the stream
RE_CONFIGS = {
    "image": dict(probability=0.6, min_area=0.1, max_area=1.6, min_count=1, max_count=3, mode="const", cube=False),
    "image_count1": dict(probability=0.25, mode="pixel", max_count=1, cube=False),
    "image_splits": dict(probability=0.9, min_count=2, max_count=2, mode="rand", num_splits=2, cube=False),
    "cube": dict(probability=0.7, min_area=0.1, max_area=1.6, min_count=1, max_count=2, mode="const", cube=True),
}
RE_SHAPE = (5, 3, 24, 31)
