"""RandAugment on the device: the counterpart of the reference's OCTCube/util/rand_augment.py (timm's auto_augment on Pillow), with its
names and its config grammar, for batches of uint8 images that are already on the GPU.

The reference applies ``num_layers`` randomly chosen Pillow operations to every image on a CPU worker.  Here the DECISIONS are drawn on
the host exactly as the reference draws them, and the PIXELS are computed by csrc/augment2d.hip, bit-equal to Pillow: with the same
seeds the result is the reference's.  Per image, in the reference's order and from the same sources (by default the global ``random``
and ``numpy.random``; instances may be given):

  1. ``numpy.random.choice`` of the ops of the image (with replacement; without when a weight set is configured)
  2. per chosen op  ``random.random() > prob`` (the op is skipped),
  3.                ``random.gauss(magnitude, magnitude_std)`` when a deviation is configured, clipped to [0, 10],
  4.                the level function, whose ``_randomly_negate`` draws ``random.random()``,
  5.                for a geometric op, ``random.choice`` of the interpolation when a tuple is configured.

No draw depends on a pixel, so the decisions of all images are drawn first, image by image, and the batch is then processed layer by
layer: one ops.image_stats launch when an op of the layer reads image statistics (AutoContrast, Equalize, Contrast), then one
ops.image_augment launch that applies every image's op of that layer.  ``last_params`` holds the drawn lists.

Not here: AutoAugment policies and AugMix (the reference's file does not carry them either); images are 3-channel uint8.
"""
from __future__ import annotations

import math
import random as _random
import re
from typing import List, Optional, Sequence, Tuple

import numpy as np

_FILL = (128, 128, 128)
_MAX_LEVEL = 10.0
_HPARAMS_DEFAULT = {"translate_const": 250, "img_mean": _FILL}
BILINEAR, BICUBIC = 2, 3                        # Pillow's Image.BILINEAR / Image.BICUBIC
_RANDOM_INTERPOLATION = (BILINEAR, BICUBIC)

_RAND_TRANSFORMS = ["AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast",
                    "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel"]
_RAND_INCREASING_TRANSFORMS = ["AutoContrast", "Equalize", "Invert", "Rotate", "PosterizeIncreasing", "SolarizeIncreasing", "SolarizeAdd",
                               "ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing", "ShearX", "ShearY",
                               "TranslateXRel", "TranslateYRel"]
_RAND_CHOICE_WEIGHTS_0 = {"Rotate": 0.3, "ShearX": 0.2, "ShearY": 0.2, "TranslateXRel": 0.1, "TranslateYRel": 0.1, "Color": 0.025,
                          "Sharpness": 0.025, "AutoContrast": 0.025, "Solarize": 0.005, "SolarizeAdd": 0.005, "Contrast": 0.005,
                          "Brightness": 0.005, "Equalize": 0.005, "Posterize": 0, "Invert": 0}
GEOMETRIC = ("Rotate", "ShearX", "ShearY", "TranslateX", "TranslateY", "TranslateXRel", "TranslateYRel")


# ---- level -> argument; rnd is the stream ``_randomly_negate`` draws from --------------------------------------------------------------
def _randomly_negate(v, rnd):
    return -v if rnd.random() > 0.5 else v


def _scaled_negated(full):                       # Rotate +-30, Shear +-0.3
    return lambda level, hp, rnd: (_randomly_negate((level / _MAX_LEVEL) * full, rnd),)


def _enhance(level, hp, rnd):                    # 0.1 ... 1.9
    return ((level / _MAX_LEVEL) * 1.8 + 0.1,)


def _enhance_increasing(level, hp, rnd):         # 1.0 -+ 0.9: away from "no change" with the level
    return (1.0 + _randomly_negate((level / _MAX_LEVEL) * 0.9, rnd),)


def _translate_abs(level, hp, rnd):
    return (_randomly_negate((level / _MAX_LEVEL) * float(hp["translate_const"]), rnd),)


def _translate_rel(level, hp, rnd):
    return (_randomly_negate((level / _MAX_LEVEL) * hp.get("translate_pct", 0.45), rnd),)


def _posterize(level, hp, rnd):                  # keep 0 ... 4 bits
    return (int((level / _MAX_LEVEL) * 4),)


def _solarize(level, hp, rnd):                   # 0 ... 256
    return (int((level / _MAX_LEVEL) * 256),)


LEVEL_TO_ARG = {
    "AutoContrast": None, "Equalize": None, "Invert": None,
    "Rotate": _scaled_negated(30.0),
    "Posterize": _posterize,
    "PosterizeIncreasing": lambda level, hp, rnd: (4 - _posterize(level, hp, rnd)[0],),
    "PosterizeOriginal": lambda level, hp, rnd: (int((level / _MAX_LEVEL) * 4) + 4,),
    "Solarize": _solarize,
    "SolarizeIncreasing": lambda level, hp, rnd: (256 - _solarize(level, hp, rnd)[0],),
    "SolarizeAdd": lambda level, hp, rnd: (int((level / _MAX_LEVEL) * 110),),
    "Color": _enhance, "ColorIncreasing": _enhance_increasing,
    "Contrast": _enhance, "ContrastIncreasing": _enhance_increasing,
    "Brightness": _enhance, "BrightnessIncreasing": _enhance_increasing,
    "Sharpness": _enhance, "SharpnessIncreasing": _enhance_increasing,
    "ShearX": _scaled_negated(0.3), "ShearY": _scaled_negated(0.3),
    "TranslateX": _translate_abs, "TranslateY": _translate_abs,
    "TranslateXRel": _translate_rel, "TranslateYRel": _translate_rel,
}


# ---- one drawn op -> the kernel's descriptor ----------------------------------------------------------------------------------------------
def rotate_matrix(W: int, H: int, degrees: float):
    """The matrix of Pillow's ``Image.rotate(degrees)`` about the centre; None where it copies instead (0 modulo 360)."""
    angle = degrees % 360.0
    if angle == 0:
        return None
    if angle in (90, 180, 270):
        raise NotImplementedError("Image.rotate transposes at 90 / 180 / 270 degrees; RandAugment's range is +-30")
    cx, cy = W / 2, H / 2
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def describe_op(rec, op: Optional[Tuple], H: int, W: int, fill=_FILL) -> None:
    """Fill ``rec`` (one ops.AUG_DESC record) for the drawn op (name, args, interpolation) on H x W images; None = no op."""
    from . import ops
    rec["kind"], rec["mode"], rec["m"], rec["factor"], rec["iarg"] = ops.AUG_NONE, 0, 0.0, 1.0, 0
    rec["fill"] = tuple(int(v) for v in fill) + (0,)
    if op is None:
        return
    name, args, interp = op
    base = name[:-len("Increasing")] if name.endswith("Increasing") else name
    if name in GEOMETRIC:
        v = float(args[0])
        if name == "Rotate":
            m = rotate_matrix(W, H, v)
        elif name == "ShearX":
            m = (1, v, 0, 0, 1, 0)
        elif name == "ShearY":
            m = (1, 0, 0, v, 1, 0)
        elif name in ("TranslateX", "TranslateXRel"):
            m = (1, 0, v * W if name.endswith("Rel") else v, 0, 1, 0)
        else:
            m = (1, 0, 0, 0, 1, v * H if name.endswith("Rel") else v)
        if m is None:
            return
        if int(interp) not in (BILINEAR, BICUBIC):
            raise NotImplementedError(f"{name}: interpolation {interp!r} (the kernel has Pillow's bilinear and bicubic filters)")
        rec["kind"], rec["mode"], rec["m"] = ops.AUG_AFFINE, int(interp), m
        return
    table = {"Invert": ops.AUG_LUT_INVERT, "AutoContrast": ops.AUG_LUT_AUTOCONTRAST, "Equalize": ops.AUG_LUT_EQUALIZE,
             "Posterize": ops.AUG_LUT_POSTERIZE, "PosterizeOriginal": ops.AUG_LUT_POSTERIZE, "Solarize": ops.AUG_LUT_SOLARIZE,
             "SolarizeAdd": ops.AUG_LUT_SOLARIZE_ADD, "Brightness": ops.AUG_LUT_BRIGHTNESS, "Contrast": ops.AUG_LUT_CONTRAST}
    if base in table:
        rec["kind"], rec["mode"] = ops.AUG_TABLE, table[base]
        if base in ("Brightness", "Contrast"):
            rec["factor"] = args[0]
        elif args:
            rec["iarg"] = int(args[0])
    elif base in ("Color", "Sharpness"):
        rec["kind"], rec["factor"] = (ops.AUG_COLOR if base == "Color" else ops.AUG_SHARPNESS), args[0]
    else:
        raise KeyError(name)


def describe(decisions: Sequence, layer: int, H: int, W: int, fill=_FILL) -> np.ndarray:
    """The descriptors of one layer: image i's ``layer``-th drawn op, or none where its list is shorter."""
    from . import ops
    desc = np.zeros(len(decisions), dtype=ops.AUG_DESC)
    for i, ops_i in enumerate(decisions):
        describe_op(desc[i], ops_i[layer] if layer < len(ops_i) else None, H, W, fill)
    return desc


class AugmentOp:
    """One op of the set: ``draw`` makes the reference's draws for one image and returns (name, args, interpolation), or None where the
    op is skipped (probability ``prob``)."""

    def __init__(self, name, prob=0.5, magnitude=10, hparams=None):
        hparams = hparams or _HPARAMS_DEFAULT
        self.name = name
        self.level_fn = LEVEL_TO_ARG[name]
        self.prob = prob
        self.magnitude = magnitude
        self.hparams = hparams.copy()
        self.fill = tuple(hparams["img_mean"]) if "img_mean" in hparams else _FILL
        self.interpolation = hparams["interpolation"] if "interpolation" in hparams else _RANDOM_INTERPOLATION
        self.magnitude_std = self.hparams.get("magnitude_std", 0)

    def draw(self, rnd=_random):
        if self.prob < 1.0 and rnd.random() > self.prob:
            return None
        magnitude = self.magnitude
        if self.magnitude_std and self.magnitude_std > 0:
            magnitude = rnd.gauss(magnitude, self.magnitude_std)
        magnitude = min(_MAX_LEVEL, max(0, magnitude))
        args = self.level_fn(magnitude, self.hparams, rnd) if self.level_fn is not None else ()
        interp = None
        if self.name in GEOMETRIC:
            interp = rnd.choice(self.interpolation) if isinstance(self.interpolation, (list, tuple)) else self.interpolation
            interp = int(interp)
        return (self.name, tuple(args), interp)


def _select_rand_weights(weight_idx=0, transforms=None):
    transforms = transforms or _RAND_TRANSFORMS
    assert weight_idx == 0          # the reference has one set
    probs = np.array([_RAND_CHOICE_WEIGHTS_0[k] for k in transforms], dtype=np.float64)
    return probs / np.sum(probs)


def rand_augment_ops(magnitude=10, hparams=None, transforms=None):
    hparams = hparams or _HPARAMS_DEFAULT
    return [AugmentOp(name, prob=0.5, magnitude=magnitude, hparams=hparams) for name in (transforms or _RAND_TRANSFORMS)]


class RandAugment:
    """``num_layers`` ops per image.  ``random`` / ``np_random``: the streams the decisions come from (default: the global ``random``
    module and ``numpy.random``, as in the reference; a ``random.Random`` / ``numpy.random.RandomState`` may be given)."""

    def __init__(self, ops, num_layers=2, choice_weights=None, random=None, np_random=None):
        self.ops = ops
        self.num_layers = num_layers
        self.choice_weights = choice_weights
        self.random = random if random is not None else _random
        self.np_random = np_random if np_random is not None else np.random
        self.last_params = None

    @property
    def fill(self):
        return self.ops[0].fill if self.ops else _FILL

    def draw(self, n: int) -> List[list]:
        """The decisions of n images, image by image: per image the list of its applied ops (name, args, interpolation)."""
        out = []
        for _ in range(n):
            idx = self.np_random.choice(len(self.ops), self.num_layers, replace=self.choice_weights is None, p=self.choice_weights)
            drawn = [self.ops[int(i)].draw(self.random) for i in idx]
            out.append([d for d in drawn if d is not None])
        return out

    def apply(self, images, decisions, lut=None, out=None):
        """uint8 [n, H, W, 3] on the GPU -> the images with their drawn ops applied: uint8, or through ``lut`` (the ToTensor ->
        Normalize table) float32 [n, 3, H, W] written by the last launch.  ``images`` is never written."""
        import torch
        from . import ops
        n, H, W, _ = images.shape
        if len(decisions) != n:
            raise ValueError(f"{len(decisions)} decision lists for {n} images")
        layers = max((len(d) for d in decisions), default=0)
        if layers == 0:
            if lut is None:
                return images if out is None else out.copy_(images)
            layers = 1                                  # normalise only
        cur, spare = images, [None, None]
        for layer in range(layers):
            desc = describe(decisions, layer, H, W, self.fill)
            need = ops.aug_needs_stats(desc)
            hist = ops.image_stats(cur, needed=need) if bool(need.any()) else None
            if layer == layers - 1:
                return ops.image_augment(cur, desc, hist=hist, lut=lut, out=out)
            k = layer & 1
            if spare[k] is None:
                spare[k] = torch.empty_like(images)
            cur = ops.image_augment(cur, desc, hist=hist, out=spare[k])

    def batch(self, images, lut=None, out=None):
        decisions = self.draw(int(images.shape[0]))
        res = self.apply(images, decisions, lut=lut, out=out)
        self.last_params = decisions
        return res

    def __call__(self, img):
        """One uint8 [H, W, 3] image on the GPU."""
        res = self.batch(img[None])[0]
        self.last_params = self.last_params[0]
        return res


def rand_augment_transform(config_str, hparams, random=None, np_random=None):
    """The reference's factory and grammar: sections separated by '-', the first 'rand', then in any order
        m<int> magnitude (default 10)   n<int> ops per image (default 2)   mstd<float> deviation of the magnitude
        w<int> weight set for the choice (only 0)   inc<int> the op list whose severity increases with the magnitude
    e.g. 'rand-m9-mstd0.5-inc1'.  As in the reference, ``inc`` is tested as a non-empty string: 'inc0' selects the increasing list too.
    ``hparams``: translate_const, img_mean (the fill colour), interpolation (a Pillow number, or a tuple to choose from per op)."""
    magnitude = _MAX_LEVEL
    num_layers = 2
    weight_idx = None
    transforms = _RAND_TRANSFORMS
    config = config_str.split("-")
    assert config[0] == "rand"
    for c in config[1:]:
        cs = re.split(r"(\d.*)", c)
        if len(cs) < 2:
            continue
        key, val = cs[:2]
        if key == "mstd":
            hparams.setdefault("magnitude_std", float(val))
        elif key == "inc":
            if bool(val):
                transforms = _RAND_INCREASING_TRANSFORMS
        elif key == "m":
            magnitude = int(val)
        elif key == "n":
            num_layers = int(val)
        elif key == "w":
            weight_idx = int(val)
    ra_ops = rand_augment_ops(magnitude=magnitude, hparams=hparams, transforms=transforms)
    choice_weights = None if weight_idx is None else _select_rand_weights(weight_idx)
    return RandAugment(ra_ops, num_layers, choice_weights=choice_weights, random=random, np_random=np_random)
