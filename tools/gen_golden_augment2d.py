"""Writes tests/golden/augment2d_small.npz WITH Pillow, through the reference's own two files (loaded by path, never copied):

    python tools/gen_golden_augment2d.py [--reference DIR] [--check]

DIR holds the reference's ``util/rand_augment.py`` and ``util/random_erasing.py`` (default: $OCTCUBE_REFERENCE, else
../reference/OCTCube beside this repository).  The file holds
  full_<case>, crcin_<case>   Pillow's output of NAME_TO_OP[op] for one case per op and interpolation (tests/augment2d_ref.py:
                              FULL_CASES), and the CRC-32 of the seeded input it was computed from
  blend_crc                   CRC-32 of Image.blend over all 256 x 256 byte pairs, per factor of BLEND_FACTORS
  sweep_keys, sweep_crc       CRC-32 of Pillow's output over the argument sweeps (sweep_cases: every boundary argument on ten inputs)
  decisions                   JSON: per configuration and seed 0...63, the ops the reference's RandAugment applied to four images in a
                              row -- [name, args, interpolation] -- recorded by wrapping its op functions
  boxes                       JSON: per configuration and seed 0...63, the boxes its RandomErasing erased, per image and cube path
  pillow_version
--check recomputes everything and compares instead of writing."""
import argparse
import importlib.util
import json
import os
import random
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import augment2d_ref as R      # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "augment2d_small.npz")
SEEDS = range(64)

RA_CONFIGS, RE_CONFIGS, RE_SHAPE = R.RA_CONFIGS, R.RE_CONFIGS, R.RE_SHAPE


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def record_decisions(ra, cfg, hparams, images=4):
    """Run the reference's RandAugment on ``images`` tiny images per seed; every op function is wrapped to note what it was called with
    (the interpolation as _interpolation resolved it)."""
    out = []
    names = ra._RAND_INCREASING_TRANSFORMS if "inc" in cfg else ra._RAND_TRANSFORMS
    log = []
    real_interp = ra._interpolation

    def interp(kwargs):
        v = real_interp(kwargs)
        log[-1][2] = int(v)
        return v
    ra._interpolation = interp
    try:
        for seed in SEEDS:
            random.seed(seed)
            np.random.seed(seed)
            t = ra.rand_augment_transform(cfg, hparams())
            for op, name in zip(t.ops, names):
                def wrapped(img, *args, _fn=op.aug_fn, _name=name, **kw):
                    log.append([_name, [a for a in args], None])
                    return _fn(img, *args, **kw)
                op.aug_fn = wrapped
            per_seed = []
            for _ in range(images):
                del log[:]
                t(Image.new("RGB", (9, 7), (10, 20, 30)))
                per_seed.append([[n, a, i if n in R.GEOMETRIC else None] for n, a, i in log])
            out.append(per_seed)
    finally:
        ra._interpolation = real_interp
    return out


def record_boxes(re_mod, kw):
    import torch

    events = []

    class Stream:           # the module's ``random``: random() opens an image, randint results are noted
        def random(self):
            events.append(("image",))
            return random.random()

        def randint(self, a, b):
            v = random.randint(a, b)
            events.append(("randint", v))
            return v

        def uniform(self, a, b):
            return random.uniform(a, b)

    def pixels(per_pixel, rand_color, patch_size, dtype=None, device=None):
        events.append(("pixels", int(patch_size[1]), int(patch_size[2])))
        return torch.ones((patch_size[0], 1, 1))
    real_random, real_pixels = re_mod.random, re_mod._get_pixels
    re_mod.random, re_mod._get_pixels = Stream(), pixels
    out = []
    try:
        for seed in SEEDS:
            random.seed(seed)
            del events[:]
            eraser = re_mod.RandomErasing(device="cpu", **kw)
            x = eraser(torch.zeros(RE_SHAPE))
            start = RE_SHAPE[0] // kw["num_splits"] if kw.get("num_splits", 0) > 1 else 0
            boxes, img, mask = [], start - 1, torch.zeros(RE_SHAPE)
            for k, e in enumerate(events):
                if e[0] == "image":
                    img += 1
                elif e[0] == "pixels":
                    if events[k - 1][0] == "randint":       # a new box: top and left were drawn just before its first fill
                        top_left, i = (events[k - 2][1], events[k - 1][1]), (start if kw["cube"] else img)
                    else:                                   # the cube path fills the same box in the next image
                        i += 1
                    box = (*top_left, e[1], e[2])
                    boxes.append([i, *box])
                    mask[i, :, box[0]:box[0] + box[2], box[1]:box[1] + box[3]] = 1
            assert torch.equal(mask, x), (seed, boxes)           # the recorded boxes are what the reference erased
            out.append(boxes)
    finally:
        re_mod.random, re_mod._get_pixels = real_random, real_pixels
    return out


def build(ref_dir):
    ra = _load(os.path.join(ref_dir, "util", "rand_augment.py"), "_ref_rand_augment")
    re_mod = _load(os.path.join(ref_dir, "util", "random_erasing.py"), "_ref_random_erasing")
    d = {"pillow_version": np.array(PIL.__version__)}

    def pillow(x, name, args, interp):
        return np.asarray(ra.NAME_TO_OP[name](Image.fromarray(x), *args, resample=interp, fillcolor=R.FILL))
    for case, (name, args, interp, spec) in R.FULL_CASES.items():
        x = R.case_input(spec)
        d["full_" + case] = pillow(x, name, args, interp)
        d["crcin_" + case] = np.array(R.crc(x), dtype=np.int64)
    keys, crcs = [], []
    for key, name, args, interp, spec in R.sweep_cases():
        keys.append(key)
        crcs.append(R.crc(pillow(R.case_input(spec), name, args, interp)))
    d["sweep_keys"] = np.array(keys)
    d["sweep_crc"] = np.array(crcs, dtype=np.int64)
    d["sweep_in_crc"] = np.array([R.crc(R.case_input(s)) for s in R.SWEEP_INPUTS], dtype=np.int64)
    a, b = R.blend_pairs()
    d["blend_crc"] = np.array([R.crc(np.asarray(Image.blend(Image.fromarray(a), Image.fromarray(b), f))) for f in R.BLEND_FACTORS],
                              dtype=np.int64)
    d["decisions"] = np.array(json.dumps({k: record_decisions(ra, cfg, hp) for k, (cfg, hp) in RA_CONFIGS.items()}))
    d["boxes"] = np.array(json.dumps({k: record_boxes(re_mod, kw) for k, kw in RE_CONFIGS.items()}))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--reference", default=os.environ.get("OCTCUBE_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference", "OCTCube")))
    a = ap.parse_args()
    d = build(a.reference)
    if a.check:
        g = np.load(PATH)
        bad = [k for k in d if k != "pillow_version" and not np.array_equal(g[k], d[k])]
        if str(g["pillow_version"]) != str(d["pillow_version"]):
            print(f"note: the file was written with Pillow {g['pillow_version']}, this is {d['pillow_version']}")
        print("differs: " + ", ".join(bad) if bad else
              f"{PATH}: {len(R.FULL_CASES)} full cases, {len(d['sweep_keys'])} swept, decisions and boxes equal Pillow {d['pillow_version']}")
        sys.exit(1 if bad else 0)
    np.savez_compressed(PATH, **d)
    print(f"{PATH}: {len(R.FULL_CASES)} full cases, {len(d['sweep_keys'])} swept, {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
