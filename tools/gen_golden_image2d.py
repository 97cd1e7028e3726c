"""Writes tests/golden/image2d_small.npz WITH Pillow -- the library torchvision's Resize / resized_crop call for a PIL image:

    python tools/gen_golden_image2d.py [--check]

Every case of tests/transform2d_ref.py: CASES runs through ``Image.fromarray(a)[.crop(box)].resize((OW, OH), Image.BICUBIC)``.  The
inputs come from seeded numpy generators, so the file holds, per case, Pillow's output (``out_<case>``) and the CRC-32 of the input it
was computed from (``crc_<case>``), not the input.  --check recomputes and compares instead of writing (needs Pillow as well)."""
import argparse
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import transform2d_ref as R      # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "image2d_small.npz")


def pillow_resize(a: np.ndarray, size, crop=None) -> np.ndarray:
    im = Image.fromarray(a)
    if crop is not None:
        t, l, h, w = crop
        im = im.crop((l, t, l + w, t + h))
    return np.asarray(im.resize((size[1], size[0]), Image.BICUBIC))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    d = {"pillow_version": np.array(Image.__version__ if hasattr(Image, "__version__") else "?")}
    for name, (_, _, _, crop, size) in R.CASES.items():
        x = R.case_input(name)
        d["out_" + name] = pillow_resize(x, size, crop)
        d["crc_" + name] = np.array(R.crc(x), dtype=np.int64)
    if a.check:
        g = np.load(PATH)
        bad = [k for k in d if k != "pillow_version" and not np.array_equal(g[k], d[k])]
        print("differs: " + ", ".join(bad) if bad else f"{PATH}: {len(R.CASES)} cases equal Pillow {d['pillow_version']}")
        sys.exit(1 if bad else 0)
    np.savez_compressed(PATH, **d)
    print(f"{PATH}: {len(R.CASES)} cases, {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
