"""CPU side of the 2-D image transforms: the numpy restatement of Pillow's 8-bit bicubic resize (tests/transform2d_ref.py) against the
golden vectors written with Pillow (tests/golden/image2d_small.npz, tools/gen_golden_image2d.py) and, where Pillow imports, against
live Pillow calls; the host-side tile planner of csrc/image2d_plan.hpp through octmae_image_resample_plan; the argument errors of the
two C-ABI entry points (reported before any launch); the crop draw and the ToTensor -> Normalize table of octcubem_amd.transforms."""
import ctypes
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import transform2d_ref as R
from tests.conftest import GOLDEN

LDS_BUDGET = 64 * 1024          # csrc/image2d_plan.hpp: IMG_LDS_BUDGET, two workgroups per 160 KiB CU
LUT_BYTES = 3 * 256 * 4
TILE_W = 64


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "image2d_small.npz"))


def test_restatement_equals_the_golden_vectors_bit_for_bit(golden):
    assert {k[4:] for k in golden.files if k.startswith("out_")} == set(R.CASES)
    for name, (_, _, _, crop, size) in R.CASES.items():
        x = R.case_input(name)
        assert R.crc(x) == int(golden["crc_" + name]), f"{name}: the seeded input is not the one the golden output was computed from"
        y = R.resize(x, size, crop)
        assert y.dtype == np.uint8 and np.array_equal(y, golden["out_" + name]), name


def test_the_binary_cases_clamp_in_both_passes_on_both_sides():
    """The restatement itself sees sums below 0 and above 255 in the horizontal and in the vertical pass of the two binary cases: a
    test on them cannot pass with a resize that rounds and clamps once at the end."""
    for name in ("binary_37x53_to_64x32", "binary_61x100_to_50x70"):
        stats = {}
        R.resize(R.case_input(name), R.CASES[name][4], stats=stats)
        assert min(stats[k] for k in ("h_below", "h_above", "v_below", "v_above")) >= 1, (name, stats)


def test_restatement_equals_live_pillow_on_random_shapes():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.Generator(np.random.PCG64(2024))
    for i in range(20):
        H, W, OH, OW = (int(v) for v in rng.integers(1, 97, 4))
        x = rng.integers(0, 256, (H, W) if i % 5 else (H, W, 3), dtype=np.uint8)
        crop = None
        if i % 2:
            h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
            crop = (int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w)
        im = Image.fromarray(x)
        if crop is not None:
            im = im.crop((crop[1], crop[0], crop[1] + crop[3], crop[0] + crop[2]))
        want = np.asarray(im.resize((OW, OH), Image.BICUBIC))
        assert np.array_equal(R.resize(x, (OH, OW), crop), want), (H, W, OH, OW, crop)


def _plan(lib, H, W, C, ch, cw, OH, OW):
    th, lds = ctypes.c_int(-7), ctypes.c_int(-7)
    rc = lib.octmae_image_resample_plan(H, W, C, ch, cw, OH, OW, ctypes.addressof(th), ctypes.addressof(lds))
    return rc, th.value, lds.value


@lru_cache(maxsize=None)
def _ksize(n_in, n_out):
    return R.axis_coeffs(n_in, n_out)[1].shape[1]


@lru_cache(maxsize=None)
def _row_span(n_in, n_out, th):
    return R.row_span(n_in, n_out, th)


def _lds_bytes(in_h, in_w, C, OH, OW, th, tw):
    """The layout of csrc/image2d_plan.hpp from the restatement's windows: the table, [ksize_x + 2][tw] and [ksize_y + 2][th] int32,
    and the horizontal pass of the longest row span of a tile, uint8 [rows][tw * C] rounded up to dwords."""
    ksx, ksy = _ksize(in_w, OW), _ksize(in_h, OH)
    tmp = (_row_span(in_h, OH, th) * tw * C + 3) // 4 * 4
    return LUT_BYTES + 4 * tw * (ksx + 2) + 4 * th * (ksy + 2) + tmp


def _expected_plan(in_h, in_w, C, OH, OW):
    """The planner's rule restated: the widest tile of {64, 32, ... 1} columns (capped by OW) for which some tile height fits the
    budget, and for it the largest height of {32, 16, ... 1}.  None: nothing fits."""
    for tw in sorted({min(t, OW) for t in (64, 32, 16, 8, 4, 2, 1)}, reverse=True):
        for th in (32, 16, 8, 4, 2, 1):
            b = _lds_bytes(in_h, in_w, C, OH, OW, th, tw)
            if b <= LDS_BUDGET:
                return th, tw, b
    return None


def test_planner_fits_the_budget_and_matches_the_restatements_row_span():
    from octcubem_amd import _lib
    lib = _lib.load()
    geoms = set()
    for name, (_, _, shape, crop, size) in R.CASES.items():
        ih, iw = (crop[2], crop[3]) if crop else shape[:2]
        geoms.add((shape[0], shape[1], 3 if len(shape) == 3 else 1, 0 if crop is None else ih, 0 if crop is None else iw, *size))
    for H in (1, 7, 64, 496, 1024):
        for W in (1, 7, 64, 496, 1024):
            for OH in (1, 8, 224, 512):
                for OW in (1, 8, 224, 512):
                    geoms.update({(H, W, 1, 0, 0, OH, OW), (H, W, 3, 0, 0, OH, OW)})
    narrowed = 0
    for H, W, C, ch, cw, OH, OW in sorted(geoms):
        rc, th, lds = _plan(lib, H, W, C, ch, cw, OH, OW)
        assert rc == 0 and th in (32, 16, 8, 4, 2, 1) and 0 < lds <= LDS_BUDGET, (H, W, C, ch, cw, OH, OW, rc, th, lds)
        ih, iw = (ch, cw) if ch else (H, W)
        want = _expected_plan(ih, iw, C, OH, OW)
        # tile_h x the restatement's row span of that tile height gives lds_bytes, and no larger tile fits
        assert want is not None and (th, lds) == (want[0], want[2]), (H, W, C, ch, cw, OH, OW, th, lds, want)
        narrowed += want[1] < min(TILE_W, OW)
    assert narrowed >= 1                     # the sweep reaches the narrowed tiles (1024 rows -> 1 under 512 RGB columns)
    # the B-scan geometries take the full tile in a few KiB
    for W in (512, 1024):
        rc, th, lds = _plan(lib, 496, W, 1, 0, 0, 512, 512)
        assert rc == 0 and th == 32 and lds <= 16 * 1024
    # a reduction by a factor in the thousands has no plan: one output's window does not fit
    assert _plan(lib, 4096, 4096, 1, 0, 0, 1, 1)[0] == -1
    assert _plan(lib, 8, 4096, 1, 0, 0, 8, 1)[0] == -1 and _plan(lib, 4096, 8, 3, 0, 0, 1, 8)[0] == -1


def test_image_entry_points_report_argument_errors_without_a_gpu():
    from octcubem_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)                 # never dereferenced: every call below is refused before a launch

    def run(src=p, n=1, H=8, W=8, C=1, top=0, left=0, ch=0, cw=0, OH=4, OW=4, flip=0, lut=None, dst=p):
        return lib.octmae_image_resample(src, n, H, W, C, top, left, ch, cw, OH, OW, flip, lut, dst, None)

    assert run(src=None) == -1 and run(dst=None) == -1
    for kw in ({"n": 0}, {"n": -1}, {"H": 0}, {"W": 0}, {"H": -3}, {"OH": 0}, {"OW": 0}, {"OW": -1}):
        assert run(**kw) == -1, kw
    for C in (0, 2, 4, -1):
        assert run(C=C) == -1, C
    # a crop outside the image, a negative one, or one with exactly one of ch, cw zero
    for kw in ({"top": 5, "ch": 4, "cw": 4}, {"left": 5, "ch": 4, "cw": 4}, {"ch": 9, "cw": 1}, {"ch": 1, "cw": 9}, {"top": -1, "ch": 2, "cw": 2},
               {"left": -1, "ch": 2, "cw": 2}, {"ch": 4, "cw": 0}, {"ch": 0, "cw": 4}, {"ch": -2, "cw": -2}, {"top": 1}, {"left": 1}):
        assert run(**kw) == -1, kw
    assert run(H=4096, W=4096, OH=1, OW=1) == -1                 # no plan fits
    th, lds = ctypes.c_int(), ctypes.c_int()
    a, b = ctypes.addressof(th), ctypes.addressof(lds)
    assert lib.octmae_image_resample_plan(8, 8, 1, 0, 0, 4, 4, None, b) == -1
    assert lib.octmae_image_resample_plan(8, 8, 1, 0, 0, 4, 4, a, None) == -1
    for H, W, C, ch, cw, OH, OW in ((0, 8, 1, 0, 0, 4, 4), (8, 0, 1, 0, 0, 4, 4), (8, 8, 2, 0, 0, 4, 4), (8, 8, 1, 9, 1, 4, 4), (8, 8, 1, 0, 3, 4, 4),
                                    (8, 8, 1, 0, 0, 0, 4), (8, 8, 1, 0, 0, 4, -1)):
        assert lib.octmae_image_resample_plan(H, W, C, ch, cw, OH, OW, a, b) == -1
    with pytest.raises(_lib.OctmaeError, match="bad argument"):
        _lib.call("octmae_image_resample", None, 1, 8, 8, 1, 0, 0, 0, 0, 4, 4, 0, None, None, None)
    # the kernel has no CPU form: a CPU tensor handed to the raw op is an error, not a fall-back; so is another dtype or shape
    from octcubem_amd import ops
    with pytest.raises(RuntimeError):
        ops.image_resample(torch.zeros(8, 8, dtype=torch.uint8), (4, 4))
    with pytest.raises(RuntimeError):
        ops.image_resample(torch.zeros(8, 8), (4, 4))
    with pytest.raises(RuntimeError):
        ops.image_resample(torch.zeros(2, 8, 8, 4, dtype=torch.uint8), (4, 4))


@pytest.mark.parametrize("H,W", [(496, 512), (8, 300), (1, 1)])
def test_crop_draw_follows_the_published_rule(H, W):
    from octcubem_amd.transforms import random_resized_crop_params as draw
    scale, ratio = (0.2, 1.0), (3 / 4, 4 / 3)
    g, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    # the centred fallback: the aspect ratio clamped into `ratio`
    if W / H > ratio[1]:
        fh, fw = H, int(round(H * ratio[1]))
    elif W / H < ratio[0]:
        fw, fh = W, int(round(W / ratio[0]))
    else:
        fh, fw = H, W
    fallback = ((H - fh) // 2, (W - fw) // 2, fh, fw)
    n_fallback = 0
    for _ in range(2000):
        top, left, h, w = draw(H, W, scale, ratio, g)
        assert (top, left, h, w) == draw(H, W, scale, ratio, g2)          # one seed, one sequence
        assert 0 <= top and 0 <= left and 1 <= h and 1 <= w and top + h <= H and left + w <= W
        # An accepted try has w = round(sqrt(A r)), h = round(sqrt(A / r)) with A / (H W) in `scale`, r in `ratio`: each side is within 0.5 of
        # its unrounded value, so (w -+ 0.5)(h -+ 0.5) brackets A.  Anything else can only be the fallback.
        lo, hi = max(w - 0.5, 0) * max(h - 0.5, 0), (w + 0.5) * (h + 0.5)
        if not (lo <= scale[1] * H * W and hi >= scale[0] * H * W):
            assert (top, left, h, w) == fallback
        if (top, left, h, w) == fallback:
            n_fallback += 1
    if (H, W) == (8, 300):
        # 300 / 8 is far outside the ratio range: a try fits only when h = round(sqrt(A / r)) <= 8, and many draws find none in ten
        assert fallback == (0, 144, 8, 11) and n_fallback >= 1
        assert abs(fallback[3] / fallback[2] - ratio[1]) <= 0.5 / fallback[2]
    if (H, W) == (1, 1):
        assert fallback == (0, 0, 1, 1)


def test_table_equals_totensor_normalize_on_all_levels():
    from octcubem_amd.transforms import IMAGENET_MEAN, IMAGENET_STD, create_2d_transforms, normalize_lut
    levels = np.arange(256, dtype=np.uint8).reshape(16, 16)
    for mean, std in ((IMAGENET_MEAN, IMAGENET_STD), (0.5, 0.25)):
        t = normalize_lut(mean, std)
        assert t.shape == (3, 256) and t.dtype == torch.float32
        want = R.to_tensor_normalize(levels, mean, std).reshape(3, 256)      # the chain on a grey image holding every level once
        assert torch.equal(t, want) and torch.equal(t, R.lut(mean, std))
        rgb = np.stack([levels, levels[::-1], levels.T], axis=2)                # and on an RGB one, channel by channel
        got = torch.stack([t[c][torch.from_numpy(np.ascontiguousarray(rgb[:, :, c])).long()] for c in range(3)])
        assert torch.equal(got, R.to_tensor_normalize(rgb, mean, std))
    assert IMAGENET_MEAN == R.IMAGENET_MEAN and IMAGENET_STD == R.IMAGENET_STD
    # the choice of arithmetic matters: the same chain in double, rounded once, is another table
    d = ((torch.arange(256, dtype=torch.float64) / 255 - IMAGENET_MEAN[0]) / IMAGENET_STD[0]).float()
    assert int((d != normalize_lut()[0]).sum()) > 0
    tr = create_2d_transforms(512)
    assert tr.size == (512, 512) and not tr.random_resized_crop and tr.hflip_prob == 0.0 and torch.equal(tr.lut, normalize_lut())
    tr = create_2d_transforms((224, 192), mean=0.5, std=0.25, random_resized_crop=True, hflip_prob=0.5)
    assert tr.size == (224, 192) and tr.random_resized_crop and torch.equal(tr.lut, normalize_lut(0.5, 0.25))
    # shape and dtype errors are raised before anything is moved to a GPU
    for bad in (torch.zeros(4, 4), torch.zeros(4, 4, 2, dtype=torch.uint8), np.zeros((2, 3, 4, 4), np.uint8), "x"):
        with pytest.raises(ValueError):
            tr(bad)
