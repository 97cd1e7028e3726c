"""CPU: the numpy restatement of RandAugment's Pillow operations (tests/augment2d_ref.py) against the golden vectors Pillow wrote through
the reference's own file (tests/golden/augment2d_small.npz, tools/gen_golden_augment2d.py) and, where Pillow is installed, against Pillow
itself; the decision streams of octcubem_amd.rand_augment / random_erasing against the reference's recorded ones; the argument rules of
the two entry points; build_transform's chains.  Every comparison is exact."""
import ctypes
import json
import os
import random
import types

import numpy as np
import pytest
import torch

from tests import augment2d_ref as R


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "augment2d_small.npz"))


def test_restatement_equals_the_golden_vectors_bit_for_bit(golden):
    assert {k[5:] for k in golden.files if k.startswith("full_")} == set(R.FULL_CASES)
    for case, (name, args, interp, spec) in R.FULL_CASES.items():
        x = R.case_input(spec)
        assert R.crc(x) == int(golden["crcin_" + case]), f"{case}: the seeded input is not the one the golden output was computed from"
        y = R.apply(x, name, args, interp)
        assert y.dtype == np.uint8 and np.array_equal(y, golden["full_" + case]), case
    assert [R.crc(R.case_input(s)) for s in R.SWEEP_INPUTS] == [int(v) for v in golden["sweep_in_crc"]]
    want = dict(zip((str(k) for k in golden["sweep_keys"]), (int(v) for v in golden["sweep_crc"])))
    inputs = {}
    n = 0
    for key, name, args, interp, spec in R.sweep_cases():
        x = inputs.setdefault(spec, R.case_input(spec))
        assert R.crc(R.apply(x, name, args, interp)) == want[key], key
        n += 1
    assert n == len(want)


def test_the_inputs_make_the_rules_bite():
    """Uniform noise leaves AutoContrast an identity; the low-contrast input does not.  Equalize: identity on a constant image (one
    bin) and on 8 x 8 (step == 0), not on the larger inputs.  The binary input drives the bicubic filter into both clips; the blend's
    clipping branch clips on both sides."""
    noise, low = R.make_input("noise", 1, 37, 53), R.make_input("lowcontrast", 1, 37, 53)
    assert np.array_equal(R.apply(noise, "AutoContrast"), noise) and not np.array_equal(R.apply(low, "AutoContrast"), low)
    assert low.min() >= 40 and low.max() <= 200
    const, small = R.make_input("constant", 2, 5, 9), R.make_input("noise", 3, 8, 8)
    for x in (const, small):
        assert np.array_equal(R.apply(x, "Equalize"), x) and np.array_equal(R.lut_equalize(R.stats(x)), np.stack([np.arange(256)] * 3))
    assert np.array_equal(R.apply(const, "AutoContrast"), const)
    assert not np.array_equal(R.apply(low, "Equalize"), low)
    binary = R.make_input("binary", 4, 37, 53)
    m = R.rotate_matrix(53, 37, 30.0)
    lin, cub = R.affine(binary, m, R.BILINEAR), R.affine(binary, m, R.BICUBIC)
    inner = (slice(12, 25), slice(20, 33))          # inside the rotated image: no fill
    assert set(np.unique(cub[inner])) >= {0, 255} and not np.array_equal(lin, cub)
    a, b = R.blend_pairs()
    hi = R.blend(a, b, 1.9)
    assert (hi == 0).sum() > 256 and (hi == 255).sum() > 256
    assert R.lut_solarize(256)[0].tolist() == list(range(256)) and R.lut_posterize(0).max() == 0


def test_blend_on_every_pair_of_bytes(golden):
    a, b = R.blend_pairs()
    for f, want in zip(R.BLEND_FACTORS, golden["blend_crc"]):
        assert R.crc(R.blend(a, b, f)) == int(want), f
    Image = pytest.importorskip("PIL.Image")
    for f in R.BLEND_FACTORS + (0.25, 0.75, 1.3, 1.7):
        want = np.asarray(Image.blend(Image.fromarray(a), Image.fromarray(b), f))
        assert np.array_equal(R.blend(a, b, f), want), f


def _pillow_op(Image, x, name, args, interp, fill):
    from PIL import ImageEnhance, ImageOps
    im = Image.fromarray(x)
    kw = dict(resample=interp, fillcolor=fill)
    if name == "Rotate":
        return im.rotate(args[0], **kw)
    if name in R.GEOMETRIC:
        return im.transform(im.size, Image.AFFINE, R.op_matrix(name, args[0], *im.size), **kw)
    if name == "AutoContrast":
        return ImageOps.autocontrast(im)
    if name == "Equalize":
        return ImageOps.equalize(im)
    if name == "Invert":
        return ImageOps.invert(im)
    if name == "Posterize":
        return im if args[0] >= 8 else ImageOps.posterize(im, args[0])
    if name == "Solarize":
        return ImageOps.solarize(im, args[0])
    if name == "SolarizeAdd":
        return im.point([min(255, i + args[0]) if i < 128 else i for i in range(256)] * 3)
    return getattr(ImageEnhance, name)(im).enhance(args[0])


def test_restatement_equals_live_pillow_on_random_shapes():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.Generator(np.random.PCG64(2025))
    ranges = {"Rotate": 30.0, "ShearX": 0.3, "ShearY": 0.3, "TranslateXRel": 0.45, "TranslateYRel": 0.45, "TranslateX": 100.0,
              "TranslateY": 100.0}
    for it in range(40):
        H, W = (int(v) for v in rng.integers(1, 97, 2))
        x = R.make_input(R.INPUT_KINDS[it % len(R.INPUT_KINDS)], 1000 + it, H, W)
        for name in R.SWEEP_ARGS:
            if name in ranges:
                args = (float(rng.uniform(-ranges[name], ranges[name])),)
            elif name in ("Color", "Contrast", "Brightness", "Sharpness"):
                args = (float(rng.uniform(0.1, 1.9)),)
            elif name in ("Posterize", "Solarize", "SolarizeAdd"):
                args = (int(rng.integers(0, {"Posterize": 9, "Solarize": 257, "SolarizeAdd": 111}[name])),)
            else:
                args = ()
            interp = int(rng.integers(2, 4))
            fill = tuple(int(v) for v in rng.integers(0, 256, 3))
            want = np.asarray(_pillow_op(Image, x, name, args, interp, fill))
            assert np.array_equal(R.apply(x, name, args, interp, fill), want), (name, args, interp, H, W)


def test_contrast_mean_and_stats():
    x = R.make_input("lowcontrast", 9, 33, 47)
    h = R.stats(x)
    assert h.shape == (4, 256) and h.dtype == np.uint32 and (h.sum(axis=1) == 33 * 47).all()
    l = R.to_l(x).astype(np.float64)
    assert R.contrast_mean(h[3]) == int(l.mean() + 0.5)


# ---- the decision streams ------------------------------------------------------------------------------------------------------------------
def _norm(decisions):
    return [[[n, list(a), i] for n, a, i in img] for img in decisions]


@pytest.mark.parametrize("cfg", list(R.RA_CONFIGS))
def test_rand_augment_draws_the_references_decisions(golden, cfg):
    from octcubem_amd.rand_augment import rand_augment_transform
    want = json.loads(str(golden["decisions"]))[cfg]
    config, hparams = R.RA_CONFIGS[cfg]
    assert len(want) == 64
    for seed in range(64):
        # the global streams, as the reference uses them ...
        random.seed(seed)
        np.random.seed(seed)
        t = rand_augment_transform(config, hparams())
        got = t.draw(R.RA_IMAGES)
        assert _norm(got) == want[seed], (cfg, seed)
        # ... and private instances
        t = rand_augment_transform(config, hparams(), random=random.Random(seed), np_random=np.random.RandomState(seed))
        assert _norm(t.draw(R.RA_IMAGES)) == want[seed], (cfg, seed)
    seen = {op[0] for s in want for img in s for op in img}
    if cfg == "timm224":
        from octcubem_amd.rand_augment import _RAND_INCREASING_TRANSFORMS
        assert seen == set(_RAND_INCREASING_TRANSFORMS)          # the 64 seeds reach every op of the set
        assert {op[2] for s in want for img in s for op in img} == {None, 3}
    if cfg == "random_interp_w0":
        assert {op[2] for s in want for img in s for op in img} == {None, 2, 3} and "Invert" not in seen and "Posterize" not in seen


@pytest.mark.parametrize("cfg", list(R.RE_CONFIGS))
def test_random_erasing_draws_the_references_boxes(golden, cfg):
    from octcubem_amd.random_erasing import RandomErasing
    want = json.loads(str(golden["boxes"]))[cfg]
    kw = R.RE_CONFIGS[cfg]
    total = 0
    for seed in range(64):
        random.seed(seed)
        eraser = RandomErasing(device="cpu", **kw)
        x = eraser(torch.ones(R.RE_SHAPE))
        assert [list(b) for b in eraser.last_boxes] == want[seed], (cfg, seed)
        eraser = RandomErasing(device="cpu", random=random.Random(seed), **kw)
        eraser(torch.ones(R.RE_SHAPE))
        assert [list(b) for b in eraser.last_boxes] == want[seed], (cfg, seed)
        inside = torch.zeros(R.RE_SHAPE, dtype=torch.bool)
        for i, top, left, h, w in want[seed]:
            inside[i, :, top:top + h, left:left + w] = True
        assert torch.equal(x[~inside], torch.ones(int((~inside).sum())))
        if kw["mode"] == "const":
            assert float(x[inside].abs().sum()) == 0.0
        total += len(want[seed])
    assert total > 0


def test_erasing_fill_modes_on_the_cpu():
    from octcubem_amd.random_erasing import RandomErasing
    for mode in ("rand", "pixel"):
        random.seed(3)
        torch.manual_seed(11)
        eraser = RandomErasing(probability=1.0, mode=mode, cube=False, device="cpu")
        x = eraser(torch.zeros(3, 3, 20, 20))
        torch.manual_seed(11)
        assert [b[0] for b in eraser.last_boxes] == [0, 1, 2]
        for i, top, left, h, w in eraser.last_boxes:        # one draw per box, in order
            shape = (3, h, w) if mode == "pixel" else (3, 1, 1)
            want = torch.empty(shape).normal_().expand(3, h, w)
            assert torch.equal(x[i, :, top:top + h, left:left + w], want)


# ---- descriptors and the entry points --------------------------------------------------------------------------------------------------------
def test_descriptor_layout_and_describe_op():
    from octcubem_amd import ops
    from octcubem_amd.rand_augment import describe
    assert ops.AUG_DESC.itemsize == 72 and ops.AUG_DESC.fields["m"][1] == 8 and ops.AUG_DESC.fields["factor"][1] == 56
    dec = [[("Rotate", (0.0,), 3)], [("Rotate", (-30.0,), 2), ("ContrastIncreasing", (1.9,), None)], [], [("PosterizeIncreasing", (2,), None)],
           [("TranslateXRel", (0.45,), 3)], [("SharpnessIncreasing", (0.1,), None)], [("Equalize", (), None)]]
    d0 = describe(dec, 0, 37, 53, fill=(1, 2, 3))
    assert d0["kind"].tolist() == [ops.AUG_NONE, ops.AUG_AFFINE, ops.AUG_NONE, ops.AUG_TABLE, ops.AUG_AFFINE, ops.AUG_SHARPNESS, ops.AUG_TABLE]
    assert d0["mode"][1] == 2 and tuple(d0["m"][1]) == R.rotate_matrix(53, 37, -30.0) and d0["fill"][1].tolist() == [1, 2, 3, 0]
    assert tuple(d0["m"][4]) == (1, 0, 0.45 * 53, 0, 1, 0) and d0["iarg"][3] == 2 and d0["factor"][5] == np.float32(0.1)
    assert ops.aug_needs_stats(d0).tolist() == [False] * 6 + [True]
    d1 = describe(dec, 1, 37, 53)
    assert d1["kind"].tolist() == [0, ops.AUG_TABLE, 0, 0, 0, 0, 0] and d1["mode"][1] == ops.AUG_LUT_CONTRAST
    assert ops.aug_needs_stats(d1).tolist() == [False, True] + [False] * 5


def test_augment_entry_points_report_argument_errors_without_a_gpu():
    from octcubem_amd import _lib, ops
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)                 # never dereferenced: every call below is refused before a launch
    q = p + 2048

    def stats(src=p, n=1, H=8, W=8, needed=None, hist=q):
        return lib.octmae_image_stats(src, n, H, W, needed, hist, None)

    assert stats(src=None) == -1 and stats(hist=None) == -1
    for kw in ({"n": 0}, {"n": -2}, {"H": 0}, {"W": -1}, {"H": 1 << 16, "W": 1 << 15}):
        assert stats(**kw) == -1, kw

    good = np.zeros(2, dtype=ops.AUG_DESC)

    def aug(src=p, n=2, H=8, W=8, desc=p, host=good, hist=None, lut=None, dst=q):
        return lib.octmae_image_augment(src, n, H, W, desc, None if host is None else host.ctypes.data, hist, lut, dst, None)

    assert aug(src=None) == -1 and aug(dst=None) == -1 and aug(desc=None) == -1 and aug(dst=p) == -1
    for kw in ({"n": 0}, {"H": 0}, {"W": 0}, {"H": -5}, {"H": 1 << 16, "W": 1 << 15}):
        assert aug(**kw) == -1, kw

    def bad(**fields):
        d = good.copy()
        d["m"][1] = (1, 0, 0, 0, 1, 0)
        for k, v in fields.items():
            d[k][1] = v
        return d

    cases = [bad(kind=5), bad(kind=-1), bad(kind=ops.AUG_TABLE, mode=8), bad(kind=ops.AUG_TABLE, mode=-1),
             bad(kind=ops.AUG_TABLE, mode=ops.AUG_LUT_POSTERIZE, iarg=-1), bad(kind=ops.AUG_TABLE, mode=ops.AUG_LUT_SOLARIZE_ADD, iarg=256),
             bad(kind=ops.AUG_TABLE, mode=ops.AUG_LUT_BRIGHTNESS, factor=np.nan), bad(kind=ops.AUG_COLOR, factor=np.nan),
             bad(kind=ops.AUG_SHARPNESS, factor=np.nan), bad(kind=ops.AUG_AFFINE, mode=0), bad(kind=ops.AUG_AFFINE, mode=4),
             bad(kind=ops.AUG_AFFINE, mode=3, m=(1, 0, np.inf, 0, 1, 0)), bad(kind=ops.AUG_AFFINE, mode=2, m=(np.nan, 0, 0, 0, 1, 0))]
    for d in cases:
        assert aug(host=d) == -1, d[1]
    # an op that reads the statistics, and no histograms
    for mode in (ops.AUG_LUT_CONTRAST, ops.AUG_LUT_AUTOCONTRAST, ops.AUG_LUT_EQUALIZE):
        assert aug(host=bad(kind=ops.AUG_TABLE, mode=mode)) == -1, mode
    with pytest.raises(_lib.OctmaeError):
        _lib.call("octmae_image_augment", None, 1, 8, 8, None, None, None, None, None, None)
    # the kernels have no CPU form: a CPU tensor handed to the raw ops is an error, not a fall-back; so is another dtype or shape
    with pytest.raises(RuntimeError):
        ops.image_stats(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        ops.image_augment(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), np.zeros(1, dtype=ops.AUG_DESC))
    with pytest.raises(RuntimeError):
        ops.image_augment(torch.zeros(1, 8, 8, dtype=torch.uint8), np.zeros(1, dtype=ops.AUG_DESC))


# ---- build_transform -------------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    base = dict(input_size=224, aa="rand-m9-mstd0.5-inc1", reprob=0.25, remode="pixel", recount=1, color_jitter=None)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_build_transform_chains_and_hparams():
    from octcubem_amd import rand_augment as RA
    from octcubem_amd.transforms import IMAGENET_MEAN, Image2DTransform, build_transform
    t = build_transform("train", _args())
    assert isinstance(t, Image2DTransform) and t.size == (224, 224) and t.random_resized_crop and t.scale == (0.08, 1.0)
    assert t.ratio == (3 / 4, 4 / 3) and t.hflip_prob == 0.5 and t.center_crop is None
    aug = t.auto_augment
    assert isinstance(aug, RA.RandAugment) and aug.num_layers == 2 and aug.choice_weights is None
    assert [op.name for op in aug.ops] == RA._RAND_INCREASING_TRANSFORMS
    for op in aug.ops:
        assert op.magnitude == 9 and op.magnitude_std == 0.5 and op.prob == 0.5 and op.interpolation == 3
        assert op.hparams["translate_const"] == 100 and op.fill == (124, 116, 104) == tuple(round(255 * m) for m in IMAGENET_MEAN)
    er = t.random_erasing
    assert er.probability == 0.25 and er.per_pixel and not er.rand_color and not er.cube and (er.min_count, er.max_count) == (1, 1)
    # color_jitter: ignored beside aa (timm), refused without
    assert build_transform("train", _args(color_jitter=0.4)).auto_augment is not None
    with pytest.raises(NotImplementedError):
        build_transform("train", _args(aa=None, color_jitter=0.4))
    plain = build_transform("train", _args(aa=None, reprob=0.0))
    assert plain.auto_augment is None and plain.random_erasing is None
    # the reference compares with the string 'train': anything else is the eval chain
    for size, full in ((224, 256), (128, 146), (512, 512), (225, 225)):
        e = build_transform("val", _args(input_size=size))
        assert e.size == (full, full) and e.center_crop == (size, size) and not e.random_resized_crop and e.hflip_prob == 0.0
        assert e.auto_augment is None and e.random_erasing is None
    assert build_transform(True, _args()).center_crop == (224, 224)


def test_image2d_transform_defaults_leave_the_new_stages_off():
    import inspect

    from octcubem_amd.transforms import Image2DTransform, create_2d_transforms
    sig = inspect.signature(Image2DTransform.__init__).parameters
    assert (sig["auto_augment"].default, sig["aa_hparams"].default, sig["re_prob"].default, sig["re_mode"].default,
            sig["re_count"].default) == (None, None, 0.0, "const", 1)
    assert list(inspect.signature(create_2d_transforms).parameters) == ["input_size", "mean", "std", "random_resized_crop", "scale", "ratio",
                                                                        "hflip_prob", "generator"]
    for t in (create_2d_transforms(512), create_2d_transforms(224, random_resized_crop=True, hflip_prob=0.5)):
        assert t.auto_augment is None and t.random_erasing is None and t.center_crop is None


def test_config_grammar():
    from octcubem_amd import rand_augment as RA
    hp = {}
    t = RA.rand_augment_transform("rand-m5-n3-mstd0.25-w0", hp)
    assert hp == {"magnitude_std": 0.25} and t.num_layers == 3 and [op.name for op in t.ops] == RA._RAND_TRANSFORMS
    assert t.ops[0].magnitude == 5 and abs(float(np.sum(t.choice_weights)) - 1.0) < 1e-12 and t.choice_weights[2] == 0.0
    assert t.ops[0].interpolation == (2, 3) and t.ops[0].fill == (128, 128, 128)
    t = RA.rand_augment_transform("rand", {"magnitude_std": 2.0})
    assert t.num_layers == 2 and t.ops[0].magnitude == 10.0 and t.ops[0].magnitude_std == 2.0 and t.choice_weights is None
    assert [op.name for op in RA.rand_augment_transform("rand-inc0", {}).ops] == RA._RAND_INCREASING_TRANSFORMS     # the reference's bool("0")
    with pytest.raises(AssertionError):
        RA.rand_augment_transform("augmix-m3", {})
    # the absolute translations are accepted as ops of a hand-made set
    op = RA.AugmentOp("TranslateX", prob=1.0, magnitude=10, hparams={"translate_const": 40, "interpolation": 2})
    assert op.draw(random.Random(0))[0] == "TranslateX" and abs(op.draw(random.Random(0))[1][0]) == 40.0
