"""GPU: RandAugment's image operations (csrc/augment2d.hip, ops.image_stats / ops.image_augment, octcubem_amd.rand_augment,
octcubem_amd.random_erasing, transforms.build_transform) against the numpy restatement of the Pillow operations
(tests/augment2d_ref.py, pinned to Pillow by tests/test_cpu_augment2d.py).

Every comparison is bit for bit (torch.equal): the uint8 form against the restatement, the float32 form against the ToTensor ->
Normalize table looked up at the uint8 form.  The kernels evaluate Pillow's float and double expressions operation by operation,
without contraction, so there is no tolerance to derive."""
import random
import types
from functools import lru_cache

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import ops
    from octcubem_amd import rand_augment as RA
    from octcubem_amd.transforms import build_transform, create_2d_transforms, normalize_lut
from tests import augment2d_ref as R
from tests import transform2d_ref as R2

FILL = (124, 116, 104)
# one pixel, thinner than the filters, border only (sharpness), odd, a whole number of tiles, one pixel past a tile both ways
SHAPES = [(1, 1), (2, 7), (3, 3), (37, 53), (64, 64), (65, 130)]


def _boundary_ops():
    """Every kind at every boundary argument, both interpolations: (name, args, interpolation), None = no op."""
    out = [None]
    for interp in (R.BILINEAR, R.BICUBIC):
        out += [("Rotate", (a,), interp) for a in (0.0, 30.0, -30.0)]
        out += [(n, (a,), interp) for n in ("ShearX", "ShearY") for a in (0.3, -0.3)]
        out += [(n, (a,), interp) for n in ("TranslateXRel", "TranslateYRel") for a in (0.0, 0.45, -0.45)]
    out += [("Posterize", (b,), None) for b in range(5)]
    out += [("Solarize", (t,), None) for t in (0, 1, 255, 256)]
    out += [("SolarizeAdd", (a,), None) for a in (0, 110)]
    out += [(n, (f,), None) for n in ("Color", "Contrast", "Brightness", "Sharpness") for f in (0.1, 1.0, 1.9)]
    out += [("AutoContrast", (), None), ("Equalize", (), None), ("Invert", (), None)]
    return out


BOUNDARY = _boundary_ops()


@lru_cache(maxsize=None)
def _lut():
    return normalize_lut().cuda()


@lru_cache(maxsize=None)
def _boundary_ref(shape):
    """(inputs uint8 [n, H, W, 3], restatement outputs) of the boundary batch at one shape, computed once and shared."""
    H, W = shape
    kinds = ("lowcontrast", "binary", "noise", "ramp", "constant")
    x = np.stack([R.make_input(kinds[i % len(kinds)], 50 + i, H, W) for i in range(len(BOUNDARY))])
    y = np.stack([xi if op is None else R.apply(xi, op[0], op[1], op[2], FILL) for xi, op in zip(x, BOUNDARY)])
    return x, y


def _float_of(u8: torch.Tensor) -> torch.Tensor:
    """The table lookup of a uint8 [n, H, W, 3] result: float32 [n, 3, H, W]."""
    lut = normalize_lut()
    return torch.stack([lut[c][u8[..., c].long()] for c in range(3)], dim=1)


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_every_kind_at_its_boundary_arguments_in_one_launch(shape):
    H, W = shape
    x, y = _boundary_ref(shape)
    xg = torch.from_numpy(x).cuda()
    decisions = [[] if op is None else [op] for op in BOUNDARY]
    desc = RA.describe(decisions, 0, H, W, FILL)
    kinds = set(desc["kind"].tolist())
    assert kinds == {ops.AUG_NONE, ops.AUG_TABLE, ops.AUG_COLOR, ops.AUG_SHARPNESS, ops.AUG_AFFINE}
    need = ops.aug_needs_stats(desc)
    assert 0 < int(need.sum()) < len(BOUNDARY)            # Contrast x 3, AutoContrast, Equalize -- and nobody else
    hist = ops.image_stats(xg, needed=need)
    want_hist = np.stack([R.stats(xi) if f else np.zeros((4, 256), np.uint32) for xi, f in zip(x, need)])
    assert np.array_equal(hist.cpu().numpy().view(np.uint32), want_hist)
    got = ops.image_augment(xg, desc, hist=hist)
    assert got.dtype == torch.uint8 and got.shape == xg.shape
    bad = [BOUNDARY[i] for i in range(len(BOUNDARY)) if not np.array_equal(got[i].cpu().numpy(), y[i])]
    assert not bad, bad
    assert torch.equal(xg.cpu(), torch.from_numpy(x))       # the source is read only
    gf = ops.image_augment(xg, desc, hist=hist, lut=_lut())
    assert gf.dtype == torch.float32 and gf.shape == (len(BOUNDARY), 3, H, W)
    assert torch.equal(gf.cpu(), _float_of(torch.from_numpy(y)))


def test_stats_of_every_image_over_several_strips():
    x = np.stack([R.make_input(k, 7, 150, 131) for k in ("noise", "lowcontrast", "constant", "ramp")])
    hist = ops.image_stats(torch.from_numpy(x).cuda())
    assert hist.dtype == torch.int32 and hist.shape == (4, 4, 256)
    assert np.array_equal(hist.cpu().numpy().view(np.uint32), np.stack([R.stats(xi) for xi in x]))
    # into a given tensor, twice: the launch clears what it adds to
    out = torch.full((4, 4, 256), 9, dtype=torch.int32, device="cuda")
    ops.image_stats(torch.from_numpy(x).cuda(), out=out)
    assert torch.equal(out, hist)


def test_argument_checks_of_the_wrappers():
    x = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device="cuda")
    desc = np.zeros(2, dtype=ops.AUG_DESC)
    with pytest.raises(RuntimeError):
        ops.image_augment(x, desc, out=x)                                   # in place
    with pytest.raises(RuntimeError):
        ops.image_augment(x, desc[:1])
    desc["kind"][1], desc["mode"][1] = ops.AUG_TABLE, ops.AUG_LUT_EQUALIZE
    with pytest.raises(RuntimeError):
        ops.image_augment(x, desc)                                          # no histograms
    desc["mode"][1] = 9
    with pytest.raises(RuntimeError):
        ops.image_augment(x, desc, hist=ops.image_stats(x))                 # refused by the entry point, before a launch
    with pytest.raises(RuntimeError):
        ops.image_stats(x, needed=[True])


def test_rand_augment_layers_random_interpolation_and_weights():
    """The object itself on a uint8 batch: three layers, ops skipped (shorter lists), both interpolations drawn, the weighted choice."""
    H, W, n = 37, 53, 6
    x = np.stack([R.make_input(k, 21 + i, H, W) for i, k in enumerate(("lowcontrast", "binary", "noise", "ramp", "lowcontrast", "binary"))])
    xg = torch.from_numpy(x).cuda()
    for cfg, seed in (("rand-m7-n3-mstd1-w0", 3), ("rand-m9-mstd0.5-inc1", 4), ("rand-n4", 5)):
        t = RA.rand_augment_transform(cfg, dict(translate_const=20, img_mean=FILL), random=random.Random(seed),
                                      np_random=np.random.RandomState(seed))
        got = t.batch(xg)
        dec = t.last_params
        assert len(dec) == n and max(len(d) for d in dec) >= 2
        want = np.stack([R.apply_chain(xi, d, FILL) for xi, d in zip(x, dec)])
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), (cfg, dec)
        assert torch.equal(t.apply(xg, dec, lut=_lut()).cpu(), _float_of(torch.from_numpy(want)))
        one = t(xg[0])
        assert np.array_equal(one.cpu().numpy(), R.apply_chain(x[0], t.last_params, FILL))
    # nothing drawn: the images themselves, or the table alone
    t = RA.RandAugment([], 0)
    assert t.apply(xg, [[]] * n) is xg
    assert torch.equal(t.apply(xg, [[]] * n, lut=_lut()).cpu(), _float_of(torch.from_numpy(x)))
    assert torch.equal(xg.cpu(), torch.from_numpy(x))


def _args(**kw):
    base = dict(input_size=224, aa="rand-m9-mstd0.5-inc1", reprob=0.25, remode="pixel", recount=1, color_jitter=None)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _raw_batch(n, H=300, W=260):
    return [R.make_input(("lowcontrast", "noise", "ramp", "binary")[i % 4], 70 + i, H, W) for i in range(n)]


def test_train_chain_of_eight_images_equals_the_restatement_driven_by_the_same_decisions():
    raw = _raw_batch(8)
    random.seed(8)
    np.random.seed(8)
    torch.manual_seed(8)                                    # the device stream of the erasing noise as well
    t = build_transform("train", _args(), generator=torch.Generator().manual_seed(1))
    out = t.batch(raw)
    assert out.shape == (8, 3, 224, 224) and out.dtype == torch.float32 and out.is_cuda
    params = t.last_params
    names = {op[0] for p in params for op in p["ops"]}
    assert names & set(R.GEOMETRIC) and names & {"AutoContrast", "Equalize", "ContrastIncreasing"}, names
    boxes = [(b, *box) for b, p in enumerate(params) for box in p["erased"]]
    assert boxes, "the seeds of this test erase at least one box"
    want = []
    for x, p in zip(raw, params):
        y = R2.resize(x, (224, 224), p["crop"])
        y = np.ascontiguousarray(y[:, ::-1]) if p["flip"] else y
        want.append(R.apply_chain(y, p["ops"], FILL))
    want = _float_of(torch.from_numpy(np.stack(want)))
    inside = torch.zeros(out.shape, dtype=torch.bool)
    torch.manual_seed(8)
    got = out.cpu()
    for b, top, left, h, w in boxes:
        inside[b, :, top:top + h, left:left + w] = True
        noise = torch.empty((3, h, w), dtype=torch.float32, device="cuda").normal_()        # one draw per box, in order
        assert torch.equal(got[b, :, top:top + h, left:left + w], noise.cpu()), (b, top, left, h, w)
    assert torch.equal(got[~inside], want[~inside])
    # the same seeds, the same batch
    random.seed(8)
    np.random.seed(8)
    torch.manual_seed(8)
    t2 = build_transform("train", _args(), generator=torch.Generator().manual_seed(1))
    assert torch.equal(t2.batch(raw), out) and t2.last_params == params


def test_eval_chain_and_erasing_alone():
    raw = _raw_batch(2, 200, 170)
    t = build_transform("val", _args(input_size=64))
    out = t.batch(raw)
    full = int(64 / (224 / 256))
    top = int(round((full - 64) / 2.0))
    want = np.stack([R2.resize(x, (full, full))[top:top + 64, top:top + 64] for x in raw])
    assert out.shape == (2, 3, 64, 64) and torch.equal(out.cpu(), _float_of(torch.from_numpy(want)))
    assert t.last_params == [{"crop": None, "flip": False, "ops": []}] * 2
    # a grey image goes through convert("RGB"); erasing without RandAugment, constant fill
    grey = raw[0][..., 0].copy()
    random.seed(2)
    t = build_transform("train", _args(aa=None, reprob=1.0, remode="const", input_size=48), generator=torch.Generator().manual_seed(3))
    out = t.batch([grey, raw[1]]).cpu()
    p = t.last_params
    assert all(len(q["erased"]) == 1 and q["ops"] == [] for q in p)
    for b, x in enumerate((np.stack([grey] * 3, axis=-1), raw[1])):
        y = R2.resize(x, (48, 48), p[b]["crop"])
        w = _float_of(torch.from_numpy((np.ascontiguousarray(y[:, ::-1]) if p[b]["flip"] else y)[None]))[0]
        tp, lf, h, ww = p[b]["erased"][0]
        w[:, tp:tp + h, lf:lf + ww] = 0.0
        assert torch.equal(out[b], w), b


def test_old_arguments_make_the_launches_they_made(monkeypatch):
    """create_2d_transforms with the arguments it always had: image_resample launches only -- one for a plain stack, one per image with
    crops -- and the result of the resize chain."""
    calls = []
    real = ops.image_resample

    def counted(*a, **kw):
        calls.append("image_resample")
        return real(*a, **kw)

    def refuse(*a, **kw):
        raise AssertionError("an augmentation launch in the plain chain")
    monkeypatch.setattr(ops, "image_resample", counted)
    monkeypatch.setattr(ops, "image_augment", refuse)
    monkeypatch.setattr(ops, "image_stats", refuse)
    raw = np.stack(_raw_batch(3, 90, 70))
    out = create_2d_transforms(64).batch(raw)
    assert calls == ["image_resample"]
    want = torch.stack([R2.to_tensor_normalize(R2.resize(x, (64, 64))) for x in raw])
    assert torch.equal(out.cpu(), want)
    del calls[:]
    t = create_2d_transforms(64, random_resized_crop=True, hflip_prob=0.5, generator=torch.Generator().manual_seed(0))
    out = t.batch(raw)
    assert calls == ["image_resample"] * 3
    for b, p in enumerate(t.last_params):
        assert set(p) == {"crop", "flip"}
        w = R2.to_tensor_normalize(R2.resize(raw[b], (64, 64), p["crop"]))
        assert torch.equal(out[b].cpu(), w.flip(2) if p["flip"] else w)
