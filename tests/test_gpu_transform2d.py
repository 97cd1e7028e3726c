"""GPU: the fused 2-D image transforms (csrc/image2d.hip, ops.image_resample, octcubem_amd.transforms.create_2d_transforms) against
the numpy restatement of Pillow's 8-bit bicubic resize (tests/transform2d_ref.py, pinned to Pillow by tests/test_cpu_transform2d.py).

Every comparison is bit for bit (torch.equal): the uint8 form against the restatement, the float32 form against the float chain
ToTensor -> Normalize applied to the restatement's uint8.  The arithmetic is integer after the coefficients, and the coefficients are
IEEE double evaluated without contraction, so there is no tolerance to derive."""
from functools import lru_cache

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import ops
    from octcubem_amd.transforms import DeviceTransformLoader, create_2d_transforms, normalize_lut
from tests import transform2d_ref as R

SINGLE = [n for n in R.CASES if "stack" not in n]
MEAN, STD = R.IMAGENET_MEAN, R.IMAGENET_STD


@lru_cache(maxsize=None)
def _ref(name):
    """(input, restatement uint8, float chain on it) of a case, computed once and shared."""
    _, _, _, crop, size = R.CASES[name]
    x = R.case_input(name)
    y = R.resize(x, size, crop)
    return x, y, R.to_tensor_normalize(y, MEAN, STD)


@lru_cache(maxsize=None)
def _lut():
    return normalize_lut(MEAN, STD).cuda()


@pytest.mark.parametrize("flip", [False, True], ids=["noflip", "flip"])
@pytest.mark.parametrize("name", SINGLE)
def test_image_resample_equals_pillow_bit_for_bit(name, flip):
    _, _, _, crop, size = R.CASES[name]
    x, y, f = _ref(name)
    if name.startswith("binary"):            # the restatement itself clamped in both passes, on both sides
        stats = {}
        R.resize(x, size, crop, stats=stats)
        assert min(stats[k] for k in ("h_below", "h_above", "v_below", "v_above")) >= 1, stats
    xg = torch.from_numpy(x).cuda()
    want_u8 = torch.from_numpy(y).flip(1) if flip else torch.from_numpy(y)   # torch's flip copies: numpy's reversed view of one column keeps a negative stride
    want_f = f.flip(2) if flip else f
    got = ops.image_resample(xg, size, crop=crop, flip=flip)
    assert got.dtype == torch.uint8 and got.shape == want_u8.shape
    assert torch.equal(got.cpu(), want_u8)
    got = ops.image_resample(xg, size, crop=crop, flip=flip, lut=_lut())
    assert got.dtype == torch.float32 and got.shape == (1, 3, *size)
    assert torch.equal(got[0].cpu(), want_f)


@pytest.mark.parametrize("prefix", ["stack", "rgbstack"])
def test_image_resample_batch_stride(prefix):
    names = [f"{prefix}{i}_37x53_to_64x32" for i in range(3)]
    size = R.CASES[names[0]][4]
    x = torch.from_numpy(np.stack([_ref(n)[0] for n in names])).cuda()
    want_u8 = torch.from_numpy(np.stack([_ref(n)[1] for n in names]))
    want_f = torch.stack([_ref(n)[2] for n in names])
    assert torch.equal(ops.image_resample(x, size).cpu(), want_u8)
    assert torch.equal(ops.image_resample(x, size, lut=_lut()).cpu(), want_f)
    # into a slice of a larger output, flipped and cropped: the offsets of src and dst together
    crop = (3, 4, 30, 40)
    out = torch.full((5, 3, *size), 7.0, device="cuda")
    ops.image_resample(x, size, crop=crop, flip=True, lut=_lut(), out=out[1:4])
    for i, n in enumerate(names):
        y = R.resize(_ref(n)[0], size, crop)
        assert torch.equal(out[1 + i].cpu(), R.to_tensor_normalize(y, MEAN, STD).flip(2)), n
    assert float(out[0].min()) == 7.0 and float(out[4].max()) == 7.0


def test_image2d_transform_input_forms_batches_and_autocast():
    name = "noise_124x256_to_128x128"
    x, _, f = _ref(name)
    t = create_2d_transforms(128)
    a = t(x)
    assert a.is_cuda and a.dtype == torch.float32 and a.shape == (3, 128, 128) and not a.requires_grad
    assert torch.equal(a.cpu(), f) and t.last_params == {"crop": None, "flip": False}
    assert torch.equal(t(torch.from_numpy(x)), a) and torch.equal(t(torch.from_numpy(x).cuda()), a)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        assert torch.equal(t(Image.fromarray(x)), a)
        rgb = _ref("rgb_37x53_to_64x32")
        t64 = create_2d_transforms((64, 32))
        assert torch.equal(t64(Image.fromarray(rgb[0])).cpu(), rgb[2])
        assert torch.equal(t64(Image.fromarray(rgb[0]).convert("RGBA")).cpu(), rgb[2])      # any other mode goes through convert("RGB")
    with torch.cuda.amp.autocast():
        assert torch.equal(t(x), a)
    # equal shapes, no crop, no flip: one launch over the stack, equal to the per-image calls; list, array and tensor stacks alike
    names = [f"stack{i}_37x53_to_64x32" for i in range(3)]
    t64 = create_2d_transforms((64, 32))
    want = torch.stack([_ref(n)[2] for n in names])
    imgs = [_ref(n)[0] for n in names]
    assert torch.equal(t64.batch(imgs).cpu(), want) and t64.last_params == [{"crop": None, "flip": False}] * 3
    assert torch.equal(torch.stack([t64(i) for i in imgs]).cpu(), want)
    assert torch.equal(t64.batch(np.stack(imgs)).cpu(), want) and torch.equal(t64.batch(torch.from_numpy(np.stack(imgs)).cuda()).cpu(), want)
    # mixed shapes with crops and flips drawn: equal to the raw op called with last_params, which holds in-image crops and both flip values
    tr = create_2d_transforms(32, mean=0.5, std=0.25, random_resized_crop=True, hflip_prob=0.5, generator=torch.Generator().manual_seed(1))
    mixed = [_ref(n)[0] for n in ("binary_37x53_to_64x32", "noise_70x90_to_8x8", "rgb_37x53_to_64x32", "noise_5x7_to_16x16",
                                  "binary_61x100_to_50x70", "noise_64x64_to_64x48")]
    got = tr.batch(mixed)
    assert got.shape == (6, 3, 32, 32) and len(tr.last_params) == 6
    assert {p["flip"] for p in tr.last_params} == {False, True}
    lut = normalize_lut(0.5, 0.25).cuda()
    for i, (im, p) in enumerate(zip(mixed, tr.last_params)):
        top, left, h, w = p["crop"]
        assert 0 <= top and 0 <= left and top + h <= im.shape[0] and left + w <= im.shape[1]
        raw = ops.image_resample(torch.from_numpy(im).cuda(), (32, 32), crop=p["crop"], flip=p["flip"], lut=lut)
        assert torch.equal(got[i], raw[0])
        y = R.resize(im, (32, 32), p["crop"])
        assert torch.equal(got[i].cpu(), R.to_tensor_normalize(y, 0.5, 0.25).flip(2) if p["flip"] else R.to_tensor_normalize(y, 0.5, 0.25))


def test_device_transform_loader():
    names = [f"stack{i}_37x53_to_64x32" for i in range(3)]
    imgs = [_ref(n)[0] for n in names]
    want = torch.stack([_ref(n)[2] for n in names])
    loader = [(imgs[:2], "a", 1), (np.stack(imgs[1:]), "b", 2)]
    t = create_2d_transforms((64, 32))
    wrapped = DeviceTransformLoader(loader, t)
    assert len(wrapped) == 2
    for _ in range(2):                      # re-iterable, as the engine restarts it when it runs out
        got = list(wrapped)
        assert [b[1:] for b in got] == [("a", 1), ("b", 2)]
        assert got[0][0].is_cuda and torch.equal(got[0][0].cpu(), want[:2]) and torch.equal(got[1][0].cpu(), want[1:])
    got = list(DeviceTransformLoader([{"x": 3, "img": imgs[:1]}], t, index="img"))
    assert got[0]["x"] == 3 and torch.equal(got[0]["img"].cpu(), want[:1])
