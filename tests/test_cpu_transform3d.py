"""CPU side of the volume transforms: the torch restatement of the reference's MONAI chain (tests/transform3d_ref.py) on a case worked
out by hand, the argument errors of the two C-ABI entry points (reported before any launch), and the host logic of
octcubem_amd.transforms that needs no GPU."""
import ctypes

import pytest
import torch

from tests import transform3d_ref as R


def _ramp():
    # x[d, h, w] = 4 d + 2 h + w: linear in every coordinate, so trilinear interpolation reproduces the same plane
    return torch.arange(8, dtype=torch.float32).view(1, 2, 2, 2)


def test_restatement_on_a_hand_written_2x2x2_to_3x3x3_case():
    """in 2 -> out 3, align_corners=False: scale 2/3, src = max(2/3 (dst + 0.5) - 0.5, 0) = 0, 0.5, 1.1667 -> taps (0, 1, w 0), (0, 1, w 0.5),
    (1, 1): per axis out = (x0, (x0 + x1) / 2, x1), i.e. the plane sampled at coordinates 0, 0.5, 1."""
    x = _ramp()
    c = torch.tensor([0.0, 0.5, 1.0])
    want = (4 * c[:, None, None] + 2 * c[None, :, None] + c[None, None, :])[None]
    y = R.resize(x, (3, 3, 3))
    assert y.shape == (1, 3, 3, 3) and y.dtype == torch.float32
    assert float((y - want).abs().max()) <= 1e-6
    assert torch.equal(R.resize(x.to(torch.uint8), (3, 3, 3)), y)              # uint8 goes through .float()
    assert torch.equal(R.resize(x, (2, 2, 2)), x)                              # identity: every weight exactly 0
    # flips reverse the first / last spatial axis of the result
    f = R.pipeline(x, (3, 3, 3), flips=(True, False))
    assert torch.equal(f, y.flip(1)) and float((f[0, 0, 0, 0] - 4.0).abs()) <= 1e-6
    f = R.pipeline(x, (3, 3, 3), flips=(True, True))
    assert torch.equal(f, y.flip(1).flip(3)) and float((f[0, 0, 0, 0] - 5.0).abs()) <= 1e-6
    # NormalizeIntensityd(0.25, 0.25, nonzero=True): the one exact zero (the corner voxel) stays, everything else is 4 y - 1
    n = R.pipeline(x, (3, 3, 3), norm=(0.25, 0.25))
    assert float(n[0, 0, 0, 0]) == 0.0 and int((n == 0).sum()) == 1
    assert float((n - torch.where(want != 0, 4 * want - 1, want)).abs().max()) <= 4e-6


def test_restatement_box_and_crop():
    x = torch.zeros(1, 4, 5, 6)
    assert R.box(x) == (0, 4, 0, 5, 0, 6)                                      # no foreground: the full extent
    x[0, 1, 2, 3] = 2.0
    assert R.box(x) == (1, 2, 2, 3, 3, 4)
    x[0, 2, 4, 1] = 1.0
    x[0, 0, 0, 0] = -3.0                                                       # negative values are background
    assert R.box(x) == (1, 3, 2, 5, 1, 4)
    # the crop is the box's sub-volume: resizing it to its own size returns it
    assert torch.equal(R.resize(x, (2, 3, 3), crop=True), x[:, 1:3, 2:5, 1:4])
    r = _ramp()
    r[0, 0] = 0                                                                # first slab empty -> box d0 = 1; the rest is one slab
    assert R.box(r) == (1, 2, 0, 2, 0, 2)
    assert torch.equal(R.resize(r, (3, 2, 2), crop=True), r[:, 1:2].expand(1, 3, 2, 2))


def test_volume_entry_points_report_argument_errors_without_a_gpu():
    from octcubem_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)                 # never dereferenced: every call below is refused before a launch
    assert lib.octmae_volume_box(None, 0, 4, 4, 4, p, None) == -1
    assert lib.octmae_volume_box(p, 0, 4, 4, 4, None, None) == -1
    for D, H, W in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        assert lib.octmae_volume_box(p, 1, D, H, W, p, None) == -1
    assert lib.octmae_volume_box(p, 2, 4, 4, 4, p, None) == -2
    assert lib.octmae_volume_box(p, -1, 4, 4, 4, p, None) == -2
    assert lib.octmae_volume_resample(None, 0, 4, 4, 4, None, p, 2, 2, 2, 0, 0, 0, 0.0, 1.0, None) == -1
    assert lib.octmae_volume_resample(p, 0, 4, 4, 4, None, None, 2, 2, 2, 0, 0, 0, 0.0, 1.0, None) == -1
    for dims in ((0, 4, 4, 2, 2, 2), (4, 4, 4, 0, 2, 2), (4, 4, 4, 2, -2, 2), (4, 4, 4, 2, 2, 0), (4, 0, 4, 2, 2, 2)):
        D, H, W, T, OH, OW = dims
        assert lib.octmae_volume_resample(p, 1, D, H, W, None, p, T, OH, OW, 0, 0, 0, 0.0, 1.0, None) == -1
    assert lib.octmae_volume_resample(p, 2, 4, 4, 4, None, p, 2, 2, 2, 0, 0, 0, 0.0, 1.0, None) == -2
    with pytest.raises(_lib.OctmaeError, match="bad argument"):
        _lib.call("octmae_volume_box", None, 0, 4, 4, 4, None, None)


def test_create_3d_transforms_host_side():
    from octcubem_amd import ops
    from octcubem_amd.transforms import create_3d_transforms
    g = torch.Generator().manual_seed(3)
    train, val = create_3d_transforms(256, num_frames=60, RandRotate90d_prob=0.3, generator=g, some_future_keyword=1)
    assert train.size == (60, 256, 256) and val.size == (60, 256, 256)
    assert train.crop and not val.crop and train.normalize is None and val.flip_prob is None
    train, val = create_3d_transforms(128)
    assert train.size == (64, 128, 128)
    train, val = create_3d_transforms((32, 48), num_frames=6, normalize=True)
    assert val.size == (6, 32, 48) and train.normalize == (0.25, 0.25) and val.normalize == (0.25, 0.25)
    # shape errors are raised before anything is moved to a GPU
    for bad in (torch.zeros(2, 3, 4, 4), torch.zeros(3, 4, 4), torch.zeros(1, 1, 3, 4, 4)):
        with pytest.raises(ValueError):
            val({"pixel_values": bad})
    # the flips are drawn on the host, d first, then w, from the generator given
    train, _ = create_3d_transforms(32, num_frames=6, generator=torch.Generator().manual_seed(11))
    want = torch.rand(2, generator=torch.Generator().manual_seed(11)) < 0.5
    assert train._draw_flips() == (bool(want[0]), bool(want[1]))
    assert create_3d_transforms(32, RandFlipd_prob=0.0)[0]._draw_flips() == (False, False)
    assert create_3d_transforms(32, RandFlipd_prob=1.0)[0]._draw_flips() == (True, True)
    # the kernels have no CPU form: a CPU tensor handed to the raw ops is an error, not a fall-back
    with pytest.raises(RuntimeError):
        ops.volume_box(torch.zeros(2, 2, 2))
    with pytest.raises(RuntimeError):
        ops.volume_resample(torch.zeros(2, 2, 2), (2, 2, 2))
