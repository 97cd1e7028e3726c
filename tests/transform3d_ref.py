"""Plain torch CPU restatement of the reference's volume pipeline (Pre-training/custom_util/PatientDataset_inhouse.py:48-84: MONAI
CropForegroundd -> Resized(trilinear) -> RandFlipd(0) -> RandFlipd(2) -> NormalizeIntensityd(nonzero)), from the calls MONAI itself
makes: the yardstick of tests/test_cpu_transform3d.py and tests/test_gpu_transform3d.py.

A note for whoever reads a failure near the bound at a 61 -> 60 axis: F.interpolate's source coordinate, scale * (dst + 0.5) - 0.5, is
ONE fused multiply-add in ATen's AVX2 / AVX512 CPU kernels (they are compiled with contraction), and the HIP kernel computes it the same
way -- the two then agree to ~1e-7 of the range.  On a host where ATen runs its DEFAULT CPU capability (no FMA; ATEN_CPU_CAPABILITY=default)
this reference rounds the multiply and the subtract separately: the coordinate near 60 moves by an ulp (3.8e-6), the weight inherits it
whole, and the 61 -> 60 cases then sit at 1.4e-6 .. 1.9e-6 of the range -- still inside the 2e-6 bound, but close to it for a reason
that is the host's, not the kernel's."""
import torch
import torch.nn.functional as F


def box(x):
    """x [1, D, H, W] -> (d0, d1, h0, h1, w0, w1), half-open: the bounding box of the voxels > 0 (CropForegroundd's default select_fn,
    margin 0); the full extent when there is none."""
    nz = (x[0] > 0).nonzero()
    if nz.numel() == 0:
        D, H, W = x.shape[1:]
        return (0, D, 0, H, 0, W)
    lo, hi = nz.min(0).values, nz.max(0).values + 1
    return (int(lo[0]), int(hi[0]), int(lo[1]), int(hi[1]), int(lo[2]), int(hi[2]))


def resize(x, size, crop=False):
    """x [1, D, H, W] -> float32 [1, T, OH, OW]: the (cropped) volume through F.interpolate, as MONAI's Resized calls it."""
    x = x.cpu()
    if crop:
        d0, d1, h0, h1, w0, w1 = box(x)
        x = x[:, d0:d1, h0:h1, w0:w1]
    return F.interpolate(x[None].float(), size=tuple(size), mode="trilinear", align_corners=False)[0]


def flip(y, flips):
    if flips[0]:
        y = y.flip(1)
    if flips[1]:
        y = y.flip(3)
    return y


def normalize(y, sub=0.25, div=0.25):
    """NormalizeIntensityd(subtrahend, divisor, nonzero=True)."""
    return torch.where(y != 0, (y - sub) / div, y)


def pipeline(x, size, crop=False, flips=(False, False), norm=None):
    y = flip(resize(x, size, crop), flips)
    return y if norm is None else normalize(y, *norm)
