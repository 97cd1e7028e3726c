"""Volume transforms: the drop-in counterpart of the reference's ``create_3d_transforms``
(Pre-training/custom_util/PatientDataset_inhouse.py:48-84, the pipeline inference_utils.py:10 imports), on the GPU.

The reference composes MONAI dictionary transforms on the CPU:

  train   CropForegroundd -> Resized(trilinear) -> RandFlipd(axis 0) -> RandFlipd(axis 2) [-> NormalizeIntensityd(0.25, 0.25, nonzero)]
  val     Resized(trilinear) [-> NormalizeIntensityd(0.25, 0.25, nonzero)]

Here val is one launch over the raw scan and train four (csrc/transform3d.hip): ops.volume_box (three launches: initialise, reduce,
finish) leaves the foreground box in device memory, ops.volume_resample (one launch) reads it there and does the crop (an offset), the
resize (8 taps per output voxel), the flips (an index reversal) and the normalisation (an epilogue) in one pass.  Nothing returns to the
host in between.

Deviations from the reference, both deliberate:
  * a volume without a voxel > 0 is resized whole (MONAI fails on the empty crop);
  * the flip decisions come from ``torch.rand(2, generator=generator) < prob`` on the host (first axis 0, then axis 2), not from MONAI's
    numpy RandomState: the same distribution, another stream.  ``last_flips`` holds the decisions of the last call.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from . import ops

KEY = "pixel_values"
NORMALIZE = (0.25, 0.25)        # NormalizeIntensityd(subtrahend=0.25, divisor=0.25, nonzero=True), as the reference hard-codes


class Volume3DTransform:
    """Callable on the reference's dict: ``t({"pixel_values": x})["pixel_values"]`` with x [1, D, H, W] (CPU or GPU; uint8 and float32
    go to the kernels as they are, anything else through ``.float()``) -> float32 [1, T, OH, OW] on the GPU, without grad."""

    def __init__(self, size: Tuple[int, int, int], crop: bool, flip_prob: Optional[float], normalize: bool,
                 generator: Optional[torch.Generator] = None):
        self.size = tuple(int(s) for s in size)
        self.crop = crop
        self.flip_prob = flip_prob              # None: the pipeline has no RandFlipd (val)
        self.normalize = NORMALIZE if normalize else None
        self.generator = generator
        self.last_flips = (False, False)

    def _draw_flips(self) -> Tuple[bool, bool]:
        if self.flip_prob is None:
            return (False, False)
        r = torch.rand(2, generator=self.generator) < self.flip_prob
        return (bool(r[0]), bool(r[1]))

    @staticmethod
    def _volume(x) -> torch.Tensor:
        x = torch.as_tensor(x)
        if x.dim() != 4 or x.shape[0] != 1:
            raise ValueError(f"{KEY}: expected one channel-first volume [1, D, H, W], got {tuple(x.shape)}")
        x = x.detach()
        if x.dtype not in (torch.uint8, torch.float32):
            x = x.float()
        if not x.is_cuda:
            x = x.cuda()
        return x[0].contiguous()

    def _run(self, vol: torch.Tensor, out: torch.Tensor, flips: Tuple[bool, bool]):
        if vol.device != out.device:
            raise ValueError(f"{KEY}: volumes of one batch must live on one device ({vol.device} and {out.device})")
        box = ops.volume_box(vol) if self.crop else None
        ops.volume_resample(vol, self.size, box=box, flip_d=flips[0], flip_w=flips[1], normalize=self.normalize, out=out)

    @torch.no_grad()
    def __call__(self, data: dict) -> dict:
        vol = self._volume(data[KEY])
        flips = self._draw_flips()
        out = torch.empty((1, *self.size), dtype=torch.float32, device=vol.device)
        with torch.cuda.device(vol.device):
            self._run(vol, out[0], flips)
        self.last_flips = flips
        d = dict(data)
        d[KEY] = out
        return d

    @torch.no_grad()
    def batch(self, volumes: Sequence) -> torch.Tensor:
        """A list of [1, D, H, W] volumes (shapes and dtypes may differ) -> float32 [B, 1, T, OH, OW]: per-sample launches on the current
        stream into slices of one output tensor.  ``last_flips`` is then the list of the samples' decisions, drawn in order."""
        vols: List[torch.Tensor] = [self._volume(v) for v in volumes]
        if not vols:
            raise ValueError("batch: no volumes")
        out = torch.empty((len(vols), 1, *self.size), dtype=torch.float32, device=vols[0].device)
        flips = []
        with torch.cuda.device(out.device):
            for b, vol in enumerate(vols):
                flips.append(self._draw_flips())
                self._run(vol, out[b, 0], flips[-1])
        self.last_flips = flips
        return out


def create_3d_transforms(input_size, num_frames=64, RandFlipd_prob=0.5, RandRotate90d_prob=0.5, normalize=False, generator=None,
                         **kwargs):
    """(train_transform, val_transform) with the reference's signature plus ``generator`` (the host torch.Generator the flip decisions
    are drawn from; None = the default one).  ``RandRotate90d_prob`` is accepted and unused, as in the reference."""
    if isinstance(input_size, int):
        input_size = (input_size, input_size)       # the reference's 256 -> (256, 256) is the same rule
    size = (int(num_frames), int(input_size[0]), int(input_size[1]))
    train_transform = Volume3DTransform(size, crop=True, flip_prob=float(RandFlipd_prob), normalize=normalize, generator=generator)
    val_transform = Volume3DTransform(size, crop=False, flip_prob=None, normalize=normalize, generator=generator)
    return train_transform, val_transform
