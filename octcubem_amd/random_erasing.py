"""Random erasing on the device: the counterpart of the reference's OCTCube/util/random_erasing.py (timm's RandomErasing), with its
constructor, for normalised batches that are already on the GPU.

The boxes are drawn from ``random`` on the host in the reference's order -- ``random() > probability``, the count, then per box up to
10 tries (100 in the cube path) of ``uniform`` area, ``uniform`` log aspect ratio and, when the box fits, ``randint`` top and left --
so with the same seed they are the reference's boxes.  The fill is zeros (``const``), one normal draw per channel (``rand``) or per
pixel (``pixel``), drawn with torch ON THE DEVICE, one draw per box (per image and box in the cube path) in the reference's order:
the device's random stream, not the CPU stream a reference worker would use.  The assignment is a plain slice assignment: at most a
third of a quarter of the images is touched, which is no hot path.

``last_boxes`` holds what the last call erased: (image index, top, left, h, w) per box."""
from __future__ import annotations

import math
import random as _random

import torch


def _get_pixels(per_pixel, rand_color, patch_size, dtype=torch.float32, device="cuda"):
    if per_pixel:
        return torch.empty(patch_size, dtype=dtype, device=device).normal_()
    if rand_color:
        return torch.empty((patch_size[0], 1, 1), dtype=dtype, device=device).normal_()
    return torch.zeros((patch_size[0], 1, 1), dtype=dtype, device=device)


class RandomErasing:
    """probability: of erasing an image (the whole batch in the cube path); min_area / max_area: of a box relative to the image, divided
    by the count; min_aspect / max_aspect: of a box; mode: 'const', 'rand' or 'pixel'; min_count / max_count: boxes per image;
    num_splits: > 1 leaves the first batch // num_splits images clean; cube: one set of boxes for the whole batch (the reference's
    default for volumes) instead of one per image; random: the stream (default the global ``random`` module)."""

    def __init__(self, probability=0.5, min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None, mode="const", min_count=1,
                 max_count=None, num_splits=0, device="cuda", cube=True, random=None):
        self.probability = probability
        self.min_area = min_area
        self.max_area = max_area
        max_aspect = max_aspect or 1 / min_aspect
        self.log_aspect_ratio = (math.log(min_aspect), math.log(max_aspect))
        self.min_count = min_count
        self.max_count = max_count or min_count
        self.num_splits = num_splits
        mode = mode.lower()
        self.rand_color = mode == "rand"
        self.per_pixel = mode == "pixel"
        assert self.rand_color or self.per_pixel or not mode or mode == "const"
        self.cube = cube
        self.device = device
        self.random = random if random is not None else _random
        self.last_boxes = []

    def _draw_boxes(self, img_h, img_w, tries):
        """The reference's draws for one image (or one cube): the list of (top, left, h, w)."""
        rnd = self.random
        if rnd.random() > self.probability:
            return []
        area = img_h * img_w
        count = self.min_count if self.min_count == self.max_count else rnd.randint(self.min_count, self.max_count)
        boxes = []
        for _ in range(count):
            for _ in range(tries):
                target_area = rnd.uniform(self.min_area, self.max_area) * area / count
                aspect_ratio = math.exp(rnd.uniform(*self.log_aspect_ratio))
                h = int(round(math.sqrt(target_area * aspect_ratio)))
                w = int(round(math.sqrt(target_area / aspect_ratio)))
                if w < img_w and h < img_h:
                    top = rnd.randint(0, img_h - h)
                    left = rnd.randint(0, img_w - w)
                    boxes.append((top, left, h, w))
                    break
        return boxes

    def _fill(self, img, chan, box, dtype):
        top, left, h, w = box
        img[:, top:top + h, left:left + w] = _get_pixels(self.per_pixel, self.rand_color, (chan, h, w), dtype=dtype, device=img.device)

    def _erase(self, img, index, chan, img_h, img_w, dtype):
        for box in self._draw_boxes(img_h, img_w, 10):
            self._fill(img, chan, box, dtype)
            self.last_boxes.append((index, *box))

    def _erase_cube(self, img, batch_start, batch_size, chan, img_h, img_w, dtype):
        for box in self._draw_boxes(img_h, img_w, 100):
            for i in range(batch_start, batch_size):
                self._fill(img[i], chan, box, dtype)
                self.last_boxes.append((i, *box))

    @torch.no_grad()
    def __call__(self, input):
        """[C, H, W] or [B, C, H, W], erased in place and returned."""
        self.last_boxes = []
        if input.dim() == 3:
            self._erase(input, 0, *input.shape, input.dtype)
            return input
        batch_size, chan, img_h, img_w = input.shape
        batch_start = batch_size // self.num_splits if self.num_splits > 1 else 0
        if self.cube:
            self._erase_cube(input, batch_start, batch_size, chan, img_h, img_w, input.dtype)
        else:
            for i in range(batch_start, batch_size):
                self._erase(input[i], i, chan, img_h, img_w, input.dtype)
        return input
