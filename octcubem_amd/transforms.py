"""Volume and image transforms on the GPU.  First the volumes; the 2-D images follow below (``create_2d_transforms``).

Volume transforms: the drop-in counterpart of the reference's ``create_3d_transforms``
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

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
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


# ---- 2-D images --------------------------------------------------------------------------------------------------------------------
# The reference's torchvision chains on PIL images, per image on the CPU:
#   joint pre-training (Pre-training/main_pretrain_oph_joint_2d512_flash_attn.py:313-317)
#       Resize((S, S), interpolation=3) -> ToTensor -> Normalize(ImageNet)
#   2-D MAE pre-training (OCTCube/main_pretrain_oph_new.py:151-156, OCTCube/main_pretrain.py:133-137)
#       RandomResizedCrop(S, scale=(0.2, 1.0), interpolation=3) -> RandomHorizontalFlip -> ToTensor -> Normalize
# Here each is one launch of ops.image_resample (csrc/image2d.hip) over the raw uint8 image: the crop is an offset, the resize is
# Pillow's integer bicubic bit for bit, the flip an index reversal of the store, ToTensor -> Normalize a 3 x 256 table built with the
# reference's own float ops -- so the result is bit-equal to the reference's for the same crop and flip decisions.
# Deviation: those decisions follow torchvision's published rule (RandomResizedCrop.get_params, RandomHorizontalFlip) but are drawn
# from ``generator`` on the host, crop first and flip second per image: the same distribution, not torchvision's random stream.
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def normalize_lut(mean=IMAGENET_MEAN, std=IMAGENET_STD) -> torch.Tensor:
    """ToTensor -> Normalize of the 256 grey levels per channel, float32 [3, 256] on the CPU, computed with the ops the reference's
    chain runs (uint8 -> float32, div(255), sub(mean), div(std)): equal to it bit for bit for any mean / std."""
    mean, std = (tuple(float(v) for v in m) if isinstance(m, (tuple, list)) else (float(m),) * 3 for m in (mean, std))
    if len(mean) != 3 or len(std) != 3:
        raise ValueError(f"mean / std: expected one value or three, got {mean} / {std}")
    g = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    return torch.stack([(g - mean[c]) / std[c] for c in range(3)])


def random_resized_crop_params(height: int, width: int, scale=(0.2, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0),
                               generator: Optional[torch.Generator] = None) -> Tuple[int, int, int, int]:
    """(top, left, h, w) by the rule of torchvision's RandomResizedCrop.get_params: up to ten tries of area = H W U(scale),
    log r ~ U(log ratio), w = round(sqrt(area r)), h = round(sqrt(area / r)), accepted when it fits, then placed uniformly; after ten
    rejections the centred crop of the aspect ratio clamped into ``ratio``."""
    area = height * width
    lo, hi = math.log(ratio[0]), math.log(ratio[1])
    for _ in range(10):
        target = area * float(torch.empty(1).uniform_(scale[0], scale[1], generator=generator))
        r = math.exp(float(torch.empty(1).uniform_(lo, hi, generator=generator)))
        w, h = int(round(math.sqrt(target * r))), int(round(math.sqrt(target / r)))
        if 0 < w <= width and 0 < h <= height:
            top = int(torch.randint(0, height - h + 1, (1,), generator=generator))
            left = int(torch.randint(0, width - w + 1, (1,), generator=generator))
            return top, left, h, w
    in_ratio = float(width) / float(height)
    if in_ratio < min(ratio):
        w = width
        h = min(max(int(round(w / min(ratio))), 1), height)
    elif in_ratio > max(ratio):
        h = height
        w = min(max(int(round(h * max(ratio))), 1), width)
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


class Image2DTransform:
    """Callable on one raw image -- a PIL image (mode L or RGB as it is, any other through ``convert("RGB")``), a numpy array or a
    tensor, uint8 [H, W] or [H, W, 3], on the CPU or the GPU -- and returns float32 [3, S, S] on the GPU, without grad."""

    def __init__(self, size: Tuple[int, int], mean=IMAGENET_MEAN, std=IMAGENET_STD, random_resized_crop: bool = False,
                 scale=(0.2, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), hflip_prob: float = 0.0, generator: Optional[torch.Generator] = None,
                 auto_augment=None, aa_hparams: Optional[dict] = None, re_prob: float = 0.0, re_mode: str = "const", re_count: int = 1,
                 center_crop=None):
        self.size = (int(size[0]), int(size[1]))
        self.random_resized_crop = bool(random_resized_crop)
        self.scale, self.ratio = (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1]))
        self.hflip_prob = float(hflip_prob)
        self.generator = generator
        self.lut = normalize_lut(mean, std)
        self._luts = {}                     # device -> the table there
        self.last_params = None             # {"crop": (top, left, h, w) or None, "flip": bool} of the last call; a list after .batch
        # The fine-tune chain (build_transform): all off by default, and then nothing below changes.  auto_augment: a config string
        # for rand_augment_transform (with aa_hparams) or a RandAugment; its decisions join last_params under "ops".  re_prob > 0:
        # RandomErasing(re_prob, mode=re_mode, max_count=re_count, cube=False) on the normalised batch ("erased" in last_params).
        # center_crop = (h, w): the resize goes to ``size`` and the centre h x w of it is the result (the eval chain).
        if isinstance(auto_augment, str):
            from .rand_augment import rand_augment_transform
            auto_augment = rand_augment_transform(auto_augment, dict(aa_hparams or {}))
        self.auto_augment = auto_augment
        self.random_erasing = None
        if re_prob > 0.0:
            from .random_erasing import RandomErasing
            self.random_erasing = RandomErasing(re_prob, mode=re_mode, max_count=re_count, num_splits=0, cube=False)
        self.center_crop = None if center_crop is None else (int(center_crop[0]), int(center_crop[1]))

    @staticmethod
    def _image(x) -> torch.Tensor:
        if hasattr(x, "convert") and hasattr(x, "mode"):        # a PIL image
            x = np.array(x if x.mode in ("L", "RGB") else x.convert("RGB"))
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x))
        if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or not (x.dim() == 2 or (x.dim() == 3 and x.shape[2] == 3)):
            what = f"{tuple(x.shape)} {x.dtype}" if isinstance(x, torch.Tensor) else type(x).__name__
            raise ValueError(f"image: expected a PIL image or uint8 [H, W] / [H, W, 3], got {what}")
        return x.detach()

    def _draw(self, height: int, width: int) -> dict:
        crop = (random_resized_crop_params(height, width, self.scale, self.ratio, self.generator)
                if self.random_resized_crop else None)
        flip = bool(torch.rand(1, generator=self.generator) < self.hflip_prob) if self.hflip_prob > 0.0 else False
        return {"crop": crop, "flip": flip}

    def _lut_on(self, device) -> torch.Tensor:
        t = self._luts.get(device)
        if t is None:
            t = self._luts[device] = self.lut.to(device)
        return t

    @torch.no_grad()
    def __call__(self, image) -> torch.Tensor:
        out = self.batch([image])[0]
        self.last_params = self.last_params[0]
        return out

    @torch.no_grad()
    def batch(self, images) -> torch.Tensor:
        """A list of images (shapes may differ), or one uint8 array / tensor [B, H, W] or [B, H, W, 3], -> float32 [B, 3, S, S].  One
        launch when every image has the same shape, no crop is drawn and nothing is flipped (the joint recipe's Resize chain);
        otherwise one launch per image into slices of one output.  ``last_params`` is then the list of the images' decisions, drawn
        in order (``__call__`` leaves the one image's dict there)."""
        stack = None
        if isinstance(images, (np.ndarray, torch.Tensor)):
            stack = torch.from_numpy(np.ascontiguousarray(images)) if isinstance(images, np.ndarray) else images.detach()
            if stack.dtype != torch.uint8 or not (stack.dim() == 3 or (stack.dim() == 4 and stack.shape[3] == 3)):
                raise ValueError(f"batch: expected uint8 [B, H, W] or [B, H, W, 3], got {tuple(stack.shape)} {stack.dtype}")
            imgs = list(stack.unbind(0))
        else:
            imgs = [self._image(x) for x in images]
        if not imgs:
            raise ValueError("batch: no images")
        params = [self._draw(int(x.shape[0]), int(x.shape[1])) for x in imgs]
        if self.auto_augment is not None or self.random_erasing is not None or self.center_crop is not None:
            return self._batch_augmented(imgs, params)
        plain = all(p["crop"] is None and not p["flip"] for p in params) and all(x.shape == imgs[0].shape for x in imgs)
        device = next((x.device for x in imgs if x.is_cuda), torch.device("cuda", torch.cuda.current_device()))
        with torch.cuda.device(device):
            out = torch.empty((len(imgs), 3, *self.size), dtype=torch.float32, device=device)
            lut = self._lut_on(device)
            if plain:
                if stack is None:
                    stack = torch.stack(imgs) if len({x.device for x in imgs}) == 1 else torch.stack([x.to(device) for x in imgs])
                ops.image_resample(stack.to(device).contiguous(), self.size, lut=lut, out=out)
            else:
                for b, (x, p) in enumerate(zip(imgs, params)):
                    ops.image_resample(x.to(device).contiguous(), self.size, crop=p["crop"], flip=p["flip"], lut=lut, out=out[b:b + 1])
        self.last_params = params
        return out


    def _batch_augmented(self, imgs, params) -> torch.Tensor:
        """The fine-tune chains: image_resample to uint8 (crop, flip) -> [centre crop] -> the RandAugment layers, whose last launch
        writes through the normalisation table (kind "none" where there is nothing else to do) -> erasing.  No launch of this path
        waits for the device."""
        from .rand_augment import RandAugment
        device = next((x.device for x in imgs if x.is_cuda), torch.device("cuda", torch.cuda.current_device()))
        with torch.cuda.device(device):
            u8 = torch.empty((len(imgs), *self.size, 3), dtype=torch.uint8, device=device)
            for b, (x, p) in enumerate(zip(imgs, params)):
                x = x.to(device)
                if x.dim() == 2:                        # convert("RGB") of a grey image: three equal channels
                    x = x[:, :, None].expand(-1, -1, 3)
                ops.image_resample(x.contiguous(), self.size, crop=p["crop"], flip=p["flip"], out=u8[b])
            if self.center_crop is not None:
                ch, cw = self.center_crop
                top, left = int(round((self.size[0] - ch) / 2.0)), int(round((self.size[1] - cw) / 2.0))     # torchvision's center_crop
                u8 = u8[:, top:top + ch, left:left + cw].contiguous()
            aug = self.auto_augment if self.auto_augment is not None else RandAugment([], 0)
            decisions = aug.draw(len(imgs)) if self.auto_augment is not None else [[] for _ in imgs]
            out = aug.apply(u8, decisions, lut=self._lut_on(device))
            aug.last_params = decisions
            for p, d in zip(params, decisions):
                p["ops"] = d
            if self.random_erasing is not None:
                self.random_erasing(out)
                for b, p in enumerate(params):
                    p["erased"] = [box[1:] for box in self.random_erasing.last_boxes if box[0] == b]
        self.last_params = params
        return out


def build_transform(is_train, args, generator=None) -> Image2DTransform:
    """The reference's OCTCube/util/datasets.py build_transform (timm's create_transform for training), as one device transform.
    ``is_train`` is compared with 'train' as there; ``args`` carries input_size, aa, reprob, remode, recount, color_jitter.
      train  RandomResizedCrop(scale=(0.08, 1), bicubic) -> flip(0.5) -> RandAugment(args.aa; translate_const = int(0.45 input_size),
             img_mean = round(255 mean), bicubic) -> ToTensor -> Normalize -> RandomErasing(reprob, remode, recount) per image
      eval   Resize(int(input_size / crop_pct), bicubic) -> CenterCrop(input_size) -> ToTensor -> Normalize, crop_pct = 224 / 256 up
             to 224 and 1.0 above
    timm applies ``color_jitter`` only when ``aa`` is unset; that chain is not built here."""
    size = int(args.input_size)
    if is_train == "train":
        aa = getattr(args, "aa", None)
        if not aa and getattr(args, "color_jitter", None) is not None:
            raise NotImplementedError("color_jitter without aa: ColorJitter has no device form; set args.aa or color_jitter=None")
        if aa and not str(aa).startswith("rand"):
            raise NotImplementedError(f"auto_augment {aa!r}: only RandAugment ('rand-...') is built")
        hparams = dict(translate_const=int(size * 0.45), img_mean=tuple(min(255, round(255 * m)) for m in IMAGENET_MEAN), interpolation=3)
        return Image2DTransform((size, size), IMAGENET_MEAN, IMAGENET_STD, random_resized_crop=True, scale=(0.08, 1.0), hflip_prob=0.5,
                                generator=generator, auto_augment=aa or None, aa_hparams=hparams,
                                re_prob=float(getattr(args, "reprob", 0.0) or 0.0), re_mode=getattr(args, "remode", "const"),
                                re_count=getattr(args, "recount", 1))
    crop_pct = 224 / 256 if size <= 224 else 1.0
    full = int(size / crop_pct)
    return Image2DTransform((full, full), IMAGENET_MEAN, IMAGENET_STD, center_crop=(size, size))


def create_2d_transforms(input_size, mean=IMAGENET_MEAN, std=IMAGENET_STD, random_resized_crop=False, scale=(0.2, 1.0),
                         ratio=(3.0 / 4.0, 4.0 / 3.0), hflip_prob=0.0, generator=None) -> Image2DTransform:
    """The reference's 2-D chains as one object: ``create_2d_transforms(512)`` is the joint recipe's Resize -> ToTensor -> Normalize,
    ``create_2d_transforms(224, random_resized_crop=True, hflip_prob=0.5)`` the 2-D MAE's RandomResizedCrop -> RandomHorizontalFlip ->
    ToTensor -> Normalize.  ``generator``: the host torch.Generator the crops and flips are drawn from (None = the default one)."""
    if isinstance(input_size, int):
        input_size = (input_size, input_size)
    return Image2DTransform(input_size, mean, std, random_resized_crop, scale, ratio, hflip_prob, generator)


class DeviceTransformLoader:
    """Iterates ``loader`` and replaces element ``index`` of every batch (a list or stack of raw uint8 images) by
    ``transform.batch(...)``.  Data-loader workers cannot touch the GPU, so the dataset returns raw arrays and the transform runs here,
    in the training process; ``train_one_epoch_joint`` takes this object as its ``data_loader_2d`` unchanged."""

    def __init__(self, loader, transform, index=0):
        self.loader, self.transform, self.index = loader, transform, index

    def __len__(self):
        return len(self.loader)

    def __getattr__(self, name):            # dataset, sampler, batch_size, ...: whatever the wrapped loader offers
        if name in ("loader", "transform", "index"):
            raise AttributeError(name)
        return getattr(self.loader, name)

    def __iter__(self):
        for batch in self.loader:
            if isinstance(batch, dict):
                batch = dict(batch)
                batch[self.index] = self.transform.batch(batch[self.index])
            else:
                items = list(batch)
                items[self.index] = self.transform.batch(items[self.index])
                batch = tuple(items) if isinstance(batch, tuple) else items
            yield batch
