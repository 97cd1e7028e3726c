"""Times the fine-tune train chain of transforms.build_transform (RandomResizedCrop -> flip -> RandAugment rand-m9-mstd0.5-inc1 ->
ToTensor -> Normalize -> RandomErasing 0.25 pixel) on the GPU against the same chain on Pillow, and writes profiles/augment2d_bench.txt:

    python tools/bench_augment2d.py [--batch 64] [--iters 20] [--threads 16] [--out profiles/augment2d_bench.txt]

GPU: ``transform.batch`` over 64 raw 512 x 512 RGB images that already lie in device memory, at 224^2 and 512^2; wall time per batch
around a device synchronisation (it holds the host's decision draws and every launch), median over the iterations after a warm-up.
CPU: per image PIL crop + bicubic resize, flip, the drawn ops through ImageOps / ImageEnhance / Image.transform, ToTensor ->
Normalize and erasing in torch, on a pool of threads (Pillow releases the GIL inside its C loops); the same decisions for both.
Bytes per image are the algorithmic HBM traffic of the launches the batch made (ops' own accounting)."""
import argparse
import os
import random
import statistics
import sys
import time
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pillow_chain(x, p, size, lut, fill):
    from PIL import Image, ImageEnhance, ImageOps
    im = Image.fromarray(x)
    if p["crop"] is not None:
        t, l, h, w = p["crop"]
        im = im.crop((l, t, l + w, t + h))
    im = im.resize((size, size), Image.BICUBIC)
    if p["flip"]:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    for name, args, interp in p["ops"]:
        base = name[:-len("Increasing")] if name.endswith("Increasing") else name
        kw = dict(resample=interp, fillcolor=fill)
        W, H = im.size
        if base == "Rotate":
            im = im.rotate(args[0], **kw)
        elif base == "ShearX":
            im = im.transform(im.size, Image.AFFINE, (1, args[0], 0, 0, 1, 0), **kw)
        elif base == "ShearY":
            im = im.transform(im.size, Image.AFFINE, (1, 0, 0, args[0], 1, 0), **kw)
        elif base == "TranslateXRel":
            im = im.transform(im.size, Image.AFFINE, (1, 0, args[0] * W, 0, 1, 0), **kw)
        elif base == "TranslateYRel":
            im = im.transform(im.size, Image.AFFINE, (1, 0, 0, 0, 1, args[0] * H), **kw)
        elif base == "AutoContrast":
            im = ImageOps.autocontrast(im)
        elif base == "Equalize":
            im = ImageOps.equalize(im)
        elif base == "Invert":
            im = ImageOps.invert(im)
        elif base == "Posterize":
            im = im if args[0] >= 8 else ImageOps.posterize(im, args[0])
        elif base == "Solarize":
            im = ImageOps.solarize(im, args[0])
        elif base == "SolarizeAdd":
            im = im.point([min(255, i + args[0]) if i < 128 else i for i in range(256)] * 3)
        else:
            im = getattr(ImageEnhance, base)(im).enhance(args[0])
    t = torch.from_numpy(np.asarray(im)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    t = t.sub_(lut["mean"]).div_(lut["std"])
    for top, left, h, w in p["erased"]:
        t[:, top:top + h, left:left + w] = torch.empty((3, h, w)).normal_()
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment2d_bench.txt"))
    a = ap.parse_args()
    from octcubem_amd import ops
    from octcubem_amd.transforms import IMAGENET_MEAN, IMAGENET_STD, build_transform
    torch.set_num_threads(1)                    # the pool's threads are the parallelism of the CPU chain
    rng = np.random.Generator(np.random.PCG64(0))
    base = rng.integers(40, 200, (a.batch, 64, 64, 3), dtype=np.uint8)
    raw = np.ascontiguousarray(base.repeat(8, axis=1).repeat(8, axis=2) + rng.integers(0, 56, (a.batch, 512, 512, 3), dtype=np.uint8))
    raw_gpu = torch.from_numpy(raw).cuda()
    norm = {"mean": torch.tensor(IMAGENET_MEAN)[:, None, None], "std": torch.tensor(IMAGENET_STD)[:, None, None]}
    lines = [f"fine-tune train chain, batch {a.batch}, raw 512 x 512 x 3 uint8; {torch.cuda.get_device_name(0)}; median of {a.iters}",
             "RandomResizedCrop(0.08-1, bicubic) -> flip 0.5 -> rand-m9-mstd0.5-inc1 -> ToTensor -> Normalize -> RandomErasing(0.25, pixel)", ""]
    for size in (224, 512):
        args = types.SimpleNamespace(input_size=size, aa="rand-m9-mstd0.5-inc1", reprob=0.25, remode="pixel", recount=1, color_jitter=None)
        random.seed(0)
        np.random.seed(0)
        t = build_transform("train", args, generator=torch.Generator().manual_seed(0))
        fill = t.auto_augment.fill
        for _ in range(3):
            t.batch(raw_gpu)
        torch.cuda.synchronize()
        times, nbytes, launches = [], [], []
        for _ in range(a.iters):
            log = []
            real = ops._launch

            def counting(kind, flops, nb, fn, exec_flops=None, _real=real, _log=log):
                _log.append((kind, nb))
                return _real(kind, flops, nb, fn, exec_flops)
            ops._launch = counting
            try:
                t0 = time.perf_counter()
                t.batch(raw_gpu)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            finally:
                ops._launch = real
            nbytes.append(sum(nb for _, nb in log) / a.batch)
            launches.append(len(log))
        gpu_ms = statistics.median(times) * 1e3
        params = t.last_params                  # the last batch's decisions drive the CPU chain
        with ThreadPoolExecutor(a.threads) as pool:
            def run():
                return list(pool.map(lambda xp: pillow_chain(xp[0], xp[1], size, norm, fill), zip(raw, params)))
            run()
            cpu = []
            for _ in range(max(3, a.iters // 4)):
                t0 = time.perf_counter()
                torch.stack(run())
                cpu.append(time.perf_counter() - t0)
        cpu_ms = statistics.median(cpu) * 1e3
        lines += [f"{size}^2  device chain   {gpu_ms:8.2f} ms/batch  {a.batch / gpu_ms * 1e3:9.0f} img/s   "
                  f"{statistics.median(launches):.0f} launches, {statistics.median(nbytes) / 1e6:.2f} MB moved per image",
                  f"{size}^2  Pillow chain   {cpu_ms:8.2f} ms/batch  {a.batch / cpu_ms * 1e3:9.0f} img/s   {a.threads} CPU threads "
                  f"(without the copy of the batch to the device)",
                  f"{size}^2  ratio          {cpu_ms / gpu_ms:8.1f} x", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
