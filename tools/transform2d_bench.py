"""The 2-D image transforms three ways, in one run: the fused gfx950 launch (ops.image_resample / create_2d_transforms), the nearest
composition of ATen ops on the same GPU (F.interpolate(float32, mode="bicubic", antialias=True) + normalise -- NOT bit-equal to the
reference: it rounds once, in float, where Pillow rounds twice, in integers) and the reference's own chain, Pillow + torch on the CPU
(Image.resize(BICUBIC) -> convert("RGB") -> ToTensor -> Normalize) on --cpu-threads threads, if Pillow is importable here.

    python tools/transform2d_bench.py [--out profiles/transform2d_bench.txt]

Workloads, grey uint8, batch 64 (what one joint pre-training step consumes per GPU):
  resize512   496 x 512  -> 512 x 512     Resize -> ToTensor -> Normalize, one launch per batch
  resize1024  496 x 1024 -> 512 x 512     the same on full-width B-scans
  rrc224      496 x 512  -> 224 x 224     RandomResizedCrop(scale (0.2, 1)) -> RandomHorizontalFlip -> ToTensor -> Normalize, one launch
                                          per image (crops drawn once, before the timed windows, the same for the three paths)
--pools distinct batches are cycled through, so that no image waits in the Infinity Cache for its next use.  Per path and workload:
microseconds per batch as the median of --reps timed windows (one pass through the pools, the device synchronised once at its end) after
--warmup untimed ones, with the windows' minimum and maximum; the algorithmic bytes (crop read once, float32 [3, S, S] written once) over
that time against the HBM rates of MI355X_MICROARCH.md; images/s.  The GPU paths start from uint8 images already on the GPU and the CPU
path from uint8 arrays in host memory; the host-to-device copy of the raw images (16-32 MB per batch) is not part of any row."""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octcubem_amd import ops                                                               # noqa: E402
from octcubem_amd.transforms import (IMAGENET_MEAN, IMAGENET_STD, create_2d_transforms, normalize_lut,     # noqa: E402
                                     random_resized_crop_params)

try:
    from PIL import Image
except ImportError:
    Image = None
PIL_VERSION = getattr(Image, "__version__", "?") if Image is not None else "not importable"

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--pools", type=int, default=8)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--cpu-reps", type=int, default=3)
ap.add_argument("--cpu-threads", type=int, default=16)
ap.add_argument("--out", default=None)
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("transform2d_bench: needs an MI355X (a timing taken without one says nothing)")
dev = torch.device("cuda")
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12
torch.set_num_threads(a.cpu_threads)
WORKLOADS = {"resize512": ((496, 512), 512, False), "resize1024": ((496, 1024), 512, False), "rrc224": ((496, 512), 224, True)}
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


LUT = normalize_lut().to(dev)
MEAN_G = torch.tensor(IMAGENET_MEAN, device=dev)[None, :, None, None]
STD_G = torch.tensor(IMAGENET_STD, device=dev)[None, :, None, None]
MEAN_C, STD_C = MEAN_G[0].cpu(), STD_G[0].cpu()


def fused(x, params, S, out):
    if params is None:
        ops.image_resample(x, (S, S), lut=LUT, out=out)
    else:
        for i, p in enumerate(params):
            ops.image_resample(x[i], (S, S), crop=p[0], flip=p[1], lut=LUT, out=out[i:i + 1])


def aten(x, params, S, out):
    if params is None:
        y = F.interpolate(x[:, None].float(), size=(S, S), mode="bicubic", antialias=True, align_corners=False)
        y = y.round_().clamp_(0, 255).div_(255).expand(-1, 3, -1, -1)
        torch.div(y - MEAN_G, STD_G, out=out)
    else:
        for i, ((t, l, h, w), flip) in enumerate(params):
            y = F.interpolate(x[i, t:t + h, l:l + w][None, None].float(), size=(S, S), mode="bicubic", antialias=True, align_corners=False)
            y = y.round_().clamp_(0, 255).div_(255).expand(-1, 3, -1, -1)
            if flip:
                y = y.flip(3)
            torch.div(y - MEAN_G, STD_G, out=out[i:i + 1])


def pillow_one(arr, p, S):
    im = Image.fromarray(arr)
    if p is not None:
        t, l, h, w = p[0]
        im = im.crop((l, t, l + w, t + h))
    im = im.resize((S, S), Image.BICUBIC)
    if p is not None and p[1]:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    x = torch.from_numpy(np.array(im.convert("RGB"))).permute(2, 0, 1).contiguous().to(torch.float32).div(255)     # ToTensor
    return x.sub_(MEAN_C).div_(STD_C)                                                                              # Normalize


def pillow(x, params, S, out, pool):
    res = list(pool.map(lambda i: pillow_one(x[i], None if params is None else params[i], S), range(len(x))))
    torch.stack(res, out=out)


def windows(run, n_batches, reps, warmup, gpu=True):
    ts = []
    for r in range(warmup + reps):
        if gpu:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        if gpu:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / n_batches)
    ts = ts[warmup:]
    return statistics.median(ts), min(ts), max(ts)


say(f"# transform2d_bench: batch {a.batch}, {a.pools} distinct batches cycled, {a.reps} timed windows after {a.warmup} warm-up, "
    f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}, Pillow {PIL_VERSION}")
say(f"# the cpu rows are a far smaller sample: {a.cpu_reps} timed windows after 1 warm-up of one batch each, {a.cpu_threads} threads "
    f"({os.cpu_count()} on the host); their spread is not comparable to the GPU rows'")
say("# us/batch = median over the windows [min .. max]; bytes = uint8 crop read + float32 [3, S, S] written; "
    f"HBM: {HBM_SPEC / 1e12:.1f} TB/s specified, {HBM_COPY / 1e12:.2f} TB/s float4 copy")
hdr = f"{'workload':12s}{'path':14s}{'us/batch':>12s}{'[min':>12s}{'max]':>12s}{'GB/s':>9s}{'%copy':>7s}{'img/s':>11s}"
results = {}
gen = torch.Generator().manual_seed(0)
for wname, ((H, W), S, rrc) in WORKLOADS.items():
    g = torch.Generator().manual_seed(1)
    host = [torch.randint(0, 256, (a.batch, H, W), dtype=torch.uint8, generator=g) for _ in range(a.pools)]
    pools = [x.to(dev) for x in host]
    params = None
    if rrc:
        params = [[(random_resized_crop_params(H, W, generator=gen), bool(torch.rand(1, generator=gen) < 0.5)) for _ in range(a.batch)]
                  for _ in range(a.pools)]
    out = torch.empty((a.batch, 3, S, S), device=dev)
    out2 = torch.empty_like(out)
    par = (lambda k: None) if params is None else (lambda k: params[k])
    # before anything is timed: what the paths compute.  fused against Pillow must be 0 differing values; ATen is another function.
    fused(pools[0], par(0), S, out)
    aten(pools[0], par(0), S, out2)
    ne = (out != out2)
    say()
    say(f"# {wname}: {H} x {W} -> {S} x {S}{', crops and flips drawn per image' if rrc else ''}; fused vs ATen: "
        f"{100 * float(ne.float().mean()):.2f} % of the values differ, max |diff| {float((out - out2).abs().max()):.4f} "
        f"(one grey level = {1 / 255 / IMAGENET_STD[0]:.4f})")
    if Image is not None:
        ref = torch.stack([pillow_one(host[0][i].numpy(), None if params is None else params[0][i], S) for i in range(4)])
        say(f"# {wname}: fused vs Pillow + torch on 4 images: {int((out[:4].cpu() != ref).sum())} differing values")
    nbytes = sum(p[0][2] * p[0][3] for p in params[0]) if rrc else a.batch * H * W
    nbytes += 4 * out.numel()
    say(hdr)
    run_f = lambda: [fused(pools[k], par(k), S, out) for k in range(a.pools)]       # noqa: E731
    run_a = lambda: [aten(pools[k], par(k), S, out2) for k in range(a.pools)]       # noqa: E731
    # the two GPU paths alternate, fused first and last: a drift of the clocks shows as a difference between the two fused rows
    rows = [("fused", run_f, a.pools, a.reps, a.warmup, True), ("aten-gpu", run_a, a.pools, a.reps, a.warmup, True),
            ("fused(2nd)", run_f, a.pools, a.reps, a.warmup, True)]
    if Image is not None:
        tp = ThreadPoolExecutor(a.cpu_threads)
        host_np = host[0].numpy()
        out_c = torch.empty((a.batch, 3, S, S))
        rows.append((f"pillow-{a.cpu_threads}thr", lambda: pillow(host_np, par(0), S, out_c, tp), 1, a.cpu_reps, 1, False))
    for path, run, nb, reps, warm, gpu in rows:
        med, lo, hi = windows(run, nb, reps, warm, gpu)
        results[(wname, path)] = med
        say(f"{wname:12s}{path:14s}{med * 1e6:12.1f}{lo * 1e6:12.1f}{hi * 1e6:12.1f}{nbytes / med / 1e9:9.1f}"
            f"{100 * nbytes / med / HBM_COPY:7.2f}{a.batch / med:11.0f}")
    if not rrc:      # the public interface on top of the raw op, from a list of host arrays: adds the stack and the host-to-device copy
        t = create_2d_transforms(S)
        imgs = [host[0][i].numpy() for i in range(a.batch)]
        med, lo, hi = windows(lambda: t.batch(imgs), 1, a.reps, a.warmup, True)
        say(f"# create_2d_transforms({S}).batch(list of {a.batch} host arrays), copy included: {med * 1e6:.1f} us/batch [{lo * 1e6:.1f} .. {hi * 1e6:.1f}]")
    del pools, out, out2

say()
say("# ratios of medians (> 1: the fused launch is faster); fused = the slower of its two rows")
notes = []
for wname in WORKLOADS:
    f = max(results[(wname, "fused")], results[(wname, "fused(2nd)")])
    s = f"{wname:12s} ATen / fused = {results[(wname, 'aten-gpu')] / f:7.2f}"
    cpu = [v for (w, p), v in results.items() if w == wname and p.startswith("pillow")]
    if cpu:
        s += f"    Pillow-{a.cpu_threads}thr / fused = {cpu[0] / f:8.1f}"
    say(s)
    if min([results[(wname, 'aten-gpu')]] + cpu) < f:
        notes.append(wname)
say("# the fused launch is " + ("NOT the fastest path at: " + ", ".join(notes) if notes else "the fastest of the measured paths in every workload"))

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
