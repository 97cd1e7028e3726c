"""Mixup / cutmix of a fine-tune batch two ways on the same GPU, in one run: the fused in-place launch (ops.mix_batch, csrc/mixup.hip)
and timm's op sequence composed from ATen ops -- batch mode: ``x.flip(0).mul_(1 - lam)``, ``x.mul_(lam).add_(...)`` for mixup and the
sliced assignment from ``x.flip(0)`` for cutmix; elem mode: ``x.clone()`` and the per-sample Python loop.

    python tools/bench_mixup.py [--out profiles/mixup_bench.txt]

Shapes [32, 1, 60, 256, 256] (volumes) and [64, 3, 512, 512] (images), float32, seeded; mixup (lam 0.3) and cutmix (the box of lam 0.5
around the centre: sides H / sqrt(2), W / sqrt(2)) in batch mode, and in elem mode with per-sample lams / boxes, every other sample
cutting.  The two paths must be bit-equal on the first call before anything is timed.  Per case: milliseconds per call from device
events around the call, the median of --reps calls after --warmup untimed ones, with minimum and maximum; the two paths alternate
call by call.  The fused path's time includes the upload of its tables.  GB/s = the bytes the fused launch has to move (ops.mix_bytes:
derived from the shapes, not measured) over the median.  For 5-D input the ATen cutmix cuts the same (H, W) box as the kernel."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from octcubem_amd import ops      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--shapes", default="32,1,60,256,256;64,3,512,512")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixup_bench.txt"))
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_mixup: needs an MI355X (a timing taken without one says nothing)")
dev = torch.device("cuda")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def aten_batch(x, kind, lam, box):
    if kind == 1:
        x_flipped = x.flip(0).mul_(1.0 - lam)
        x.mul_(lam).add_(x_flipped)
    else:
        yl, yh, xl, xh = box
        x[..., yl:yh, xl:xh] = x.flip(0)[..., yl:yh, xl:xh]


def aten_elem(x, kinds, lams, boxes):
    B = len(x)
    x_orig = x.clone()
    for i in range(B):
        j = B - i - 1
        if kinds[i] == 2:
            yl, yh, xl, xh = boxes[i]
            x[i][..., yl:yh, xl:xh] = x_orig[j][..., yl:yh, xl:xh]
        elif kinds[i] == 1:
            x[i] = x[i] * lams[i] + x_orig[j] * (1 - lams[i])


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def compare(name, x0, fused, aten, nbytes):
    xa, xb = x0.clone(), x0.clone()
    fused(xa)
    aten(xb)
    same = torch.equal(xa, xb)
    assert same, f"{name}: the fused launch and the ATen composition differ"
    for _ in range(a.warmup):
        fused(xa); aten(xb)
    tf, ta = [], []
    for _ in range(a.reps):
        tf.append(event_ms(lambda: fused(xa)))
        ta.append(event_ms(lambda: aten(xb)))
    mf, ma = statistics.median(tf), statistics.median(ta)
    say(f"  {name:<22} fused {mf:8.3f} [{min(tf):.3f} .. {max(tf):.3f}]  {nbytes / (mf * 1e-3) / 1e9:7.0f} GB/s ({nbytes / 1e6:.0f} MB)"
        f"   ATen {ma:8.3f} [{min(ta):.3f} .. {max(ta):.3f}]   ATen / fused {ma / mf:5.2f}")
    del xa, xb


say(f"# tools/bench_mixup.py  {torch.cuda.get_device_name(0)}  torch {torch.__version__}  reps {a.reps} warm-up {a.warmup}")
say("# ms per call (device events): median [min .. max]; bit-equal results checked before timing")
for spec in a.shapes.split(";"):
    shape = tuple(int(v) for v in spec.split(","))
    B, H, W = shape[0], shape[-2], shape[-1]
    S = int(np.prod(shape[1:]))
    x0 = torch.randn(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    say(f"{list(shape)}  ({x0.numel() * 4 / 1e6:.0f} MB)")
    ch, cw = int(H * np.sqrt(0.5)), int(W * np.sqrt(0.5))
    cbox = (H // 2 - ch // 2, H // 2 + ch // 2, W // 2 - cw // 2, W // 2 + cw // 2)
    zero = np.zeros((B, 4), dtype=np.int32)
    # batch mode
    lam = 0.3
    k1, l1, o1 = np.full(B, 1, np.int32), np.full(B, np.float32(lam)), np.full(B, np.float32(1.0 - lam))
    compare("batch mixup", x0, lambda x: ops.mix_batch(x, k1, l1, o1, zero, H, W), lambda x: aten_batch(x, 1, lam, None),
            ops.mix_bytes(k1, zero, S, H, W))
    k2, b2 = np.full(B, 2, np.int32), np.tile(np.array(cbox, dtype=np.int32), (B, 1))
    compare("batch cutmix", x0, lambda x: ops.mix_batch(x, k2, l1, o1, b2, H, W), lambda x: aten_batch(x, 2, lam, cbox),
            ops.mix_bytes(k2, b2, S, H, W))
    # elem mode: per-sample decisions, every other sample cuts
    rs = np.random.RandomState(1)
    lams = rs.beta(0.8, 0.8, size=B).astype(np.float32)
    ke = np.where(np.arange(B) % 2 == 0, 1, 2).astype(np.int32)
    be = np.zeros((B, 4), dtype=np.int32)
    for i in range(B):
        if ke[i] == 2:
            hh, ww = int(H * np.sqrt(1 - lams[i])), int(W * np.sqrt(1 - lams[i]))
            cy, cx = rs.randint(0, H), rs.randint(0, W)
            be[i] = (np.clip(cy - hh // 2, 0, H), np.clip(cy + hh // 2, 0, H), np.clip(cx - ww // 2, 0, W), np.clip(cx + ww // 2, 0, W))
    oe = np.float32(1) - lams
    for label, kinds in (("elem mixup", np.ones(B, np.int32)), ("elem cutmix", np.full(B, 2, np.int32)),
                         ("elem mixup + cutmix", ke)):
        bx = be.copy()
        if label == "elem cutmix":                                   # every sample cuts: give the mixing ones a box as well
            for i in range(B):
                if ke[i] != 2:
                    bx[i] = be[(i + 1) % B]
        bl = [tuple(int(v) for v in b) for b in bx]
        compare(label, x0, lambda x, kinds=kinds, bx=bx: ops.mix_batch(x, kinds, lams, oe, bx, H, W),
                lambda x, kinds=kinds, bl=bl: aten_elem(x, kinds, lams, bl), ops.mix_bytes(kinds, bx, S, H, W))
    del x0
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
