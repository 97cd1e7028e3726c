#!/usr/bin/env python3
"""Times the 2-D half of the validation pass at the joint recipe's shape (one batch of 64 B-scan triplets of 3 x 512 x 512):

  blanking   ops.white_border (csrc/recon2d.hip, two launches)  against
             aten   the same result composed from ATen ops on the GPU (per-image extremes, first / last white column by argmax, the two
                    runs and their extensions as column masks; about 40 launches)
             cpu    the reference's row-and-column loop restated in Python on the CPU (find_and_convert_large_white_region is such a
                    loop), timed on --cpu-images images and reported per image
  panels     ops.mae_compose_nc for 64 x 3 x 512 x 512 (C = 3, u = 1: the 2-D MAE) and for 64 x 1 x 3 x 512 x 512 (C = 1, u = 3: the
             joint model's triplets), p = 16, on the strided ``pred_full[:, 1:, :]`` view, against tests/recon2d_ref.panels_nc on the GPU

HIP events around each call on the launch stream, every shape warmed up first, the fused and the ATen form alternated inside one loop
so that both see the same machine; the median and the spread (min .. max) of the repeats are reported.  The blanking works in place, so
every repeat (of both forms) starts from a fresh copy made outside the timed window.  The byte counts are the algorithm's, computed
here from the shapes.  The fused results are compared with the ATen results at the timed size before anything is timed (all equal).

    python tools/bench_recon2d.py [--batch 64] [--reps 20] [--out profiles/recon2d_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from octcubem_amd import ops  # noqa: E402
from tests import recon2d_ref as R  # noqa: E402


def aten_blank(x):
    """x [B, T, H, W] on the GPU -> (blanked copy, region bool), the semantics of octmae_white_border in whole-tensor ops"""
    B, T, H, W = x.shape
    lim = ops.white_border_limits(W)
    mx, mn = x.amax(dim=(1, 2, 3)), x.amin(dim=(1, 2, 3))                 # amax / amin propagate a NaN, as torch.max does
    thresh = mx - (255 - 240) / 255 * (mx - mn)
    g = x[:, 0]
    white = g > thresh.view(B, 1, 1)
    col = torch.arange(W, device=x.device).view(1, 1, W)
    anyw = white.any(-1)
    f = torch.where(anyw, white.int().argmax(-1), W)
    l = torch.where(anyw, W - 1 - white.flip(-1).int().argmax(-1), -1)
    after = ~white & (col >= f.unsqueeze(-1))
    e = torch.where(after.any(-1), after.int().argmax(-1), W)
    before = ~white & (col <= l.unsqueeze(-1))
    s = torch.where(before.any(-1), W - 1 - before.flip(-1).int().argmax(-1), -1)
    left, right = anyw & (f < lim[0]), anyw & (l >= lim[2])
    e2 = torch.where(left & (e < W) & (e >= lim[1]), (e + 5).clamp(max=W), e)
    rext = right & (s >= 0) & (s < lim[3]) & (s <= 4)
    u = lambda t: t.unsqueeze(-1)       # noqa: E731
    region = (u(left) & (col >= u(f)) & (col < u(e2))) | (u(right) & (col > u(s)) & (col <= u(l))) | \
             (u(rext) & (col >= u(s)) & (col < u(W + s - 5)))
    g = torch.where(region, torch.zeros((), device=x.device), g)
    return g.unsqueeze(1).repeat(1, T, 1, 1), region.unsqueeze(1).repeat(1, T, 1, 1)


def loop_blank(image):
    """The row-and-column loop on the CPU: every row walked pixel by pixel from its first and from its last white column."""
    import numpy as np
    thresh = R.threshold(image)
    g = image[0].clone()
    white = (g > thresh).numpy()
    H, W = white.shape
    region = np.zeros((H, W), dtype=bool)
    for y in range(H):
        row = white[y]
        if not row.any():
            continue
        f = int(row.argmax())
        if not (f > 0.01 * W):
            for c in range(f, W):
                if not row[c]:
                    if c > 0.05 * W:
                        region[y, c:c + 5] = True
                    break
                region[y, c] = True
        l = W - 1 - int(row[::-1].argmax())
        if not (l < W - 0.01 * W):
            for c in range(l, -1, -1):
                if not row[c]:
                    if c < W - 0.05 * W:
                        region[y, c:c - 5] = True
                    break
                region[y, c] = True
    g[torch.from_numpy(region)] = 0
    return g.unsqueeze(0).repeat(image.shape[0], 1, 1), torch.from_numpy(region)


def timed(fn, before=None):
    if before is not None:
        before()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(); fn(); e.record()
    e.synchronize()
    return s.elapsed_time(e)


def fmt(ts):
    return f"{statistics.median(ts):9.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def triplets(B, H, W, g):
    """B-scan-like triplets: dim speckle, a bright band of varying width at the left edge of about half the rows of every image and at
    the right edge of a quarter of them"""
    x = torch.rand(B, 3, H, W, generator=g) * 0.6
    wl = torch.randint(0, W // 8, (B, H), generator=g) * (torch.rand(B, H, generator=g) < 0.5)
    wr = torch.randint(0, W // 8, (B, H), generator=g) * (torch.rand(B, H, generator=g) < 0.25)
    col = torch.arange(W).view(1, 1, W)
    x[:, 0][(col < wl.unsqueeze(-1)) | (col >= W - wr.unsqueeze(-1))] = 1.0
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-images", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_recon2d needs an MI355X: a timing taken elsewhere says nothing about it"
    dev = torch.device("cuda", 0)
    B, H, W, p = a.batch, a.size, a.size, 16
    g = torch.Generator().manual_seed(0)
    lines = [f"2-D validation half, batch {B} of 3 x {H} x {W}; {torch.cuda.get_device_name(0)}; {a.reps} alternated repeats, HIP events, "
             "ms: median (min .. max)"]
    # ---- blanking
    src = triplets(B, H, W, g)
    src_d = src.to(dev)
    work = torch.empty_like(src_d)
    fresh = lambda: work.copy_(src_d)                                        # noqa: E731
    fresh()
    want_img, want_reg = aten_blank(work)
    got_img, got_reg = ops.white_border(work)
    got_img = got_img.clone()                                                 # ``work`` itself is refilled before every repeat
    assert torch.equal(got_img, want_img) and torch.equal(got_reg, want_reg), "the fused blanking differs from the ATen chain"
    marked = float(got_reg[:, 0].float().mean())
    for _ in range(2):
        fresh(); ops.white_border(work); fresh(); aten_blank(work)
    torch.cuda.synchronize()
    tf, ta = [], []
    for _ in range(a.reps):
        tf.append(timed(lambda: ops.white_border(work), fresh))
        ta.append(timed(lambda: aten_blank(work), fresh))
    tc = []
    for i in range(a.cpu_images):
        t0 = time.perf_counter()
        img, reg = loop_blank(src[i])
        tc.append(1e3 * (time.perf_counter() - t0))
        assert torch.equal(img, got_img[i].cpu()) and torch.equal(reg, got_reg[i, 0].cpu())
    npx = B * 3 * H * W
    nbytes = 4 * npx + 4 * npx + npx                                          # every frame read once, every frame and every mark written
    mf, ma = statistics.median(tf), statistics.median(ta)
    lines += [f"blanking: {100 * marked:.1f} % of frame 0 marked; algorithmic traffic {nbytes / 1e6:.1f} MB = {nbytes / npx:.0f} bytes per pixel "
              "(4 read, 4 + 1 written; frame 0 is read three times more, from cache)",
              f"  fused HIP, 2 launches  {fmt(tf)}   {nbytes / mf / 1e9:7.3f} TB/s algorithmic",
              f"  ATen ops on the GPU    {fmt(ta)}   {nbytes / ma / 1e9:7.3f} TB/s algorithmic   x {ma / mf:.1f}",
              f"  Python loop on the CPU {statistics.median(tc):9.1f} per image ({min(tc):.1f} .. {max(tc):.1f}, {a.cpu_images} images), "
              f"{B * statistics.median(tc):.0f} for the batch; results equal"]
    del work, want_img, want_reg, got_img, got_reg
    # ---- panels
    for C, u, what in ((3, 1, "C = 3, u = 1 (the 2-D MAE)"), (1, 3, "C = 1, u = 3 (the joint model's triplets)")):
        T = 3 if C == 1 else 1
        L, PD = (H // p) * (W // p), u * p * p * C
        imgs = (torch.rand(B, C, T, H, W, generator=g) * 1.4 - 0.2).to(dev)
        pred = (torch.rand(B, 1 + L, PD, generator=g) * 1.4 - 0.2).to(dev)[:, 1:, :]
        mask = (torch.rand(B, L, generator=g) < 0.75).float().to(dev)
        fused = lambda: ops.mae_compose_nc(pred, imgs, mask, u, p)            # noqa: E731
        aten = lambda: R.panels_nc(pred, imgs, mask, u, p).to(torch.uint8)    # noqa: E731
        assert torch.equal(fused(), aten()), "the fused panels differ from the ATen chain"
        for _ in range(2):
            fused(); aten()
        torch.cuda.synchronize()
        tf, ta = [], []
        for _ in range(a.reps):
            tf.append(timed(fused)); ta.append(timed(aten))
        nel = B * C * T * H * W
        nbytes = 4 * B * L * PD + 4 * nel + 4 * B * L + 4 * nel               # pred, image and mask read, four uint8 panels written
        mf, ma = statistics.median(tf), statistics.median(ta)
        lines += [f"panels, {what}: algorithmic traffic {nbytes / 1e6:.1f} MB = {nbytes / nel:.1f} bytes per pixel and channel "
                  "(4 + 4 read, 4 x 1 written); all bytes equal",
                  f"  fused HIP kernel       {fmt(tf)}   {nbytes / mf / 1e9:7.3f} TB/s algorithmic",
                  f"  ATen ops on the GPU    {fmt(ta)}   {nbytes / ma / 1e9:7.3f} TB/s algorithmic   x {ma / mf:.1f}"]
        del imgs, pred, mask
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
