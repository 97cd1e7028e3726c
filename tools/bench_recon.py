#!/usr/bin/env python3
"""Times the reconstruction volumes of the validation pass at the headline shape (batch 32 of 60 x 256 x 256, L = 5120, PD = 768):

  fused   ops.mae_compose (csrc/recon.hip, one kernel), on the strided ``pred_full[:, 1:, :]`` view the decoder leaves behind
  aten    the same chain composed from ATen ops on the GPU: tests/recon_ref.panels moved to the device (unpatchify of pred and of the
          mask expanded to pixels, untransform_image of both, the two blends; with --denorm the per-patch mean / variance first)
  cpu     the chain as the reference runs it: pred, mask and the frames copied to the host, then the same torch ops on 16 CPU threads

HIP events around each call on the launch stream, every shape warmed up first, fused and aten alternated inside one loop so that both
see the same machine; the median and the spread (min .. max) of the repeats are reported.  The byte count is the algorithm's, computed
here from the shapes: pred + gathered frames + mask read, 4 x uint8 written; with denorm the target patch is read twice.  The fused
result is compared with the aten result at the timed size before anything is timed (equal without denorm; within one grey level with).

    python tools/bench_recon.py [--batch 32] [--reps 20] [--out profiles/recon_bench.txt]
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
from tests import recon_ref as R  # noqa: E402


def aten_chain(pred, imgs, mask, fi, u, p, denorm):
    if denorm:
        Tp = R.pred_frames(pred, imgs, u, p)
        target = R.patchify(R.select_frames(imgs, fi, Tp), p, u)
        pred = pred * (target.var(dim=-1, keepdim=True) + 1.0e-6) ** 0.5 + target.mean(dim=-1, keepdim=True)
    return R.panels(pred, imgs, mask, fi, u, p).to(torch.uint8)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, T, H, W, p, u = a.batch, 60, 256, 256, 16, 3
    L, PD = (T // u) * (H // p) * (W // p), u * p * p
    g = torch.Generator().manual_seed(0)
    imgs = (torch.rand(B, 1, T, H, W, generator=g) * 3.6 - 0.7).to(dev)
    pred_full = (torch.rand(B, 1 + L, PD, generator=g) * 3.6 - 0.7).to(dev)
    pred = pred_full[:, 1:, :]
    mask = (torch.rand(B, L, generator=g) < 0.75).float().to(dev)
    nvox = B * T * H * W
    lines = [f"reconstruction volumes, batch {B} of {T} x {H} x {W}, L = {L}, PD = {PD}; {torch.cuda.get_device_name(0)}; "
             f"{a.reps} alternated repeats, HIP events, ms: median (min .. max)"]
    for denorm in (False, True):
        nbytes = 4 * B * L * PD + 4 * nvox * (2 if denorm else 1) + 4 * B * L + 4 * nvox
        fused = lambda: ops.mae_compose(pred, imgs, mask, None, u, p, denorm)       # noqa: E731
        aten = lambda: aten_chain(pred, imgs, mask, None, u, p, denorm)             # noqa: E731
        a_out, f_out = aten(), fused()                                              # warm-up of both, and the comparison
        diff = (a_out.int() - f_out.int()).abs()
        if denorm:
            assert int(diff.max()) <= 1, int(diff.max())
        else:
            assert int(diff.max()) == 0
        ndiff = int((diff != 0).sum())
        del a_out, f_out, diff
        for _ in range(2):
            fused(); aten()
        torch.cuda.synchronize()
        tf, ta = [], []
        for _ in range(a.reps):
            tf += timed(fused, 1); ta += timed(aten, 1)
        torch.set_num_threads(16)
        tc = []
        for _ in range(a.cpu_reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            aten_chain(pred.cpu(), imgs.cpu(), mask.cpu(), None, u, p, denorm)
            tc.append(1e3 * (time.perf_counter() - t0))
        tc = tc[1:]
        mf, ma, mc = statistics.median(tf), statistics.median(ta), statistics.median(tc)
        lines += [f"denorm = {int(denorm)}   algorithmic traffic {nbytes / 1e6:.1f} MB   voxels that differ from the ATen chain: {ndiff} of {4 * nvox}",
                  f"  fused HIP kernel      {mf:9.3f} ({min(tf):.3f} .. {max(tf):.3f})   {nbytes / mf / 1e9:7.3f} TB/s algorithmic",
                  f"  ATen ops on the GPU   {ma:9.3f} ({min(ta):.3f} .. {max(ta):.3f})   {nbytes / ma / 1e9:7.3f} TB/s algorithmic   x {ma / mf:.1f}",
                  f"  torch, 16 CPU threads {mc:9.1f} ({min(tc):.1f} .. {max(tc):.1f})   incl. device -> host copies              x {mc / mf:.0f}"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
