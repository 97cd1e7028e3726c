#!/usr/bin/env python3
"""Times the saliency passes on ViT-L at 60 x 256 x 256, batch 4 (5121 tokens x 1024 channels per sample):

  input_gradient / grad_cam             octcubem_amd.saliency, the backward under ops.weight_grads(False)
  the same passes, weight_grads on      the identical code path with ops.weight_grads(True) nested inside it: the weight-gradient
                                        GEMMs, bias column sums and LayerNorm parameter gradients of the blocks the backward walks
                                        run too (into the gradient arena, which is zeroed afterwards, outside the timed window).
                                        grad_cam's backward stops at the chosen block in both forms
  Grad-CAM reduction / heat volume      --inner calls inside one event pair, so that a window holds milliseconds of work.  A and G
                                        (168 MB at batch 4) fit the MI355X's 256 MB last-level cache and the same pair is read again
                                        and again: these figures are CACHE-WARM, not HBM rates
  Grad-CAM reduction, fused / ATen      ops.cam_weights + ops.cam_tokens against relu((G[:, 1:].mean(1, keepdim=True) * A[:, 1:]).sum(-1))
  heat volume, fused / ATen             ops.heatmap against normalise -> F.interpolate(trilinear) -> floor -> uint8
  eigen-smoothed map / plain reduction  ops.cam_eigen at 32 iterations against ops.cam_tokens, both behind ops.cam_weights, on the model's
                                        streams (4 x 5121 x 1024) and at the en-face size (4 x 257 x 1024); cache-warm as above
  aug_smooth                            grad_cam(aug_smooth=True): six passes and six folds, against one plain grad_cam

HIP events around each call on the launch stream, everything warmed up first, the two forms of a pair alternated inside one loop so that
both see the same machine; the median and the spread (min .. max) of the repeats are reported.  Until this has run on an MI355X no time
and no ratio is claimed anywhere.

    python tools/bench_saliency.py [--batch 4] [--reps 10] [--out profiles/saliency_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from octcubem_amd import models_vit_st, ops, saliency  # noqa: E402


def timed(fn, inner=1):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner


def fmt(ts):
    return f"{statistics.median(ts):9.3f} ({min(ts):.3f} .. {max(ts):.3f})"


_REAL_SWITCH = ops.weight_grads


class _SwitchOn:
    """ops.weight_grads stand-in that leaves the switch on: saliency's own code path, weight gradients and all"""

    def __init__(self, enabled):
        self.inner = _REAL_SWITCH(True)

    def __enter__(self):
        return self.inner.__enter__()

    def __exit__(self, *exc):
        return self.inner.__exit__(*exc)


def with_weight_grads(fn):
    """the same saliency call with ops.weight_grads(True) nested inside it"""
    def run():
        real, ops.weight_grads = ops.weight_grads, _SwitchOn
        try:
            return fn()
        finally:
            ops.weight_grads = real
    return run


def aten_cam(A, G):
    return torch.relu((G[:, 1:].mean(dim=1, keepdim=True) * A[:, 1:]).sum(-1))


def aten_heat(m, size):
    B = m.shape[0]
    mn = m.reshape(B, -1).min(1).values.view(B, 1, 1, 1)
    mx = m.reshape(B, -1).max(1).values.view(B, 1, 1, 1)
    v = (m - mn) / (1e-7 + (mx - mn))
    v = F.interpolate(v[:, None], size=size, mode="trilinear", align_corners=False)[:, 0]
    return (255.0 * v).floor().to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=50, help="calls of a reduction / heat-volume form inside one event pair")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, T, H, W = a.batch, 60, 256, 256
    torch.manual_seed(0)
    model = models_vit_st.vit_large_patch16(num_frames=T, t_patch_size=3, img_size=H, in_chans=1, num_classes=8, sep_pos_embed=True,
                                            cls_embed=True, global_pool=True, dropout=0.0).to(dev)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 1, T, H, W, generator=g).to(dev)
    tgt = torch.randint(0, 8, (B,), generator=g).to(dev)
    lines = [f"saliency passes, ViT-L, batch {B} of {T} x {H} x {W}; {torch.cuda.get_device_name(0)}; operands {ops.BF16}; {a.reps} alternated "
             "repeats, HIP events, ms: median (min .. max)"]
    passes = [("input_gradient", lambda: saliency.input_gradient(model, x, tgt)), ("grad_cam      ", lambda: saliency.grad_cam(model, x, tgt))]
    for name, off in passes:
        on = with_weight_grads(off)
        off(); on()
        model.arena.zero_grad()
        torch.cuda.synchronize()
        t_off, t_on = [], []
        for _ in range(a.reps):
            t_off.append(timed(off)); t_on.append(timed(on))
            model.arena.zero_grad()                                  # what the switched-on pass left in the arena; not timed
            torch.cuda.synchronize()
        lines += [f"{name}  weight_grads(False) {fmt(t_off)}   weight gradients on {fmt(t_on)}   x {statistics.median(t_on) / statistics.median(t_off):.2f}"]
    r = saliency.grad_cam(model, x, tgt, return_streams=True)
    A, G, cam = r["activations"], r["gradients"], r["cam"]
    nb = 2 * 4 * A.numel()
    ref = aten_cam(A, G)
    err = float((cam.reshape(B, -1) - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
    fused = lambda: ops.cam_tokens(A, ops.cam_weights(G, 1), 1)      # noqa: E731
    aten = lambda: aten_cam(A, G)                                    # noqa: E731
    for _ in range(2):
        fused(); aten()
    torch.cuda.synchronize()
    tf, ta = [], []
    for _ in range(a.reps):
        tf.append(timed(fused, a.inner)); ta.append(timed(aten, a.inner))
    lines += [f"Grad-CAM reduction over A, G f32 {tuple(A.shape)}: {nb / 1e6:.1f} MB read, cache-warm ({a.inner} calls per event pair on the same buffers, which fit the last-level cache); max |fused - ATen| / max |ATen| = {err:.1e}",
              f"  fused HIP kernels     {fmt(tf)}   {nb / statistics.median(tf) / 1e9:7.3f} TB/s algorithmic, cache-warm",
              f"  ATen ops on the GPU   {fmt(ta)}   {nb / statistics.median(ta) / 1e9:7.3f} TB/s algorithmic, cache-warm   x {statistics.median(ta) / statistics.median(tf):.1f}"]
    # the eigen-smoothed map (32 power iterations: 103 launches) against the plain reduction (3 launches), on the model's own streams and
    # on random streams of the en-face size; both forms include ops.cam_weights.  Cache-warm as above: A alone is read 66 times per call
    g2 = torch.Generator().manual_seed(2)
    enface = (torch.randn(B, 257, 1024, generator=g2).to(dev), torch.randn(B, 257, 1024, generator=g2).to(dev))
    for label, Ae, Ge, inner in (("ViT-L volume", A, G, max(1, a.inner // 10)), ("en-face image", *enface, a.inner)):
        plain = lambda: ops.cam_tokens(Ae, ops.cam_weights(Ge, 1), 1)                 # noqa: E731
        eigen = lambda: ops.cam_eigen(Ae, ops.cam_weights(Ge, 1), 1, 32)              # noqa: E731
        for _ in range(2):
            plain(); eigen()
        residual = eigen()[1]
        torch.cuda.synchronize()
        tp, te = [], []
        for _ in range(a.reps):
            tp.append(timed(plain, inner)); te.append(timed(eigen, inner))
        lines += [f"eigen-smoothed map, {label}, A, G f32 {tuple(Ae.shape)}, 32 iterations, cache-warm ({inner} calls per event pair on the same "
                  f"buffers); residual after 32 iterations: max {float(residual.max()):.1e}",
                  f"  plain reduction       {fmt(tp)}",
                  f"  ops.cam_eigen         {fmt(te)}   x {statistics.median(te) / statistics.median(tp):.1f}   "
                  f"{statistics.median(te) * 1e3 / 103:.1f} us per launch"]
    # augmentation smoothing: six forward + backward passes and six folds against one plain pass
    one = lambda: saliency.grad_cam(model, x, tgt)                                     # noqa: E731
    six = lambda: saliency.grad_cam(model, x, tgt, aug_smooth=True)                    # noqa: E731
    one(); six()
    torch.cuda.synchronize()
    t1, t6 = [], []
    for _ in range(a.reps):
        t1.append(timed(one)); t6.append(timed(six))
    lines += [f"grad_cam, aug_smooth (six passes)   plain {fmt(t1)}   aug_smooth {fmt(t6)}   x {statistics.median(t6) / statistics.median(t1):.2f}"]
    size = (T, H, W)
    hv, hr = ops.heatmap(cam, size), aten_heat(cam, size)
    d = (hv.int() - hr.int()).abs()
    nb = 4 * cam.numel() + hv.numel()
    fused = lambda: ops.heatmap(cam, size)                           # noqa: E731
    aten = lambda: aten_heat(cam, size)                              # noqa: E731
    for _ in range(2):
        fused(); aten()
    torch.cuda.synchronize()
    tf, ta = [], []
    for _ in range(a.reps):
        tf.append(timed(fused, a.inner)); ta.append(timed(aten, a.inner))
    lines += [f"heat volume {tuple(cam.shape)} -> uint8 {tuple(hv.shape)}: {nb / 1e6:.1f} MB algorithmic; bytes that differ from the ATen chain: "
              f"{int((d != 0).sum())} of {d.numel()} (max {int(d.max())})",
              f"  fused HIP kernels     {fmt(tf)}   {nb / statistics.median(tf) / 1e9:7.3f} TB/s algorithmic, cache-warm",
              f"  ATen ops on the GPU   {fmt(ta)}   {nb / statistics.median(ta) / 1e9:7.3f} TB/s algorithmic, cache-warm   x {statistics.median(ta) / statistics.median(tf):.1f}"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
