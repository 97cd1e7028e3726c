#!/usr/bin/env python3
"""Times attention rollout (octcubem_amd.saliency.attention_rollout, csrc/rollout.hip) against the same quantity from ATen ops:

  one step        ops.rollout_step on widened f32 q, k of one block (mean and max fusion), against an ATen step that materialises
                  softmax(scale q k^T) for all heads in row chunks of at most 1 GiB, fuses the heads, and multiplies the weighted rows
                  into the columns (the chunked form is what fits beside a ViT-L at all: the whole [H, N, N] is 1.7 GB per volume)
  the whole call  attention_rollout(model, x): one forward under capture_attention, then depth steps; beside it the forward alone, the
                  fused chain alone (widening + step per captured qkv) and the ATen chain alone on the same captured qkv

Shapes: the ViT-L 3-D trunk at 60 x 256 x 256 (N 5121, H 16, HD 64, 24 blocks) at batch 1 and 4; the 2-D ViT-L at 224^2 and 512^2
(N 197, 1025) at batch 1.  HIP events around each form on the launch stream, everything warmed up first, the two forms alternated
inside one loop so that both see the same machine; median (min .. max) of the repeats.  "held" is the peak of
torch.cuda.max_memory_allocated() above what was allocated before the call: workspace and temporaries, the operands not counted.
Until this has run on an MI355X no time and no ratio is claimed anywhere.

    python tools/bench_rollout.py [--reps 5] [--out profiles/rollout_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from octcubem_amd import models_vit, models_vit_st, ops, saliency  # noqa: E402

CHUNK_BYTES = 1 << 30


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def fmt(ts):
    return f"{statistics.median(ts):9.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def held(fn):
    """peak bytes allocated during fn above what was allocated before it"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def aten_step(q, k, B, N, H, HD, scale, r, fusion):
    """the same step from ATen ops: per sample, rows in chunks whose [H, rows, N] f32 probabilities stay at or below 1 GiB"""
    rows = max(1, min(N, CHUNK_BYTES // (4 * H * N)))
    out = torch.zeros_like(r)
    qv, kv = q.view(B, N, H, HD), k.view(B, N, H, HD)
    for b in range(B):
        kt = kv[b].permute(1, 2, 0)                                     # [H, HD, N]
        for i0 in range(0, N, rows):
            qc = qv[b, i0:i0 + rows].permute(1, 0, 2)                   # [H, rows, HD]
            P = torch.softmax(torch.matmul(qc, kt) * scale, dim=-1)     # [H, rows, N]
            Fu = P.mean(dim=0) if fusion == "mean" else (P.amax(dim=0) if fusion == "max" else P.amin(dim=0))
            rc = r[b, i0:i0 + rows]
            c = rc * 0.5 if fusion == "mean" else rc / (1.0 + Fu.sum(dim=1))
            out[b] += c @ Fu
            out[b, i0:i0 + rows] += c
    return out


def widen(qkv, B, N, H, HD):
    C = H * HD
    qk = qkv.detach().view(B * N, 3 * C)[:, :2 * C].float()
    return qk[:, :C], qk[:, C:]


def chain(seen, r, fusion, step):
    for qkv, B, N, H, HD, scale in reversed(seen):
        q, k = widen(qkv, B, N, H, HD)
        r = step(q, k, B, N, H, HD, scale, r, fusion)
    return r


def fused_step(q, k, B, N, H, HD, scale, r, fusion):
    return ops.rollout_step(q, k, B, N, H, HD, scale, r, fusion)


def alternate(reps, a, b):
    a(); b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(a)); tb.append(timed(b))
    return ta, tb


def bench(label, model, x, reps, lines):
    dev = x.device
    with torch.no_grad(), ops.capture_attention() as seen:
        model.eval()(x)
    _, B, N, H, HD, scale = seen[0]
    depth = len(seen)
    lines += [f"{label}: B {B}, N {N}, H {H}, HD {HD}, {depth} blocks; captured qkv {sum(e[0].numel() * 2 for e in seen) / 1e6:.0f} MB"]
    g = torch.Generator().manual_seed(3)
    r = torch.rand(B, N, generator=g).to(dev)
    q, k = widen(seen[depth // 2][0], B, N, H, HD)
    flop = 2.0 * B * H * N * N * HD
    for fusion, walks in (("mean", 2), ("max", 3)):
        fu = lambda: fused_step(q, k, B, N, H, HD, scale, r, fusion)              # noqa: E731
        at = lambda: aten_step(q, k, B, N, H, HD, scale, r, fusion)               # noqa: E731
        got, ref = fu(), at()
        err = float((got - ref).abs().max() / ref.abs().max())
        tf, ta = alternate(reps, fu, at)
        mf, ma = held(fu), held(at)
        lines += [f"  one step, {fusion:4s}  fused {fmt(tf)} ms  {walks * flop / statistics.median(tf) / 1e9:6.1f} TFLOP/s over {walks} walks, held {mf / 1e6:8.1f} MB"
                  f"   ATen {fmt(ta)} ms, held {ma / 1e6:8.1f} MB   ATen / fused x {statistics.median(ta) / statistics.median(tf):.2f}"
                  f"   max |fused - ATen| / max |ATen| {err:.1e}"]
    fwd = lambda: model(x)                                                       # noqa: E731
    whole = lambda: saliency.attention_rollout(model, x)                         # noqa: E731
    with torch.no_grad():
        tw, tfw = alternate(reps, whole, fwd)
        r0 = torch.zeros(B, N, device=dev)
        r0[:, 0] = 1.0
        tc, tac = alternate(reps, lambda: chain(seen, r0, "mean", fused_step), lambda: chain(seen, r0, "mean", aten_step))
    a, b = saliency.attention_rollout(model, x)["tokens"], saliency.attention_rollout(model, x)["tokens"]
    lines += [f"  whole call, mean  attention_rollout {fmt(tw)} ms   forward alone {fmt(tfw)} ms   fused chain alone {fmt(tc)} ms   "
              f"ATen chain alone {fmt(tac)} ms   ATen / fused x {statistics.median(tac) / statistics.median(tc):.2f}   "
              f"two calls bit-equal: {bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    lines = [f"attention rollout; {torch.cuda.get_device_name(0)}; operands {ops.BF16}; {a.reps} alternated repeats, HIP events, ms: median (min .. max)"]
    g = torch.Generator().manual_seed(1)
    m3 = models_vit_st.vit_large_patch16(num_frames=60, t_patch_size=3, img_size=256, in_chans=1, num_classes=8, sep_pos_embed=True,
                                         cls_embed=True, global_pool=True, dropout=0.0).to(dev)
    for B in (1, 4):
        bench(f"ViT-L 3-D trunk, 60 x 256 x 256, batch {B}", m3, torch.rand(B, 1, 60, 256, 256, generator=g).to(dev), a.reps, lines)
    del m3
    for size in (224, 512):
        m2 = models_vit.vit_large_patch16(img_size=size, in_chans=3, num_classes=8, global_pool=True).to(dev)
        bench(f"ViT-L 2-D, {size} x {size}, batch 1", m2, torch.rand(1, 3, size, size, generator=g).to(dev), a.reps, lines)
        del m2
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
