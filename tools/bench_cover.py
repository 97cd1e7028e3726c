#!/usr/bin/env python3
"""Times the full-coverage reconstruction kernels (csrc/cover.hip) against the same result composed from ATen ops on the same GPU:

  accumulate      ops.cover_accumulate on the [:, 1:, :] view of a [B, 1 + L, PD] buffer, first pass and a later pass at mask ratio 0.75,
                  against  sum = torch.where(mask, sum + pred, sum); cnt += mask
  finish          ops.cover_finish (recon, err, score) against  v = sum / cnt -> unpatchify -> the three level ops, clip and cast ->
                  (v - x) ** 2 -> per-token mean, with the temporaries ATen allocates for them
  the whole call  model.reconstruct_full on the ViT-L 3-D MAE beside its K forwards alone: the share of the call that is not forwards

Shape: ViT-L's, 60 x 256 x 256 volumes, p 16, u 3 (L 5120, PD 768), batches 1 and 8.  HIP events around each form on the launch
stream, everything warmed up first, the two forms alternated inside one loop so that both see the same machine; median (min .. max)
of the repeats.  "held" is the peak of torch.cuda.max_memory_allocated() above what was allocated before the call: outputs and
temporaries, the operands not counted (the kernels' outputs are counted too: recon, err and score are allocated in the call).
GB/s is the algorithmic byte count ops.py states for the launch over the median.  Until this has run on an MI355X no time and no
ratio is claimed anywhere.

    python tools/bench_cover.py [--reps 7] [--out profiles/cover_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from octcubem_amd import models_mae, ops  # noqa: E402

T, H, W, P, U = 60, 256, 256, 16, 3
L, PD = (T // U) * (H // P) * (W // P), U * P * P
IMG_MEAN, IMG_STD = 45.79 / 255, 76.03 / 255


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def fmt(ts):
    return f"{statistics.median(ts):8.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def held(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def alternate(reps, a, b):
    a(); b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(a)); tb.append(timed(b))
    return ta, tb


def aten_accumulate(pred, mask, acc, cnt):
    m = mask != 0
    return torch.where(m.unsqueeze(-1), acc + pred, acc), cnt + m.to(torch.int32)


def aten_finish(acc, cnt, imgs):
    B = acc.shape[0]
    t, h, w = T // U, H // P, W // P
    seen = (cnt > 0).view(B, L, 1)
    x = torch.einsum("nctuhpwq->nthwupqc", imgs.reshape(B, 1, t, U, h, P, w, P)).reshape(B, L, PD)
    v = acc / cnt.clamp(min=1).to(torch.float32).view(B, L, 1)
    d = v - x
    e = torch.where(seen, d * d, torch.zeros((), device=acc.device))
    v = torch.where(seen, v, x)
    un = lambda z: torch.einsum("nthwupqc->nctuhpwq", z.reshape(B, t, h, w, U, P, P, 1)).reshape(B, T, H, W)      # noqa: E731
    vol = un(v)
    recon = torch.where(torch.isfinite(vol), torch.clip((vol * IMG_STD + IMG_MEAN) * 255, 0, 255), torch.zeros((), device=acc.device))
    return recon.to(torch.uint8), un(e), e.mean(dim=-1)


def bench_kernels(B, reps, lines):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(B)
    imgs = (torch.rand(B, 1, T, H, W, generator=g) * 3.6 - 0.7).to(dev)
    full = [(torch.rand(B, 1 + L, PD, generator=g) * 3.6 - 0.7).to(dev) for _ in range(2)]
    preds = [f[:, 1:, :] for f in full]
    masks = [(torch.rand(B, L, generator=g) < 0.75).float().to(dev) for _ in range(2)]
    acc, cnt = ops.cover_accumulate(preds[0], masks[0])
    zero, zcnt = torch.zeros_like(acc), torch.zeros_like(cnt)
    ref_acc, ref_cnt = aten_accumulate(preds[0], masks[0], zero, zcnt)
    same = [bool(torch.equal(acc, ref_acc) and torch.equal(cnt, ref_cnt))]
    nb = 4.0 * B * L * PD
    lines += [f"batch {B}: L {L}, PD {PD}; pred / sum {nb / 1e6:.0f} MB each, volume {4.0 * B * T * H * W / 1e6:.0f} MB"]
    # first pass: the kernel writes every row (no zero fill in front); ATen adds into a zero buffer that the fill launch wrote
    tf, ta = alternate(reps, lambda: ops.cover_accumulate(preds[0], masks[0], acc, cnt, first=True),
                       lambda: aten_accumulate(preds[0], masks[0], torch.zeros_like(acc), torch.zeros_like(cnt)))
    mf, ma = held(lambda: ops.cover_accumulate(preds[0], masks[0])), held(lambda: aten_accumulate(preds[0], masks[0], torch.zeros_like(acc), torch.zeros_like(cnt)))
    lines += [f"  accumulate, first   kernel {fmt(tf)} ms  {(0.75 + 1) * nb / statistics.median(tf) / 1e6:7.0f} GB/s, held {mf / 1e6:7.1f} MB"
              f"   ATen {fmt(ta)} ms, held {ma / 1e6:7.1f} MB   ATen / kernel x {statistics.median(ta) / statistics.median(tf):.2f}"]
    # a later pass: in place on the masked rows; ATen writes a new sum
    work = acc.clone(), cnt.clone()
    tf, ta = alternate(reps, lambda: ops.cover_accumulate(preds[1], masks[1], *work), lambda: aten_accumulate(preds[1], masks[1], acc, cnt))
    mf, ma = held(lambda: ops.cover_accumulate(preds[1], masks[1], *work)), held(lambda: aten_accumulate(preds[1], masks[1], acc, cnt))
    lines += [f"  accumulate, later   kernel {fmt(tf)} ms  {0.75 * 3 * nb / statistics.median(tf) / 1e6:7.0f} GB/s, held {mf / 1e6:7.1f} MB"
              f"   ATen {fmt(ta)} ms, held {ma / 1e6:7.1f} MB   ATen / kernel x {statistics.median(ta) / statistics.median(tf):.2f}"]
    acc2, cnt2 = ops.cover_accumulate(preds[1], masks[1], acc.clone(), cnt.clone())
    ref2, rcnt2 = aten_accumulate(preds[1], masks[1], ref_acc, ref_cnt)
    same.append(bool(torch.equal(acc2, ref2) and torch.equal(cnt2, rcnt2)))
    got, ref = ops.cover_finish(acc2, cnt2, imgs, None, U, P), aten_finish(acc2, cnt2, imgs)
    same.append(bool(torch.equal(got[1], ref[1])))
    level = int((got[0].int() - ref[0].int()).abs().max())
    rel = float(((got[2] - ref[2]).abs() / ref[2].abs().clamp(min=1e-30)).max())
    del got, ref
    tf, ta = alternate(reps, lambda: ops.cover_finish(acc2, cnt2, imgs, None, U, P), lambda: aten_finish(acc2, cnt2, imgs))
    mf, ma = held(lambda: ops.cover_finish(acc2, cnt2, imgs, None, U, P)), held(lambda: aten_finish(acc2, cnt2, imgs))
    fin_bytes = 2 * nb + 4.0 * B * L * 2 + 5.0 * B * T * H * W
    lines += [f"  finish              kernel {fmt(tf)} ms  {fin_bytes / statistics.median(tf) / 1e6:7.0f} GB/s, held {mf / 1e6:7.1f} MB"
              f"   ATen {fmt(ta)} ms, held {ma / 1e6:7.1f} MB   ATen / kernel x {statistics.median(ta) / statistics.median(tf):.2f}",
              f"  kernel == ATen: sums after the first pass {same[0]}, after the second {same[1]}, err volume {same[2]}; largest level "
              f"difference {level} (the ATen chain leaves v * s + m to one fused op or three, as the dispatcher has it); token score "
              f"max relative difference {rel:.1e} (another summation order)"]


def bench_model(B, reps, lines):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = models_mae.octcube_vit_large_3dmae().to(dev).eval()
    x = (torch.rand(B, 1, T, H, W, generator=torch.Generator().manual_seed(7)) * 3.6 - 0.7).to(dev)
    noise = models_mae.cover_noise(B, L, 0.75, generator=torch.Generator().manual_seed(1), device=dev)

    def forwards():
        with torch.no_grad():
            for k in range(noise.shape[0]):
                m(x, 0.75, noise=noise[k])

    whole = lambda: m.reconstruct_full(x, 0.75, generator=torch.Generator().manual_seed(1))      # noqa: E731
    tw, tf = alternate(reps, whole, forwards)
    a, b = whole(), whole()
    same = all(torch.equal(a[k], b[k]) for k in ("recon", "count")) and \
        all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in ("error", "token_score"))
    share = 1.0 - statistics.median(tf) / statistics.median(tw)
    lines += [f"reconstruct_full, ViT-L 3-D MAE, batch {B}, {a['passes']} passes: whole call {fmt(tw)} ms   its {a['passes']} forwards alone "
              f"{fmt(tf)} ms   share that is not forwards {100 * share:.1f} % (schedule draw on the host and its upload, accumulate, "
              f"finish, frame and volume means, the loss read-back)   two calls bit-equal: {same}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cover: needs the GPU; nothing is measured without one")
    lines = [f"full-coverage reconstruction; {torch.cuda.get_device_name(0)}; {a.reps} alternated repeats, HIP events, ms: median (min .. max)"]
    for B in (1, 8):
        bench_kernels(B, a.reps, lines)
        torch.cuda.empty_cache()
    for B in (1, 2):
        bench_model(B, a.reps, lines)
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
