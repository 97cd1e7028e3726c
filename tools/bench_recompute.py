"""Step time and peak allocated memory of the three activation-recomputation levels (video_vit.set_recompute: none / light / full), in
one run, on the two workloads the levels are for:

    python tools/bench_recompute.py [--out profiles/recompute_bench.txt]

(a) the ViT-L OCT tower (models_vit_st, flash blocks) on unmasked 60 x 256 x 256 volumes: 5121 tokens per volume, forward + backward;
(b) a ViT-L pre-training micro-batch (models_mae.octcube_vit_large_3dmae, 75 % masking): forward + backward.
Per level: time per step from device events around --reps steps, median [min .. max] of --rounds windows with the three levels
alternating; ``torch.cuda.max_memory_allocated()`` of one step, and what of it the step itself added (the peak minus what was allocated
before the step: parameters, their 16-bit copy, the gradient arena, the input).  Level none is the code path without this feature: the
comparison point of the same run.  Before anything is timed the loss and the whole gradient arena of light and full are compared with
those of none -- and none with a second run of itself: the bit equality the tests show at their sizes holds here as far as level none
repeats itself."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from octcubem_amd import models_mae, models_vit_st, ops, video_vit      # noqa: E402

LEVELS = ("none", "light", "full")

ap = argparse.ArgumentParser()
ap.add_argument("--tower-batch", type=int, default=4)
ap.add_argument("--mae-batch", type=int, default=32)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--cases", nargs="+", default=["tower", "mae"], choices=["tower", "mae"])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recompute_bench.txt"))
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_recompute: needs an MI355X (a timing taken without one says nothing)")
dev = torch.device("cuda")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps       # milliseconds per step


def case(title, model, step):
    say(f"## {title}")
    model.train()

    def at(level):
        def run():
            video_vit.set_recompute(model, level)
            model.arena.zero_grad()
            torch.manual_seed(1)          # the tower's dropout in front of its head: the same masks in every step
            return step()
        return run
    paths = {level: at(level) for level in LEVELS}
    # level none twice: what one code path differs from itself by (at these sizes the split-K weight gradients add fp32 atomically)
    ref = [None, None]
    for k in range(2):
        loss = paths["none"]()
        ref[k] = (loss.detach().clone(), model.arena.grad.clone())
    torch.cuda.synchronize()
    gn = float(ref[0][1].double().norm())
    self_diff = float((ref[1][1].double() - ref[0][1].double()).norm()) / gn
    assert torch.equal(ref[0][0], ref[1][0])
    say(f"  level none against itself: loss bit-equal, gradient arena {'bit-equal' if self_diff == 0.0 else f'rel L2 {self_diff:.1e}'}")
    ref = ref[0]
    mem = {}
    for level, fn in paths.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        loss = fn()
        torch.cuda.synchronize()
        mem[level] = (torch.cuda.max_memory_allocated(), torch.cuda.max_memory_allocated() - before)
        if level != "none":
            d = float((model.arena.grad.double() - ref[1].double()).norm()) / gn
            assert torch.equal(loss.detach(), ref[0]), f"{title}: the loss of level {level} is not bit-equal to none's"
            assert d <= max(4 * self_diff, 1e-6), f"{title}: the gradient arena of level {level} is {d:.1e} (rel L2) from none's"
            say(f"  level {level:5s} against none: loss bit-equal, gradient arena {'bit-equal' if d == 0.0 else f'rel L2 {d:.1e}'}")
        del loss
    del ref
    ts = {level: [] for level in LEVELS}
    for _ in range(a.rounds):                      # alternating: a drift of the box hits all three
        for level, fn in paths.items():
            ts[level].append(window(fn, a.reps))
    t0, m0 = statistics.median(ts["none"]), mem["none"][1]
    for level in LEVELS:
        t = statistics.median(ts[level])
        peak, added = mem[level]
        say(f"  {level:5s} {t:9.1f} ms / step [{min(ts[level]):.1f} .. {max(ts[level]):.1f}]  x{t / t0:.3f}   peak allocated {peak / 2 ** 30:7.2f} GiB, "
            f"added by the step {added / 2 ** 30:7.2f} GiB  x{added / m0:.3f}")
    video_vit.set_recompute(model, "none")


say(f"# tools/bench_recompute.py  {torch.cuda.get_device_name(0)}  torch {torch.__version__}  operands {ops.BF16}  forward + backward, median "
    f"[min .. max] of {a.rounds} alternating windows of {a.reps} steps after {a.warmup} per level; x = against level none of this run")
if "tower" in a.cases:
    torch.manual_seed(0)
    tower = models_vit_st.flash_attn_vit_large_patch16(num_frames=60, t_patch_size=3, img_size=256, in_chans=1, num_classes=512,
                                                       sep_pos_embed=True, cls_embed=True).to(dev)
    x = torch.randn(a.tower_batch, 1, 60, 256, 256, device=dev)
    w = torch.randn(a.tower_batch, 512, device=dev)

    def tower_step():
        loss = (tower(x) * w).sum()
        loss.backward()
        return loss
    case(f"(a) models_vit_st ViT-L, flash blocks, 60 x 256 x 256 unmasked (5121 tokens per volume), B = {a.tower_batch}", tower, tower_step)
    del tower, x, w
    torch.cuda.empty_cache()
if "mae" in a.cases:
    torch.manual_seed(0)
    mae = models_mae.octcube_vit_large_3dmae().to(dev)
    vol = torch.randn(a.mae_batch, 1, 60, 256, 256, device=dev)
    noise = torch.rand(a.mae_batch, 20 * 16 * 16, device=dev)

    def mae_step():
        loss, _, _ = mae(vol, mask_ratio=0.75, noise=noise)
        loss.backward()
        return loss
    case(f"(b) models_mae.octcube_vit_large_3dmae, mask_ratio 0.75, micro-batch B = {a.mae_batch}", mae, mae_step)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
