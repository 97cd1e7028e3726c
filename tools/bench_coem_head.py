"""Two timings around the COEM classification models, each against the form it replaces, in one run:

    python tools/bench_coem_head.py [--out profiles/coem_head_bench.txt]

(a) the join in front of the classification head, forward + backward: ops.JoinFn (csrc/join.hip, one kernel each way) against the ATen
    composition the reference runs (F.normalize per tower output, cat, F.layer_norm, a cast to the GEMM's 16-bit operand type, autograd),
    at B in {4, 32, 256}, D = 512, M in {2, 3}, every modality present;
(b) the two-modality en-face tower, forward + backward: ``forward_pair`` (one trunk pass at 2 B) against two ``forward`` calls (two
    passes at B, as the reference), ViT-L at 384 x 384, B in {1, 4, 8}.
Per form: time per call from device events around --reps calls after --warmup untimed ones, median [min .. max] of --rounds windows with
the two forms alternating.  The two forms are compared before anything is timed."""
import argparse
import os
import statistics
import sys
from functools import partial

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from octcubem_amd import models_vit_2mod, ops      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--join-batches", type=int, nargs="+", default=[4, 32, 256])
ap.add_argument("--dim", type=int, default=512)
ap.add_argument("--pair-batches", type=int, nargs="+", default=[1, 4, 8])
ap.add_argument("--image", type=int, default=384)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--pair-reps", type=int, default=8)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coem_head_bench.txt"))
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_coem_head: needs an MI355X (a timing taken without one says nothing)")
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
    return e0.elapsed_time(e1) * 1e3 / reps       # microseconds per call


def race(paths, reps, warmup):
    for fn in paths.values():
        for _ in range(warmup):
            fn()
    ts = {name: [] for name in paths}
    for _ in range(a.rounds):                      # alternating: a drift of the box hits both
        for name, fn in paths.items():
            ts[name].append(window(fn, reps))
    return ts


def join_case(B, M):
    D = a.dim
    g = torch.Generator().manual_seed(B + M)
    fs = [(torch.randn(B, D, generator=g) * (1 + k)).to(dev).requires_grad_(True) for k in range(M)]
    gamma = torch.nn.Parameter((1 + 0.1 * torch.randn(M * D, generator=g)).to(dev))
    beta = torch.nn.Parameter((0.1 * torch.randn(M * D, generator=g)).to(dev))
    dy = torch.randn(B, M * D, generator=g).to(dev).to(ops.BF16)
    mask = (1 << M) - 1

    def clear():
        gamma.grad = beta.grad = None
        for f in fs:
            f.grad = None

    def fused():
        clear()
        y, *_ = ops.JoinFn.apply(gamma, beta, 1e-5, mask, *fs)
        y.backward(dy)
        return y

    def aten():
        clear()
        y = F.layer_norm(torch.cat([F.normalize(f, dim=-1) for f in fs], dim=-1), (M * D,), gamma, beta, 1e-5).to(ops.BF16)
        y.backward(dy)
        return y
    paths = {"fused": fused, "ATen": aten}
    res = {}
    for name, fn in paths.items():
        y = fn()
        res[name] = (y.detach().float(), [f.grad.clone() for f in fs], gamma.grad.clone())
    dyv = float((res["fused"][0] - res["ATen"][0]).norm() / res["ATen"][0].norm())
    dg = max(float((p - q).norm() / q.norm()) for p, q in zip(res["fused"][1] + [res["fused"][2]], res["ATen"][1] + [res["ATen"][2]]))
    assert dyv <= 5e-3 and dg <= 1e-4, f"join B = {B}, M = {M}: the forms differ (y {dyv:.2e}, gradients {dg:.2e})"
    say(f"join  B = {B}, D = {D}, M = {M}: forms agree to {dyv:.1e} (y, rel L2 in the 16-bit type) / {dg:.1e} (gradients)")
    ts = race(paths, a.reps, a.warmup)
    for name in paths:
        say(f"  {name:6s} {statistics.median(ts[name]):10.1f} us / call [{min(ts[name]):.1f} .. {max(ts[name]):.1f}]")


def pair_case(tower, B):
    g = torch.Generator().manual_seed(B)
    x0 = torch.randn(B, 3, a.image, a.image, generator=g).to(dev)
    x1 = torch.randn(B, 3, a.image, a.image, generator=g).to(dev)
    w = torch.randn(B, tower.out_dim, generator=g).to(dev)

    def pair():
        tower.arena.zero_grad()
        y0, y1 = tower.forward_pair(x0, x1)
        ((y0 * w).sum() + (y1 * w).sum()).backward()
        return y0, y1

    def two():
        tower.arena.zero_grad()
        y0 = tower(x0, modality=0)
        (y0 * w).sum().backward()
        y1 = tower(x1, modality=1)
        (y1 * w).sum().backward()
        return y0, y1
    paths = {"pair": pair, "two": two}
    res = {}
    for name, fn in paths.items():
        y0, y1 = fn()
        res[name] = (torch.cat([y0, y1]).detach(), tower.arena.grad.clone())
    dyv = float((res["pair"][0] - res["two"][0]).norm() / res["two"][0].norm())
    dg = float((res["pair"][1] - res["two"][1]).norm() / res["two"][1].norm())
    assert dyv <= 2e-2 and dg <= 6e-2, f"pair B = {B}: the forms differ (features {dyv:.2e}, gradient arena {dg:.2e})"
    say(f"tower B = {B} per modality, {a.image} x {a.image}: forms agree to {dyv:.1e} (features, rel L2) / {dg:.1e} (gradient arena)")
    ts = race(paths, a.pair_reps, 2)
    for name in paths:
        say(f"  {name:6s} {statistics.median(ts[name]) / 1e3:10.2f} ms / call [{min(ts[name]) / 1e3:.2f} .. {max(ts[name]) / 1e3:.2f}]")


say(f"# tools/bench_coem_head.py  {torch.cuda.get_device_name(0)}  torch {torch.__version__}  operands {ops.BF16}  forward + backward, median "
    f"[min .. max] of {a.rounds} alternating windows")
say(f"# (a) the join: {a.reps} calls per window after {a.warmup}")
for M in (2, 3):
    for B in a.join_batches:
        join_case(B, M)
say(f"# (b) models_vit_2mod ViT-L (24 blocks, width 1024, out_dim 512), train(), drop_path_rate 0: {a.pair_reps} calls per window after 2")
torch.manual_seed(0)
tower = models_vit_2mod.VisionTransformer(image_size=a.image, out_dim=512, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4,
                                          norm_layer=partial(torch.nn.LayerNorm, eps=1e-6)).to(dev).train()
for B in a.pair_batches:
    pair_case(tower, B)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
