"""The ConvNeXt layer kernels of the SLIViT baseline (csrc/convnext.hip) against ATen / MIOpen, in one run.

    python tools/bench_convnext.py [--out profiles/convnext_bench.txt]

1. ops.dwconv7_fwd / dwconv7_bwd_input / dwconv7_bwd_weight at the four stage shapes of a volume of P = 20 slices laid side by side
   ([1, 64, 1280, 96], [1, 32, 640, 192], [1, 16, 320, 384], [1, 8, 160, 768], channels-last fp32) and at batch 8 of the same, each
   against ``F.conv2d(groups=C)`` / ``aten.convolution_backward`` on the same memory (a channels_last view, fp32): time per call from
   device events around --reps calls after --warmup untimed ones, median [min .. max] of --rounds windows with the two paths
   alternating.  Algorithmic bytes: 4 B read + 4 B written per element forward and for the input gradient, two 4 B reads per element
   for the weight gradient; the share of HBM bandwidth is those bytes over the time over 6.29 TB/s (the measured copy rate; 8 TB/s spec).
   The inputs of the small shapes fit the caches: their "share" can exceed what HBM could deliver, and says so.
2. A whole ConvNeXt-T feature extractor, forward + backward, on a P = 20 volume [1, 3, 256, 5120]: model_slivit_baseline's against the
   ATen composition of the same weights (tests/slivit_ref.extractor_forward: conv2d / layer_norm / linear / gelu on channels-last
   views), the latter in fp32 and under bfloat16 autocast.
The two paths of every row are compared before anything is timed."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from octcubem_amd import model_slivit_baseline as M, ops      # noqa: E402
import slivit_ref as R      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--model-reps", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convnext_bench.txt"))
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_convnext: needs an MI355X (a timing taken without one says nothing)")
dev = torch.device("cuda")
HBM = 6.29e12
STAGES = [(64, 1280, 96), (32, 640, 192), (16, 320, 384), (8, 160, 768)]
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


def compare(tag, paths, nbytes, reps, warmup):
    for fn in paths.values():
        for _ in range(warmup):
            fn()
    ts = {name: [] for name in paths}
    for _ in range(a.rounds):                      # alternating: a drift of the machine hits both
        for name, fn in paths.items():
            ts[name].append(window(fn, reps))
    med = {name: statistics.median(v) for name, v in ts.items()}
    cells = []
    for name in paths:
        share = f"  {nbytes / (med[name] * 1e-6) / HBM * 100:5.1f} % of HBM" if nbytes else ""
        cells.append(f"{name} {med[name]:9.1f} us [{min(ts[name]):.1f} .. {max(ts[name]):.1f}]{share}")
    names = list(paths)
    say(f"  {tag:14s} " + "   ".join(cells) + f"   {names[0]} / {names[1]} = {med[names[0]] / med[names[1]]:.2f}")
    return med


def rel(x, y):
    return float((x.double() - y.double()).norm() / y.double().norm())


def kernels(B, H, W, C):
    g = torch.Generator().manual_seed(H + C + B)
    x = torch.randn((B, H, W, C), generator=g).to(dev)
    dz = torch.randn((B, H, W, C), generator=g).to(dev)
    wt = (torch.randn((C, 7, 7), generator=g) / 7).to(dev)
    bias = torch.randn((C,), generator=g).to(dev)
    gw, gb = torch.zeros_like(wt), torch.zeros_like(bias)
    xc, dzc, w4 = x.permute(0, 3, 1, 2), dz.permute(0, 3, 1, 2), wt.view(C, 1, 7, 7)      # channels_last views of the same memory
    assert xc.is_contiguous(memory_format=torch.channels_last) or B * H * W == 1 or C == 1

    def aten_bwd(mask):
        return torch.ops.aten.convolution_backward(dzc, xc, w4, [C], [1, 1], [3, 3], [1, 1], False, [0, 0], C, mask)

    n = x.numel()
    say(f"[{B}, {H}, {W}, {C}]  {4 * n / 2 ** 20:.1f} MiB per map")
    ref = F.conv2d(xc, w4, bias, padding=3, groups=C).permute(0, 2, 3, 1)
    d_f = rel(ops.dwconv7_fwd(x, wt, bias), ref)
    d_i = rel(ops.dwconv7_bwd_input(dz, wt), aten_bwd([True, False, False])[0].permute(0, 2, 3, 1))
    ops.dwconv7_bwd_weight(dz, x, gw, gb)
    _, rw, rb = aten_bwd([False, True, True])
    d_w = max(rel(gw, rw.view(C, 7, 7)), rel(gb, rb))
    assert max(d_f, d_i, d_w) <= 1e-4, (d_f, d_i, d_w)
    say(f"  paths agree to {d_f:.1e} (forward) / {d_i:.1e} (input gradient) / {d_w:.1e} (weight, bias gradient), rel L2")
    compare("forward", {"HIP": lambda: ops.dwconv7_fwd(x, wt, bias), "ATen": lambda: F.conv2d(xc, w4, bias, padding=3, groups=C)}, 8.0 * n,
            a.reps, a.warmup)
    compare("input grad", {"HIP": lambda: ops.dwconv7_bwd_input(dz, wt), "ATen": lambda: aten_bwd([True, False, False])}, 8.0 * n,
            a.reps, a.warmup)
    compare("weight grad", {"HIP": lambda: ops.dwconv7_bwd_weight(dz, x, gw, gb), "ATen": lambda: aten_bwd([False, True, True])}, 8.0 * n,
            a.reps, a.warmup)


def whole_model():
    torch.manual_seed(0)
    fe = M.ConvNextFeatureExtractor().to(dev)
    with torch.no_grad():                          # HF's 1e-6 layer scale makes every branch invisible: compare and time at O(1)
        for n_, p in fe.named_parameters():
            if n_.endswith("layer_scale_parameter"):
                p.fill_(0.5)
    cfg = dict(depths=fe.depths, hidden_sizes=fe.hidden_sizes)
    P = {k: v.detach().clone().requires_grad_(True) for k, v in fe.state_dict().items()}
    img = torch.randn((1, 3, 256, 5120), generator=torch.Generator().manual_seed(3)).to(dev)

    def hip():
        fe.arena.zero_grad()
        out = fe(img)
        out.square().mean().backward()
        return out

    def aten(amp):
        def run():
            for p in P.values():
                p.grad = None
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                out = R.extractor_forward(P, img, cfg, None)
            out.float().square().mean().backward()
            return out
        return run

    o_h, o_a = hip().detach().float(), aten(False)().detach().float()
    gk = "1.stages.0.layers.0.dwconv.weight"
    g_h, g_a = dict(fe.named_parameters())[gk].grad.clone(), P[gk].grad.clone()
    say(f"ConvNeXt-T (depths {fe.depths}, widths {fe.hidden_sizes}) on [1, 3, 256, 5120], forward + backward: features agree to "
        f"{rel(o_h, o_a):.1e}, the first depthwise filter's gradient to {rel(g_h, g_a):.1e} (rel L2, 16-bit operands against fp32)")
    compare("fwd + bwd", {"HIP": hip, "ATen fp32": aten(False)}, 0, a.model_reps, 2)
    compare("fwd + bwd", {"HIP": hip, "ATen bf16 autocast": aten(True)}, 0, a.model_reps, 2)


say(f"# tools/bench_convnext.py  {torch.cuda.get_device_name(0)}  torch {torch.__version__}  operands {ops.BF16}  {a.reps} calls per window "
    f"after {a.warmup}, median [min .. max] of {a.rounds} alternating windows; HBM share = algorithmic bytes / time / 6.29 TB/s")
for B in a.batches:
    for H, W, C in STAGES:
        kernels(B, H, W, C)
whole_model()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
