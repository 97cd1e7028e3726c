"""The slice embedding of OCTCube's SLIViT head (csrc/slabnorm.hip, ops.SliceEmbedFn) against the ATen composition it replaces, in one run.

    python tools/bench_slice_embed.py [--out profiles/slice_embed_bench.txt]

At the ViT-L shape (C = 1024, L = 256, T = 20: rows of K = 262144) for 1, 4 and 8 volumes, forward + backward:
1. the two new kernels alone -- ops.slab_norm_fwd, ops.slab_norm_bwd (with dgamma / dbeta) -- against what ATen needs for the same
   result: ``x[:, 1:].view(N, T, L, C).transpose(2, 3).reshape(N * T, K)`` (a materialised fp32 transpose), ``F.layer_norm``, a cast to the
   16-bit operand type; and autograd's backward of that chain from a 16-bit gradient;
2. ops.SliceEmbedFn whole against that chain in front of the SAME GEMMs (ops.LinearFn) on the same weights.
Time per call from device events around --reps calls after --warmup untimed ones, median [min .. max] of --rounds windows with the
two paths alternating.  Bytes model of the kernels (algorithmic: every operand once): forward 4 (x) + 2 (A) per element + 8 K (gamma,
beta); backward 2 (dA) + 4 (x) + 4 (dx) per element + 12 K (gamma read, dgamma / dbeta updated); the share of HBM bandwidth is those
bytes over the time over 6.29 TB/s (the measured copy rate; 8 TB/s spec).  The kernels read x twice (statistics, then the transposing
pass), which the model does not count.  Peak memory: torch's allocator peak during one forward + backward above what is allocated
before it (the operands: x, the weights, their gradient buffers).
The two paths of every row are compared before anything is timed."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from octcubem_amd import ops      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--volumes", type=int, nargs="+", default=[1, 4, 8])
ap.add_argument("--C", type=int, default=1024)
ap.add_argument("--L", type=int, default=256)
ap.add_argument("--T", type=int, default=20)
ap.add_argument("--dim", type=int, default=256)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slice_embed_bench.txt"))
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_slice_embed: needs an MI355X (a timing taken without one says nothing)")
dev = torch.device("cuda")
HBM = 6.29e12
EPS = 1e-5
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


def compare(tag, paths, nbytes):
    for fn in paths.values():
        for _ in range(a.warmup):
            fn()
    ts = {name: [] for name in paths}
    for _ in range(a.rounds):                      # alternating: a drift of the machine hits both
        for name, fn in paths.items():
            ts[name].append(window(fn, a.reps))
    med = {name: statistics.median(v) for name, v in ts.items()}
    cells = []
    for name in paths:
        share = f"  {nbytes / (med[name] * 1e-6) / HBM * 100:5.1f} % of HBM" if nbytes else ""
        cells.append(f"{name} {med[name]:9.1f} us [{min(ts[name]):.1f} .. {max(ts[name]):.1f}]{share}")
    names = list(paths)
    say(f"  {tag:22s} " + "   ".join(cells) + f"   {names[0]} / {names[1]} = {med[names[0]] / med[names[1]]:.2f}")
    return med


def rel(x, y):
    return float((x.double() - y.double()).norm() / y.double().norm())


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def case(N):
    C, L, T, D = a.C, a.L, a.T, a.dim
    K, rows = C * L, N * T
    g = torch.Generator().manual_seed(N)
    x = (torch.randn((N, 1 + T * L, C), generator=g) * 1.5 + 0.3).to(dev).requires_grad_(True)
    gamma = torch.nn.Parameter((1 + 0.1 * torch.randn(K, generator=g)).to(dev))
    beta = torch.nn.Parameter((0.1 * torch.randn(K, generator=g)).to(dev))
    W = torch.nn.Parameter((torch.randn((D, K), generator=g) * K ** -0.5).to(dev))
    b = torch.nn.Parameter((0.1 * torch.randn(D, generator=g)).to(dev))
    for p in (gamma, beta, W, b):
        p.grad = torch.zeros_like(p)
    w_lp = W.detach().to(ops.BF16)
    dy = torch.randn((N, T, D), generator=g).to(dev)
    dA = torch.randn((rows, K), generator=g).to(dev).to(ops.BF16)
    say(f"[{N} volumes]  rows {rows} x K {K}: x {4 * x.numel() / 2 ** 20:.0f} MiB, A {2 * rows * K / 2 ** 20:.0f} MiB, weight {2 * D * K / 2 ** 20:.0f} MiB (16-bit)")

    def aten_rows(xx):
        return xx[:, 1:, :].view(N, T, L, C).transpose(2, 3).reshape(rows, K)

    # ---- the kernels alone
    xd = x.detach()
    A, mean, rstd = ops.slab_norm_fwd(xd, gamma.detach(), beta.detach(), EPS, T, L, 1)
    A_ref = F.layer_norm(aten_rows(xd), (K,), gamma.detach(), beta.detach(), EPS)
    xr = xd.clone().requires_grad_(True)
    gr, br = gamma.detach().clone().requires_grad_(True), beta.detach().clone().requires_grad_(True)
    y_ref = F.layer_norm(aten_rows(xr), (K,), gr, br, EPS)
    y_ref.backward(dA.float())
    dgm, dbt = torch.zeros(K, device=dev), torch.zeros(K, device=dev)
    dx = ops.slab_norm_bwd(dA, xd, mean, rstd, gamma.detach(), T, L, 1, dgm, dbt)
    d_f, d_x, d_g = rel(A.float(), A_ref), rel(dx, xr.grad), max(rel(dgm, gr.grad), rel(dbt, br.grad))
    say(f"  kernels agree with ATen to {d_f:.1e} (A, one 16-bit rounding) / {d_x:.1e} (dx) / {d_g:.1e} (dgamma, dbeta), rel L2")
    assert d_f <= 6e-3 and d_x <= 1e-4 and d_g <= 1e-4, (d_f, d_x, d_g)
    del A_ref, y_ref, xr

    def aten_fwd():
        return F.layer_norm(aten_rows(xd), (K,), gamma.detach(), beta.detach(), EPS).to(ops.BF16)

    xg = xd.clone().requires_grad_(True)
    yg = F.layer_norm(aten_rows(xg), (K,), gamma, beta, EPS)
    dAf = dA.float()

    def aten_bwd():
        return torch.autograd.grad(yg, (xg, gamma, beta), dAf, retain_graph=True)

    compare("slab LayerNorm fwd", {"HIP": lambda: ops.slab_norm_fwd(xd, gamma.detach(), beta.detach(), EPS, T, L, 1), "ATen": aten_fwd},
            6.0 * rows * K + 8.0 * K)
    compare("slab LayerNorm bwd", {"HIP": lambda: ops.slab_norm_bwd(dA, xd, mean, rstd, gamma.detach(), T, L, 1, dgm, dbt), "ATen": aten_bwd},
            10.0 * rows * K + 12.0 * K)
    del xg, yg, dAf

    # ---- the slice embedding whole: forward + backward on the same weights
    def fused():
        x.grad = None
        y = ops.SliceEmbedFn.apply(x, gamma, beta, EPS, T, L, 1, w_lp, b.detach(), lambda: W.grad, lambda: b.grad, W, b)
        y.backward(dy)
        return y

    def aten():
        x.grad = None
        yn = F.layer_norm(aten_rows(x), (K,), gamma, beta, EPS)
        y = ops.LinearFn.apply(yn, w_lp, b.detach(), lambda: W.grad, lambda: b.grad, True, W, b).view(N, T, D)
        y.backward(dy)
        return y

    for p in (gamma, beta, W, b):
        p.grad.zero_()
    yf = fused().detach().clone()
    gf = (x.grad.clone(), W.grad.clone(), gamma.grad.clone())
    for p in (gamma, beta, W, b):
        p.grad.zero_()
    ya = aten().detach().clone()
    ga = (x.grad.clone(), W.grad.clone(), gamma.grad.clone())
    say(f"  forms agree to {rel(yf, ya):.1e} (output) / {rel(gf[0], ga[0]):.1e} (dx) / {rel(gf[1], ga[1]):.1e} (weight gradient) / "
        f"{rel(gf[2], ga[2]):.1e} (dgamma), rel L2")
    del gf, ga
    compare("slice embed fwd + bwd", {"SliceEmbedFn": fused, "ATen + GEMMs": aten}, 0)
    pf, pa = peak_above(fused), peak_above(aten)
    say(f"  peak memory above the operands, one forward + backward: SliceEmbedFn {pf:.0f} MiB   ATen + GEMMs {pa:.0f} MiB")


say(f"# tools/bench_slice_embed.py  {torch.cuda.get_device_name(0)}  torch {torch.__version__}  operands {ops.BF16}  C {a.C} L {a.L} T {a.T} "
    f"dim {a.dim}; {a.reps} calls per window after {a.warmup}, median [min .. max] of {a.rounds} alternating windows; HBM share = "
    f"algorithmic bytes / time / 6.29 TB/s")
for N in a.volumes:
    case(N)
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
