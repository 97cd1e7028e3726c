"""Forward + backward of the COEM contrastive loss two ways, in one run: the fused kernel path (ClipLoss(fused=True) ->
ops.clip_pair_loss, csrc/cliploss.hip: no [n, m] array) and the unchanged ATen composition (ClipLoss(fused=False): logits matmul,
transpose, two cross entropies, autograd).

    python tools/bench_cliploss.py [--out profiles/cliploss_bench.txt]

d = 512, scale = 100; the symmetric loss at n = m in {64, 512, 2048, 8192} and the local-loss form (local rows against all gathered
columns, both directions: two rectangular calls / two logits matmuls with offset labels, as ClipLoss forms them under ``local_loss``) at
the shipped shape 32 x 256 (8 ranks x batch 8 x accumulation 4, seen from the last rank) and at 64 x 2048.  Per path and shape: time per
call (forward + backward into leaf features and the temperature) from device events around --reps calls after --warmup untimed ones,
median of --rounds such windows with the two paths alternating; kernel launches per call (torch.profiler, one call); and
torch.cuda.max_memory_allocated over one call above what the operands occupy.  The two paths are compared before anything is timed."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from octcubem_amd import coem, ops      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="+", default=[64, 512, 2048, 8192])
ap.add_argument("--local", type=int, nargs="+", default=[32, 256, 64, 2048], help="pairs: local rows, gathered columns")
ap.add_argument("--dim", type=int, default=512)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cliploss_bench.txt"))
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_cliploss: needs an MI355X (a timing taken without one says nothing)")
dev = torch.device("cuda")
lines = []
SCALE = 100.0


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def features(n, m, seed):
    g = torch.Generator().manual_seed(seed)
    x = F.normalize(torch.randn(n, a.dim, generator=g), dim=-1)
    y = F.normalize(torch.randn(m, a.dim, generator=g), dim=-1)
    y[m - n:] = F.normalize(y[m - n:] + 0.12 * x, dim=-1)          # the partners: the last n columns (the last rank's offset)
    return x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)


def symmetric(fused):
    loss = coem.ClipLoss(cache_labels=True, fused=fused)
    return lambda x, y, s: loss(x, y, s)


def local(fused):
    """ClipLoss's local_loss branch on one process: the local rows of each tower against all gathered rows of the other (the other
    ranks' rows of the first tower are seeded constants, the local rows come last; the concatenation is part of both paths)"""
    others = {}

    def gathered(x, off):
        if off not in others:
            others[off] = F.normalize(torch.randn(off, a.dim, generator=torch.Generator().manual_seed(off)), dim=-1).to(dev)
        return torch.cat([others[off], x])

    def aten(x, y, s):
        n, off = x.shape[0], y.shape[0] - x.shape[0]
        labels = torch.arange(n, device=dev) + off
        return (F.cross_entropy(s * x @ y.T, labels) + F.cross_entropy(s * y[off:] @ gathered(x, off).T, labels)) / 2

    def kern(x, y, s):
        n, off = x.shape[0], y.shape[0] - x.shape[0]
        w = torch.full((n,), 0.5 / n, dtype=torch.float32, device=dev)
        return ops.clip_pair_loss(x, y, s, w, None, off) + ops.clip_pair_loss(y[off:], gathered(x, off), s, w, None, off)
    return kern if fused else aten


def one_call(fn, x, y, s):
    x.grad = y.grad = s.grad = None
    fn(x, y, s).backward()


def window(fn, x, y, s):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(a.reps):
        one_call(fn, x, y, s)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.reps       # microseconds per call


def launches(fn, x, y, s):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            one_call(fn, x, y, s)
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    except Exception as e:      # a profiler that cannot trace here: say so, time anyway
        return f"n/a ({type(e).__name__})"


def peak_extra(fn, x, y, s):
    one_call(fn, x, y, s)
    torch.cuda.synchronize()
    x.grad = y.grad = s.grad = None
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    one_call(fn, x, y, s)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def measure(tag, n, m, make):
    x, y = features(n, m, seed=n + m)
    s = torch.tensor(SCALE, dtype=torch.float32, device=dev, requires_grad=True)
    paths = {"fused": make(True), "ATen": make(False)}
    res = {}
    for name, fn in paths.items():
        one_call(fn, x, y, s)
        res[name] = (float(fn(x, y, s)), x.grad.clone(), y.grad.clone(), float(s.grad))
    dl = abs(res["fused"][0] - res["ATen"][0]) / abs(res["ATen"][0])
    dg = max(float((res["fused"][k] - res["ATen"][k]).norm() / res["ATen"][k].norm()) for k in (1, 2))
    assert dl <= 1e-4 and dg <= 1e-3, f"{tag}: the paths differ (loss {dl:.2e}, gradients {dg:.2e})"
    say(f"{tag}  n = {n}, m = {m}: loss {res['ATen'][0]:.4f}, paths agree to {dl:.1e} (loss) / {dg:.1e} (feature gradients, rel L2)")
    for fn in paths.values():
        for _ in range(a.warmup):
            one_call(fn, x, y, s)
    ts = {name: [] for name in paths}
    for _ in range(a.rounds):                      # alternating: a drift of the box hits both
        for name, fn in paths.items():
            ts[name].append(window(fn, x, y, s))
    for name, fn in paths.items():
        med = statistics.median(ts[name])
        say(f"  {name:6s} {med:10.1f} us / call [{min(ts[name]):.1f} .. {max(ts[name]):.1f}]   launches / call {launches(fn, x, y, s)}"
            f"   peak memory above the operands {peak_extra(fn, x, y, s):9.2f} MiB")
    return {name: statistics.median(v) for name, v in ts.items()}


say(f"# tools/bench_cliploss.py  {torch.cuda.get_device_name(0)}  torch {torch.__version__}  d = {a.dim}  scale = {SCALE}  forward + backward,"
    f" {a.reps} calls per window after {a.warmup}, median [min .. max] of {a.rounds} alternating windows")
for n in a.sizes:
    measure("symmetric", n, n, symmetric)
for i in range(0, len(a.local), 2):
    measure("local   ", a.local[i], a.local[i + 1], local)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
