"""The six directions of get_metrics_3modalities two ways in one run: one P = 3 launch of ops.retrieval_pair_ranks
(csrc/retrieval_pair.hip: each of the three products walked once, rows and columns counted together, plus its diagonal pre-pass) against
the six launches of ops.retrieval_ranks it replaces (every product walked twice).

    python tools/bench_pair_ranks.py [--out profiles/pair_ranks_bench.txt]

D = 512, N in {1 024, 3 000, 16 384}; seeded unit-norm features, text1 / text2 = normalize(0.1 image + unit noise).  Both paths are whole
calls of the public ops, host checks and the finiteness read-back included (what coem.get_metrics_3modalities pays).  Before anything is
timed the counts are compared and must be EQUAL.  The two paths take turns inside every repetition.  A timed sample is a window of
`inner` back-to-back calls that ends in a device synchronise, `inner` chosen so that the window lasts about --window seconds; reported
are milliseconds per call as the median over --reps windows with the minimum and maximum, the pair kernel's workspace in bytes, and the
ratio of the medians.  coem.PAIR_RANKS_DEFAULT is True only if the one launch is not slower at N = 3 000."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from octcubem_amd import ops      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 3000, 16384])
ap.add_argument("--dim", type=int, default=512)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls per timed sample")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_ranks_bench.txt"))
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_pair_ranks: needs an MI355X (a timing taken without one says nothing)")
dev = torch.device("cuda")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def window(fn, inner):
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def fmt(ts):
    return f"{statistics.median(ts):10.3f} [{min(ts):.3f} .. {max(ts):.3f}]"


say(f"# tools/bench_pair_ranks.py  {torch.cuda.get_device_name(0)}  torch {torch.__version__}  D = {a.dim}  reps {a.reps} warm-up {a.warmup} "
    f"window {a.window} s")
say("# ms per call: median [min .. max] over the windows; the two paths alternate inside every repetition")
unit = lambda x: torch.nn.functional.normalize(x, dim=-1)
for n in a.sizes:
    gen = torch.Generator().manual_seed(n)
    img_h = unit(torch.randn(n, a.dim, generator=gen))
    img, t1, t2 = (x.to(dev) for x in (img_h, unit(0.1 * img_h + unit(torch.randn(n, a.dim, generator=gen))),
                                       unit(0.1 * img_h + unit(torch.randn(n, a.dim, generator=gen)))))
    products = [(img, t1), (img, t2), (t1, t2)]
    paths = {"pair": lambda: ops.retrieval_pair_ranks(products),
             "six": lambda: [ops.retrieval_ranks(x, y) for p in products for x, y in (p, p[::-1])]}
    # ---- the same counts?
    one, six = paths["pair"](), paths["six"]()
    for p in range(3):
        for k in (0, 1):
            assert torch.equal(one[p, k], six[2 * p + k][:, :2]), f"N = {n}: pair {p}, direction {k} differs"
    r1 = float(((one[0, 0].sum(dim=1)) < 1).float().mean())
    say(f"N = {n}: the {one.numel()} counts are equal; image-to-text1 R@1 {r1:.3f}; workspace {int(ops.load().octmae_retrieval_pair_ws(n, 3))} bytes")
    del one, six
    # ---- time: warm up, size the windows, alternate
    inner = {}
    for name, fn in paths.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        inner[name] = max(1, min(500, int(a.window * 1e3 / max(window(fn, 1), 1e-3))))
    ts = {name: [] for name in paths}
    for r in range(a.reps):
        for name, fn in paths.items():
            ts[name].append(window(fn, inner[name]))
    mp, ms = statistics.median(ts["pair"]), statistics.median(ts["six"])
    say(f"  one retrieval_pair_ranks, P = 3     {fmt(ts['pair'])}   {inner['pair']} calls per window, "
        f"{6.0 * n * n * a.dim / (mp * 1e-3) / 1e12:.2f} TFLOP/s over the whole call")
    say(f"  six retrieval_ranks                 {fmt(ts['six'])}   {inner['six']} calls per window, "
        f"{12.0 * n * n * a.dim / (ms * 1e-3) / 1e12:.2f} TFLOP/s over the whole calls")
    say(f"  six / one: {ms / mp:.2f} x")
    del img, t1, t2, products
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
