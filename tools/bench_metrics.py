"""AUROC and average precision of [n, C] scores three ways, in one run: the rank-count kernel plus its host finish (ops.rank_counts ->
metrics.binary_rank_metrics: exact integers, float64 finish), a sort-based composition of ATen ops on the same GPU (sort, gather, cumsum,
cummax in float64, one point per distinct score), and numpy on the CPU (tests/metrics_ref.py, one class per thread on --cpu-threads
threads; numpy's sort itself is single-threaded, so at most C threads work).

    python tools/bench_metrics.py [--out profiles/metrics_bench.txt]

n in {2 000, 20 000, 120 000} at C = 8, seeded float32 scores with random 0 / 1 labels, already on the GPU for the two GPU paths and in
host memory for numpy.  Per path and n: milliseconds per call as the median of --reps timed calls after --warmup untimed ones, with the
minimum and maximum; every call ends with its results on the host (so each is timed by a host clock around work that ends in a
synchronising copy).  The kernel alone is timed with device events as well, with its comparison rate (n * n * C pairs per second).  The
three paths must agree to 1e-9 before anything is timed.  The kernel is O(n^2 C) on purpose (exact, deterministic, no sort): where the
ATen sort is faster at large n this file says so."""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from octcubem_amd import metrics, ops      # noqa: E402
from tests import metrics_ref as R         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 20000, 120000])
ap.add_argument("--classes", type=int, default=8)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--cpu-reps", type=int, default=3)
ap.add_argument("--cpu-threads", type=int, default=16)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.txt"))
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_metrics: needs an MI355X (a timing taken without one says nothing)")
dev = torch.device("cuda")
torch.set_num_threads(a.cpu_threads)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def kernel_path(scores, labels):
    res = metrics.binary_rank_metrics(ops.rank_counts(scores, labels), labels)
    return res["roc_auc"], res["AP"]


def aten_path(scores, labels):
    """Per class: sort descending, cumulative true positives, one curve point at the last sample of every run of equal scores."""
    n = scores.shape[0]
    s, idx = torch.sort(scores, dim=0, descending=True)
    tp = torch.gather(labels, 0, idx).double().cumsum(0)
    k = torch.arange(1, n + 1, device=scores.device, dtype=torch.float64)[:, None]
    fp = k - tp
    last = torch.ones_like(s, dtype=torch.bool)
    last[:-1] = s[1:] != s[:-1]
    zero = torch.zeros_like(tp[:1])
    tp_prev = torch.cat([zero, torch.cummax(torch.where(last, tp, zero), 0).values[:-1]])      # tp at the previous point (tp never falls)
    fp_prev = torch.cat([zero, torch.cummax(torch.where(last, fp, zero), 0).values[:-1]])
    P, N = tp[-1], fp[-1]
    lastf = last.double()
    auroc = (lastf * (fp - fp_prev) * (tp + tp_prev) * 0.5).sum(0) / (P * N)
    ap_ = (lastf * (tp - tp_prev) * (tp / k)).sum(0) / P
    return auroc.cpu().numpy(), ap_.cpu().numpy()


def numpy_path(scores, labels, pool):
    cols = range(scores.shape[1])
    roc = list(pool.map(lambda c: R.auroc(scores[:, c], labels[:, c]), cols))
    ap_ = list(pool.map(lambda c: R.average_precision(scores[:, c], labels[:, c]), cols))
    return np.array(roc), np.array(ap_)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def kernel_only(scores, labels, reps, warmup):
    for _ in range(warmup):
        ops.rank_counts(scores, labels)
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        ops.rank_counts(scores, labels)          # includes the NaN check that precedes the launch
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


say(f"# tools/bench_metrics.py  {torch.cuda.get_device_name(0)}  torch {torch.__version__}  C = {a.classes}  reps {a.reps} warm-up {a.warmup}"
    f"  numpy: {a.cpu_reps} reps on {a.cpu_threads} threads")
say("# ms per call: median [min .. max]; every call ends with AUROC and AP of all classes on the host")
pool = ThreadPoolExecutor(a.cpu_threads)
for n in a.sizes:
    g = torch.Generator().manual_seed(n)
    scores_h = torch.rand(n, a.classes, generator=g)
    labels_h = (torch.rand(n, a.classes, generator=g) < 0.3).to(torch.uint8)
    scores, labels = scores_h.to(dev), labels_h.to(dev)
    sn, ln = scores_h.numpy(), labels_h.numpy()
    k_roc, k_ap = kernel_path(scores, labels)
    a_roc, a_ap = aten_path(scores, labels)
    c_roc, c_ap = numpy_path(sn, ln, pool)
    err = max(np.abs(k_roc - a_roc).max(), np.abs(k_ap - a_ap).max(), np.abs(k_roc - c_roc).max(), np.abs(k_ap - c_ap).max())
    assert err <= 1e-9, f"n = {n}: the three paths differ by {err:.3e}"
    say(f"n = {n}: the three paths agree to {err:.1e}")
    med, lo, hi = timed(lambda: kernel_path(scores, labels), a.reps, a.warmup)
    say(f"  rank_counts + host finish     {med:10.3f} [{lo:.3f} .. {hi:.3f}]")
    med, lo, hi = kernel_only(scores, labels, a.reps, a.warmup)
    say(f"    rank_counts alone (events)  {med:10.3f} [{lo:.3f} .. {hi:.3f}]   {n * n * a.classes / (med * 1e-3) / 1e12:.3f} T pairs/s")
    med, lo, hi = timed(lambda: aten_path(scores, labels), a.reps, a.warmup)
    say(f"  ATen sort composition (GPU)   {med:10.3f} [{lo:.3f} .. {hi:.3f}]")
    med, lo, hi = timed(lambda: numpy_path(sn, ln, pool), a.cpu_reps, 1)
    say(f"  numpy sort (CPU)              {med:10.3f} [{lo:.3f} .. {hi:.3f}]")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
