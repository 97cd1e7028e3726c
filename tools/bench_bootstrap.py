"""R bootstrap resamples of the four ranking metrics three ways in one run: the fused call ops.bootstrap_rank_metrics (one sort, then
csrc/bootstrap.hip walks every resample), the same six quantities composed from ATen ops on the GPU (per class: a gather of the
multiplicities along the sorted order, two batched cumsums over [R, n], an index_select at the tie-group ends, masked reductions), and
the same composition in numpy on 16 CPU threads (the resamples dealt to a thread pool).

    python tools/bench_bootstrap.py [--out profiles/bootstrap_bench.txt]

n in {1 000, 10 000, 100 000}, C = 5, R = 1 000; seeded scores on a grid of 4096 values (ties), 10 % positives, the multiplicities of
metrics.bootstrap_multiplicities.  Before anything is timed the three results are compared: P, N, U2 equal, the floats within the
derived bounds of tests/bootstrap_ref.py.  The fused call is the whole public op (checks, read-back, sort, operand preparation,
kernel); the sort alone and the kernel alone (the C entry point on prepared operands) are timed beside it.  The GPU paths take turns
inside every repetition; a timed sample is a window of `inner` back-to-back calls that ends in a device synchronise, `inner` chosen so
that the window lasts about --window seconds; reported are milliseconds per call as the median over --reps windows with the minimum
and maximum, and the peak device memory a call holds above its operands.  numpy is timed per call, --cpu-reps times."""
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
from octcubem_amd._lib import call         # noqa: E402
from tests import bootstrap_ref as B       # noqa: E402  (the derived bounds)

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 10000, 100000])
ap.add_argument("--classes", type=int, default=5)
ap.add_argument("--resamples", type=int, default=1000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--cpu-reps", type=int, default=3)
ap.add_argument("--cpu-threads", type=int, default=16)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls per timed sample")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bootstrap_bench.txt"))
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_bootstrap: needs an MI355X (a timing taken without one says nothing)")
dev = torch.device("cuda")
lines = []
KEYS = ("P", "N", "U2", "ap_sum", "auprc", "max_f1")


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


def finish_groups(xp, TP, ALL, P, N):
    """The six quantities from the cumulative pairs at the tie-group ends, [R, G] each; ``xp`` is torch or numpy."""
    zero, cat = xp.zeros_like(TP[:, :1]), np.concatenate if xp is np else torch.cat
    pTP, pALL = cat([zero, TP[:, :-1]], 1), cat([zero, ALL[:, :-1]], 1)
    posw = TP - pTP
    negw = (ALL - pALL) - posw
    U2 = (posw * (2 * (N - (ALL - TP)) + negw)).sum(1)
    f = (lambda t: t.astype(np.float64)) if xp is np else (lambda t: t.double())
    one = 1.0 if xp is np else torch.ones((), dtype=torch.float64, device=TP.device)
    prec = xp.where(ALL > 0, f(TP) / f(xp.where(ALL > 0, ALL, 1)), one)
    pprec = xp.where(pALL > 0, f(pTP) / f(xp.where(pALL > 0, pALL, 1)), one)
    Pd = f(xp.where(P > 0, P, 1))
    rec = f(TP) / Pd
    ap_sum = (f(posw) * prec).sum(1)
    area = ((f(posw) / Pd) * (prec + pprec) * 0.5).sum(1)
    f1 = (2 * prec * rec / (prec + rec + 1e-8)).max(1)
    f1 = f1 if xp is np else f1.values
    return P[:, 0], N[:, 0], U2, ap_sum, area, f1


def aten_path(scores, labels, mult):
    vals, order = torch.sort(scores, dim=0, descending=True, stable=True)
    out = [[] for _ in KEYS]
    for c in range(scores.shape[1]):
        idx = order[:, c]
        end = torch.ones(vals.shape[0], dtype=torch.bool, device=vals.device)
        end[:-1] = vals[:-1, c] != vals[1:, c]
        ends = end.nonzero().squeeze(1)
        W = mult.index_select(1, idx).long()
        ALL = W.cumsum(1)
        TP = (W * labels[idx, c].long()).cumsum(1)
        P, N = TP[:, -1:], ALL[:, -1:] - TP[:, -1:]
        for o, v in zip(out, finish_groups(torch, TP.index_select(1, ends), ALL.index_select(1, ends), P, N)):
            o.append(v)
    return {k: torch.stack(o, 1) for k, o in zip(KEYS, out)}


def numpy_path(scores, labels, mult, pool, threads):
    R, C = mult.shape[0], scores.shape[1]
    out = {k: np.zeros((R, C), dtype=np.int64 if k in KEYS[:3] else np.float64) for k in KEYS}
    parts = [p for p in np.array_split(np.arange(R), threads) if p.size]
    for c in range(C):
        idx = np.argsort(-scores[:, c], kind="stable")
        v, lab = scores[idx, c], labels[idx, c].astype(np.int64)
        ends = np.nonzero(np.r_[v[1:] != v[:-1], True])[0]

        def work(rows):
            W = mult[rows][:, idx].astype(np.int64)
            ALL, TP = W.cumsum(1), (W * lab).cumsum(1)
            res = finish_groups(np, TP[:, ends], ALL[:, ends], TP[:, -1:], ALL[:, -1:] - TP[:, -1:])
            for k, x in zip(KEYS, res):
                out[k][rows, c] = x

        list(pool.map(work, parts))
    return out


say(f"# tools/bench_bootstrap.py  {torch.cuda.get_device_name(0)}  torch {torch.__version__}  C = {a.classes}  R = {a.resamples}  reps {a.reps} "
    f"warm-up {a.warmup} window {a.window} s; numpy {np.__version__} on {a.cpu_threads} threads, {a.cpu_reps} calls")
say("# ms per call: median [min .. max]; the GPU paths alternate inside every repetition; peak = device memory above the operands")
pool = ThreadPoolExecutor(a.cpu_threads)
C, R = a.classes, a.resamples
for n in a.sizes:
    rng = np.random.default_rng(n)
    lab_h = (rng.random((n, C)) < 0.1).astype(np.uint8)
    s_h = (np.round((0.35 * lab_h + rng.random((n, C))) * 4096) / 4096).astype(np.float32)
    scores, labels = torch.from_numpy(s_h).to(dev), torch.from_numpy(lab_h).to(dev)
    mult = metrics.bootstrap_multiplicities(R, n, 0, dev)
    mult_h = mult.cpu().numpy()
    # ---- the same numbers?
    fused = {k: v.cpu().numpy() for k, v in ops.bootstrap_rank_metrics(scores, labels, mult).items()}
    for name, other in (("ATen", {k: v.cpu().numpy() for k, v in aten_path(scores, labels, mult).items()}),
                        ("numpy", numpy_path(s_h, lab_h, mult_h, pool, a.cpu_threads))):
        bad = B.mismatches(fused, other, n)
        assert not bad, f"n = {n}: the fused call and {name} differ: {bad[:3]}"
    defined = int(((fused["P"] > 0) & (fused["N"] > 0)).sum())
    say(f"n = {n}: the three results agree (integers equal, floats within the derived bounds); {defined} of {R * C} pairs defined")
    # ---- prepared operands for the kernel alone
    vals, order = torch.sort(scores, dim=0, descending=True, stable=True)
    end = torch.ones((n, C), dtype=torch.bool, device=dev)
    end[:-1] = vals[:-1] != vals[1:]
    flags = (torch.gather(labels, 0, order) | (end.to(torch.uint8) << 1) | 4).t().contiguous()
    unit_sorted = order.to(torch.int32).t().contiguous()
    outs = [torch.empty((R, C), dtype=torch.int64 if k in KEYS[:3] else torch.float64, device=dev) for k in KEYS]
    del vals, order, end
    paths = {"fused": lambda: ops.bootstrap_rank_metrics(scores, labels, mult),
             "aten": lambda: aten_path(scores, labels, mult),
             "sort": lambda: torch.sort(scores, dim=0, descending=True, stable=True),
             "kernel": lambda: call("octmae_bootstrap_rank_metrics", unit_sorted.data_ptr(), flags.data_ptr(), mult.data_ptr(),
                                    *(o.data_ptr() for o in outs), n, C, R, n, ops._stream())}
    inner, peak = {}, {}
    for name, fn in paths.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t1 = window(fn, 1)
        peak[name] = torch.cuda.max_memory_allocated() - base
        inner[name] = max(1, min(500, int(a.window * 1e3 / max(t1, 1e-3))))
    ts = {name: [] for name in paths}
    for r in range(a.reps):
        for name, fn in paths.items():
            ts[name].append(window(fn, inner[name]))
    tc = []
    for r in range(a.cpu_reps):
        t0 = time.perf_counter()
        numpy_path(s_h, lab_h, mult_h, pool, a.cpu_threads)
        tc.append((time.perf_counter() - t0) * 1e3)
    mf, ma = statistics.median(ts["fused"]), statistics.median(ts["aten"])
    say(f"  ops.bootstrap_rank_metrics (whole call)  {fmt(ts['fused'])}   {inner['fused']} calls per window, peak {peak['fused'] / 2 ** 20:.1f} MiB")
    say(f"    of which torch.sort alone              {fmt(ts['sort'])}   {inner['sort']} calls per window")
    say(f"    of which the kernel alone              {fmt(ts['kernel'])}   {inner['kernel']} calls per window, "
        f"{2.0 * R * C * n / (statistics.median(ts['kernel']) * 1e-3) / 1e9:.1f} G weighted positions/s (two passes)")
    say(f"  ATen composition on the GPU              {fmt(ts['aten'])}   {inner['aten']} calls per window, peak {peak['aten'] / 2 ** 20:.1f} MiB")
    say(f"  numpy, {a.cpu_threads} threads                        {fmt(tc)}")
    say(f"  ATen / fused: {ma / mf:.2f} x    numpy / fused: {statistics.median(tc) / mf:.1f} x")
    del scores, labels, mult, flags, unit_sorted, outs
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
