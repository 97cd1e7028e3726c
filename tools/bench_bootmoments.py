"""R bootstrap resamples of the regression metrics three ways in one run: the fused call ops.bootstrap_moments (the two kernels of
csrc/bootmoments.hip: the per-unit sums, then the int32 x f64 product on the f64 MFMA) with the float64 host finish of
metrics.finish_regression_moments, the same product composed from ATen ops on the GPU (the per-sample terms, an index_add_ over the
units, ``mult.double() @ F``) with the same finish, and numpy on 16 CPU threads (the resamples dealt to a thread pool).

    python tools/bench_bootmoments.py [--out profiles/bootmoments_bench.txt]

C in {1, 5}, R = 1 000, n in {1 000, 10 000, 100 000}, sample level (U = n) and group level (U = n / 4 patients, 1 .. 7 samples each);
seeded targets at an offset of 1000, predictions that follow them loosely, the multiplicities of metrics.bootstrap_multiplicities.
Before anything is timed the three products are compared entry by entry within the inner-product bound of tests/bootmoments_ref.py
(each side within (U + s + 8) 2^-53 of sum mult |F|).  The fused call is the whole public op (checks, read-back, centre, operand
preparation, both kernels) plus the finish; the two kernels alone (the C entry points on prepared operands) are timed beside it.
The GPU paths take turns inside every repetition; a timed sample is a window of `inner` back-to-back calls that ends in a device
synchronise, `inner` chosen so that the window lasts about --window seconds; reported are milliseconds per call as the median over
--reps windows with the minimum and maximum, and the peak device memory a call holds above its operands.  numpy is timed per call,
--cpu-reps times."""
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
from octcubem_amd._lib import call, load   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 10000, 100000])
ap.add_argument("--columns", type=int, nargs="+", default=[1, 5])
ap.add_argument("--resamples", type=int, default=1000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--cpu-reps", type=int, default=3)
ap.add_argument("--cpu-threads", type=int, default=16)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls per timed sample")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bootmoments_bench.txt"))
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_bootmoments: needs an MI355X (a timing taken without one says nothing)")
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


def terms(xp, x, y, centre):
    """[n, C, 8] float64: the eight terms of every sample; ``xp`` is torch or numpy."""
    xd, yd = (x.double(), y.double()) if xp is torch else (x.astype(np.float64), y.astype(np.float64))
    p, q, e = xd - centre[0], yd - centre[1], yd - xd
    return xp.stack([xp.ones_like(p), p, q, p * p, q * q, p * q, e * e, xp.abs(e)], 2)


def aten_path(x, y, mult, unit, centre, n_tau):
    U = mult.shape[1]
    T = terms(torch, x, y, centre).reshape(x.shape[0], -1)
    F = T if unit is None else torch.zeros((U, T.shape[1]), dtype=torch.float64, device=x.device).index_add_(0, unit, T)
    D = mult.double() @ F
    return D, metrics.finish_regression_moments(D.reshape(mult.shape[0], -1, 8), centre, n_tau)


def numpy_path(x, y, mult, unit, centre, n_tau, pool, threads):
    U = mult.shape[1]
    T = terms(np, x, y, centre).reshape(x.shape[0], -1)
    if unit is None:
        F = T
    else:
        F = np.zeros((U, T.shape[1]))
        np.add.at(F, unit, T)
    D = np.empty((mult.shape[0], F.shape[1]))
    parts = [p for p in np.array_split(np.arange(mult.shape[0]), threads) if p.size]

    def work(rows):
        D[rows] = mult[rows].astype(np.float64) @ F

    list(pool.map(work, parts))
    return D, metrics.finish_regression_moments(D.reshape(mult.shape[0], -1, 8), centre, n_tau)


def fused_path(x, y, mult, unit, n_tau):
    raw = ops.bootstrap_moments(x, y, mult, unit)
    return raw, metrics.finish_regression_moments(raw["moments"], raw["centre"], n_tau)


say(f"# tools/bench_bootmoments.py  {torch.cuda.get_device_name(0)}  torch {torch.__version__}  R = {a.resamples}  reps {a.reps} "
    f"warm-up {a.warmup} window {a.window} s; numpy {np.__version__} on {a.cpu_threads} threads, {a.cpu_reps} calls")
say("# ms per call: median [min .. max]; the GPU paths alternate inside every repetition; peak = device memory above the operands")
pool = ThreadPoolExecutor(a.cpu_threads)
R = a.resamples
for C in a.columns:
    for n in a.sizes:
        for level in ("sample", "group"):
            rng = np.random.default_rng([n, C])
            y_h = (1000.0 + rng.normal(size=(n, C))).astype(np.float32)
            x_h = (y_h + 0.5 * rng.normal(size=(n, C))).astype(np.float32)
            if level == "sample":
                U, unit_h, unit, smax = n, None, None, 1
            else:
                U = max(1, n // 4)
                ids = np.repeat(np.arange(U), 1 + np.arange(U) % 7)[:n]
                unit_h = rng.permutation(np.concatenate([ids, rng.integers(0, U, n - ids.size)])).astype(np.int64)
                unit, smax = torch.from_numpy(unit_h).to(dev), int(np.bincount(unit_h).max())
            x, y = torch.from_numpy(x_h).to(dev), torch.from_numpy(y_h).to(dev)
            mult = metrics.bootstrap_multiplicities(R, U, 0, dev)
            mult_h = mult.cpu().numpy()
            n_tau = max(n, U)
            # ---- the same numbers?
            raw, fin = fused_path(x, y, mult, unit, n_tau)
            centre = raw["centre"]
            centre_h = centre.cpu().numpy()
            Df = raw["moments"].reshape(R, -1).cpu().numpy()
            scale = (mult.double() @ raw["unit_moments"].reshape(U, -1).abs()).cpu().numpy()
            tol = 2.0 * (U + smax + 8) * 2.0 ** -53 * scale
            for name, (D, other) in (("ATen", aten_path(x, y, mult, unit, centre, n_tau)),
                                     ("numpy", numpy_path(x_h, y_h, mult_h, unit_h, centre_h, n_tau, pool, a.cpu_threads))):
                D = D.cpu().numpy() if isinstance(D, torch.Tensor) else D
                assert (np.abs(D - Df) <= tol).all(), f"n = {n}, C = {C}, {level}: the fused product and {name} differ"
                assert all(np.array_equal(np.isnan(fin[k]), np.isnan(other[k])) for k in fin), f"{name}: other resamples are defined"
            defined = int((~np.isnan(fin["pearsonr"])).sum())
            say(f"C = {C}  n = {n}  {level} level (U = {U}): the three products agree within the inner-product bound; {defined} of {R * C} defined")
            # ---- prepared operands for the kernels alone
            cpad8 = (8 * C + 15) // 16 * 16
            if unit is None:
                order, start = torch.arange(n, dtype=torch.int32, device=dev), torch.arange(U + 1, dtype=torch.int32, device=dev)
            else:
                order = torch.sort(unit, stable=True).indices.to(torch.int32)
                start = torch.zeros(U + 1, dtype=torch.int32, device=dev)
                start[1:] = torch.cumsum(torch.bincount(unit, minlength=U), 0)
            F = torch.empty((U, cpad8), dtype=torch.float64, device=dev)
            D = torch.empty((R, cpad8), dtype=torch.float64, device=dev)
            ws = torch.empty(max(1, int(load().octmae_bootstrap_moments_ws(R, U, C))), dtype=torch.float64, device=dev)

            def kernels():
                call("octmae_unit_moments", x.data_ptr(), C, y.data_ptr(), C, 0, C, centre.data_ptr(), order.data_ptr(), start.data_ptr(),
                     F.data_ptr(), n, C, U, ops._stream())
                call("octmae_bootstrap_moments", mult.data_ptr(), F.data_ptr(), D.data_ptr(), ws.data_ptr(), R, U, C, ops._stream())

            paths = {"fused": lambda: fused_path(x, y, mult, unit, n_tau),
                     "aten": lambda: aten_path(x, y, mult, unit, centre, n_tau),
                     "kernels": kernels}
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
                numpy_path(x_h, y_h, mult_h, unit_h, centre_h, n_tau, pool, a.cpu_threads)
                tc.append((time.perf_counter() - t0) * 1e3)
            mf, ma, mk = statistics.median(ts["fused"]), statistics.median(ts["aten"]), statistics.median(ts["kernels"])
            say(f"  ops.bootstrap_moments + finish (whole call)  {fmt(ts['fused'])}   {inner['fused']} calls per window, peak {peak['fused'] / 2 ** 20:.1f} MiB")
            say(f"    of which the two kernels alone             {fmt(ts['kernels'])}   {inner['kernels']} calls per window, "
                f"{2.0 * R * U * cpad8 / (mk * 1e-3) / 1e9:.1f} GFLOP/s f64, {R * U * 4 / (mk * 1e-3) / 1e9:.1f} GB/s of mult (workspace "
                f"{ws.numel() * 8 / 2 ** 20:.1f} MiB)")
            say(f"  ATen: mult.double() @ F + finish             {fmt(ts['aten'])}   {inner['aten']} calls per window, peak {peak['aten'] / 2 ** 20:.1f} MiB")
            say(f"  numpy, {a.cpu_threads} threads + finish                  {fmt(tc)}")
            say(f"  ATen / fused: {ma / mf:.2f} x    numpy / fused: {statistics.median(tc) / mf:.1f} x")
            del x, y, mult, F, D, ws, order, start, raw, centre
            torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
