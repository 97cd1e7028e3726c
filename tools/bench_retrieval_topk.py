"""Top-k cross-modal retrieval with the query's own group excluded, three ways in one run: the fused kernel (ops.retrieval_topk,
csrc/retrieval_topk.hip: lists kept on the chip, plus the merge launch where the column tiles are split), the composition from ATen ops on
the same GPU (a @ b.T, the same-group columns overwritten, torch.topk -- in row chunks where the [N, N] float32 matrix would pass
--chunk-bytes), and the same composition with torch on the CPU (--cpu-threads threads; the reference script's way).  For scale, ops.retrieval_ranks on the
same operands takes its turn too: the same tile walk with four counters per row in place of the lists.

    python tools/bench_retrieval_topk.py [--out profiles/retrieval_topk_bench.txt]

D = 512, k = 10, N = M in {1 024, 3 000, 16 384, 65 536}; seeded unit-norm features, text = normalize(0.1 image + unit noise), groups of
four consecutive samples (a patient with four scans).  The three paths take turns inside every repetition.  A timed sample is a window
of `inner` back-to-back calls that ends in a device synchronise, `inner` chosen so that the window lasts about --window seconds; reported
are milliseconds per call as the median over --reps windows with the minimum and maximum.  Peak memory is what the path holds on the
device above the operands (torch's allocator statistics: outputs, workspace and temporaries, the finiteness check's included); for the
CPU path it is the size of one chunk's logits and mask, computed from the shapes.  Before anything is timed the lists are compared:
the paths round the scores differently (f32 fmaf chain, the GPU's f32 GEMM, the CPU's), so slots within rounding of each other may
change places; the share of equal indices and the largest score difference are printed, and 99 % / 1e-5 are asserted."""
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
ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 3000, 16384, 65536])
ap.add_argument("--dim", type=int, default=512)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls per timed sample (GPU paths)")
ap.add_argument("--cpu-reps", type=int, default=2)
ap.add_argument("--cpu-threads", type=int, default=16)
ap.add_argument("--cpu-max-n", type=int, default=65536, help="largest N at which the CPU path runs")
ap.add_argument("--chunk-bytes", type=int, default=2 ** 30, help="largest logits chunk of the ATen and CPU compositions")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_topk_bench.txt"))
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_retrieval_topk: needs an MI355X (a timing taken without one says nothing)")
dev = torch.device("cuda")
torch.set_num_threads(a.cpu_threads)
lines = []
MASKED = -1e5      # the reference script's value for an excluded column


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def chunk_rows(n, m):
    return max(1, min(n, a.chunk_bytes // (4 * m)))


def composed(q, g, grp, k):
    """matmul, mask, topk on whatever device the features are on; row chunks of at most --chunk-bytes of logits"""
    rows = chunk_rows(q.shape[0], g.shape[0])
    idx, score = [], []
    for r0 in range(0, q.shape[0], rows):
        logits = q[r0:r0 + rows] @ g.t()
        logits.masked_fill_(grp[r0:r0 + rows, None] == grp[None, :], MASKED)
        s, i = torch.topk(logits, k, dim=1)
        idx.append(i)
        score.append(s)
    return torch.cat(idx), torch.cat(score)


def fused(q, g, grp, k):
    return ops.retrieval_topk(q, g, k, row_group=grp, col_group=grp)


def window(fn, inner):
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def peak_above_operands(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def fmt(ts):
    return f"{statistics.median(ts):10.3f} [{min(ts):.3f} .. {max(ts):.3f}]"


def mib(b):
    return f"{b / 2 ** 20:10.1f} MiB"


say(f"# tools/bench_retrieval_topk.py  {torch.cuda.get_device_name(0)}  torch {torch.__version__}  D = {a.dim}  k = {a.k}  "
    f"reps {a.reps} warm-up {a.warmup} window {a.window} s  CPU: {a.cpu_reps} reps on {a.cpu_threads} threads")
say("# ms per call: median [min .. max] over the windows; the paths alternate inside every repetition; peak = device memory above the operands")
for n in a.sizes:
    gen = torch.Generator().manual_seed(n)
    img_h = torch.nn.functional.normalize(torch.randn(n, a.dim, generator=gen), dim=-1)
    txt_h = torch.nn.functional.normalize(0.1 * img_h + torch.nn.functional.normalize(torch.randn(n, a.dim, generator=gen), dim=-1), dim=-1)
    grp_h = (torch.arange(n) // 4).to(torch.int32)
    img, txt, grp = img_h.to(dev), txt_h.to(dev), grp_h.to(dev)
    cpu = n <= a.cpu_max_n
    # "ranks": ops.retrieval_ranks on the same operands -- the same tile walk with four counters per row in place of the lists, for scale
    paths = {"fused": lambda: fused(img, txt, grp, a.k), "aten": lambda: composed(img, txt, grp, a.k),
             "ranks": lambda: ops.retrieval_ranks(img, txt, row_group=grp, col_group=grp)}
    # ---- the same lists?
    fi, fs = paths["fused"]()
    ai, as_ = paths["aten"]()
    same = float((fi.long() == ai).float().mean())
    err = float((fs - as_).abs().max())
    assert int((fi < 0).sum()) == 0 and same >= 0.99 and err <= 1e-5, f"N = {n}: {same:.5f} of the indices agree, scores differ by {err:.2e}"
    say(f"N = {n}: fused and ATen lists: {100 * same:.3f} % of the indices equal, largest score difference {err:.1e}; split "
        f"{'yes' if ops.load().octmae_retrieval_topk_ws(n, n, a.k) else 'no'}, ATen row chunk {chunk_rows(n, n)}")
    del fi, fs, ai, as_
    # ---- memory
    mem = {name: peak_above_operands(fn) for name, fn in paths.items()}
    # ---- time: warm up, size the windows, alternate
    inner = {}
    for name, fn in paths.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        inner[name] = max(1, min(500, int(a.window * 1e3 / max(window(fn, 1), 1e-3))))
    ts = {name: [] for name in paths}
    cpu_ts = []
    for r in range(a.reps):
        for name, fn in paths.items():
            ts[name].append(window(fn, inner[name]))
        if cpu and r < a.cpu_reps:
            t0 = time.perf_counter()
            composed(img_h, txt_h, grp_h, a.k)
            cpu_ts.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median(ts["fused"])
    say(f"  fused retrieval_topk (+ merge)      {fmt(ts['fused'])}   peak {mib(mem['fused'])}   {inner['fused']} calls per window, "
        f"{2.0 * n * n * a.dim / (med * 1e-3) / 1e12:.2f} TFLOP/s over the whole call")
    say(f"  ATen matmul + mask + topk (GPU)     {fmt(ts['aten'])}   peak {mib(mem['aten'])}   {inner['aten']} calls per window")
    say(f"  (retrieval_ranks, the same walk)    {fmt(ts['ranks'])}   peak {mib(mem['ranks'])}   {inner['ranks']} calls per window")
    if cpu:
        rows = chunk_rows(n, n)
        say(f"  torch matmul + mask + topk (CPU)    {fmt(cpu_ts)}   chunk {mib(rows * n * 5)} (logits and mask of {rows} rows, from the shapes)")
    else:
        say("  torch matmul + mask + topk (CPU)    not run: N is above --cpu-max-n")
    say(f"  fused / ATen: {med / statistics.median(ts['aten']):.2f} x the time, {mem['fused'] / max(mem['aten'], 1):.4f} x the memory")
    del img, txt, grp
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
