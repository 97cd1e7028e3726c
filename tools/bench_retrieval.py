"""The ten retrieval metrics of the COEM validation (coem.get_metrics) three ways, in one run: the fused similarity-rank kernel plus its
host finish (ops.retrieval_ranks, csrc/retrieval.hip: no [N, N] matrix), matmul + argsort composed from ATen ops on the same GPU (where
the [N, N] float32 matrix and its int64 argsort fit), and the reference's way with torch on the CPU (--cpu-threads threads: matmul,
argsort of every row, where(ranking == ground_truth), both directions).

    python tools/bench_retrieval.py [--out profiles/retrieval_bench.txt]

D = 512, N in {2 000, 20 000}; seeded normalised features, text = normalize(0.1 image + unit noise), already on the GPU for the two GPU
paths and in host memory for the CPU path.  Per path and N: milliseconds per call as the median of --reps timed calls after --warmup
untimed ones, with the minimum and maximum; every call ends with the metrics on the host.  The kernel alone is timed with device events as
well, with its rate (2 N N D flop per direction).  The three paths are checked against each other before anything is timed: they round the
scores differently (f32 fmaf chain, the GPU's f32 GEMM, the CPU's), so a candidate within rounding of the partner may change places:
R@k and the median must agree to 1e-3, the mean rank to 1e-3 relative."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from octcubem_amd import coem, ops      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 20000])
ap.add_argument("--dim", type=int, default=512)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--cpu-reps", type=int, default=2)
ap.add_argument("--cpu-threads", type=int, default=16)
ap.add_argument("--aten-max-n", type=int, default=20000, help="largest N at which the ATen composition forms the [N, N] matrix")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_bench.txt"))
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_retrieval: needs an MI355X (a timing taken without one says nothing)")
dev = torch.device("cuda")
torch.set_num_threads(a.cpu_threads)
lines = []
SCALE = 1 / 0.07


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def sorted_path(img, txt):
    """the reference's get_metrics on whatever device the features are on"""
    out = {}
    logits = SCALE * img @ txt.t()
    gt = torch.arange(len(txt), device=img.device).view(-1, 1)
    for name, lg in (("image_to_text", logits), ("text_to_image", logits.t())):
        preds = torch.where(torch.argsort(lg, descending=True) == gt)[1].cpu().numpy()
        out[f"{name}_mean_rank"] = preds.mean() + 1
        out[f"{name}_median_rank"] = np.floor(np.median(preds)) + 1
        for k in (1, 5, 10):
            out[f"{name}_R@{k}"] = np.mean(preds < k)
    return out


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


def kernel_only(img, txt, reps, warmup):
    for _ in range(warmup):
        ops.retrieval_ranks(img, txt)
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        ops.retrieval_ranks(img, txt)              # one direction; includes the finiteness check that precedes the launch
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def differ(x, y):
    worst = 0.0
    for k in x:
        d = abs(x[k] - y[k]) / (abs(y[k]) if k.endswith("mean_rank") else 1.0)
        worst = max(worst, d)
    return worst


say(f"# tools/bench_retrieval.py  {torch.cuda.get_device_name(0)}  torch {torch.__version__}  D = {a.dim}  reps {a.reps} warm-up {a.warmup}"
    f"  CPU: {a.cpu_reps} reps on {a.cpu_threads} threads")
say("# ms per call: median [min .. max]; every call ends with the ten metrics of both directions on the host")
for n in a.sizes:
    g = torch.Generator().manual_seed(n)
    img_h = torch.nn.functional.normalize(torch.randn(n, a.dim, generator=g), dim=-1)
    txt_h = torch.nn.functional.normalize(0.1 * img_h + torch.nn.functional.normalize(torch.randn(n, a.dim, generator=g), dim=-1), dim=-1)
    img, txt = img_h.to(dev), txt_h.to(dev)
    k_res = coem.get_metrics(img, txt, SCALE)
    c_res = sorted_path(img_h, txt_h)
    aten = n <= a.aten_max_n
    err = differ(k_res, c_res)
    if aten:
        err = max(err, differ(sorted_path(img, txt), c_res))
    assert err <= 1e-3, f"N = {n}: the paths differ by {err:.3e}"
    say(f"N = {n}: the paths agree to {err:.1e}   (R@1 {k_res['image_to_text_R@1']:.4f}, mean rank {k_res['image_to_text_mean_rank']:.2f})")
    med, lo, hi = timed(lambda: coem.get_metrics(img, txt, SCALE), a.reps, a.warmup)
    say(f"  retrieval_ranks x 2 + host finish   {med:10.3f} [{lo:.3f} .. {hi:.3f}]")
    med, lo, hi = kernel_only(img, txt, a.reps, a.warmup)
    say(f"    retrieval_ranks alone (events)    {med:10.3f} [{lo:.3f} .. {hi:.3f}]   {2.0 * n * n * a.dim / (med * 1e-3) / 1e12:.2f} TFLOP/s")
    if aten:
        med, lo, hi = timed(lambda: sorted_path(img, txt), a.reps, a.warmup)
        say(f"  ATen matmul + argsort (GPU)         {med:10.3f} [{lo:.3f} .. {hi:.3f}]")
    else:
        say(f"  ATen matmul + argsort (GPU)         not run: the [N, N] matrix is above --aten-max-n")
    med, lo, hi = timed(lambda: sorted_path(img_h, txt_h), a.cpu_reps, 1)
    say(f"  torch matmul + argsort (CPU)        {med:10.3f} [{lo:.3f} .. {hi:.3f}]")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
