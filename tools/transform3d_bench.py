"""The volume transforms three ways, in one run: the fused gfx950 path (octcubem_amd.transforms: ops.volume_box + ops.volume_resample),
the same chain composed from ATen ops on the GPU (nonzero / amin / amax with their host synchronisation, slice, F.interpolate, flip,
where) and the torch CPU chain on 16 threads.

    python tools/transform3d_bench.py [--out profiles/transform3d_bench.txt]

Raw uint8 and float32 volumes of 61 x 496 x 512 -> 60 x 256 x 256, train (crop, resize, both flips, normalise) and val (resize,
normalise) pipelines, one volume at a time (the device synchronised after every volume: the latency a caller sees) and a batch of 32
(synchronised once per batch).  The 32 volumes are distinct and are cycled through, so that no volume waits in the Infinity Cache for its next use
(32 x 15.5 MB of uint8 is 496 MB, of float32 2 GB; the cache holds 256 MiB).

Per path and case: microseconds per volume as the median of --reps timed windows after --warmup untimed ones, with the windows' minimum
and maximum; the algorithmic bytes (the raw volume read twice for train -- box pass and resample pass -- and once for val, the output
written once) over that time as a fraction of the HBM rates of MI355X_MICROARCH.md (8.0 TB/s specified, 6.29 TB/s measured with a
float4 copy); and volumes/s beside the rate the headline pre-training step consumes (README status: 168-173 volumes/s per GPU)."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octcubem_amd import ops                                    # noqa: E402
from octcubem_amd.transforms import create_3d_transforms        # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", type=int, nargs=3, default=[61, 496, 512])
ap.add_argument("--size", type=int, nargs=3, default=[60, 256, 256])
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--cpu-reps", type=int, default=3)
ap.add_argument("--cpu-threads", type=int, default=16)
ap.add_argument("--headline-vps", type=float, default=170.0)
ap.add_argument("--out", default=None)
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("transform3d_bench: needs an MI355X (a timing taken without one says nothing)")
dev = torch.device("cuda")
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12
SIZE = tuple(a.size)
NORM = (0.25, 0.25)
CPU_VOLS = 4                    # volumes per CPU window
torch.set_num_threads(a.cpu_threads)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def make_pool(dtype):
    """--batch distinct raw volumes: uniform noise with x < 0.05 set to 0 and empty slabs at three faces (a box that is not the extent)."""
    g = torch.Generator().manual_seed(0)
    pool = []
    for _ in range(a.batch):
        x = torch.rand(1, *a.shape, generator=g)
        x[x < 0.05] = 0
        x[:, :1] = 0
        x[:, :, :40] = 0
        x[:, :, :, -30:] = 0
        pool.append((x * 255).to(torch.uint8) if dtype == torch.uint8 else x)
    return pool


# ---- the three chains; each takes one [1, D, H, W] volume and an output slice [T, OH, OW] ------------------------------------------
def fused(x, out, train):
    vol = x[0]
    ops.volume_resample(vol, SIZE, box=ops.volume_box(vol) if train else None, flip_d=train, flip_w=train, normalize=NORM, out=out)


def aten(x, out, train):
    v = x[0]
    if train:
        nz = (v > 0).nonzero()
        lo, hi = nz.amin(0).tolist(), (nz.amax(0) + 1).tolist()             # the host synchronisation of the composed form
        v = v[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    y = F.interpolate(v[None, None].float(), size=SIZE, mode="trilinear", align_corners=False)[0, 0]
    if train:
        y = y.flip(0).flip(2)
    out.copy_(torch.where(y != 0, (y - NORM[0]) / NORM[1], y))


def measure(chain, pool, out, train, batched, reps, warmup, gpu=True):
    """Median / min / max seconds per volume over windows of one pass through the pool.  single: the device is synchronised after
    every volume (the latency a caller of one transform sees); batch: once, after the last."""
    def run():
        if gpu:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, x in enumerate(pool):
            chain(x, out[i, 0], train)
            if gpu and not batched:
                torch.cuda.synchronize()
        if gpu:
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / len(pool)

    for _ in range(warmup):
        run()
    ts = [run() for _ in range(reps)]
    return statistics.median(ts), min(ts), max(ts)


def agree(pool, train):
    """Before anything is timed: the two GPU chains compute the same thing (relative to the input's range)."""
    o1 = torch.empty((1, 1, *SIZE), device=dev)
    o2 = torch.empty_like(o1)
    fused(pool[0], o1[0, 0], train)
    aten(pool[0], o2[0, 0], train)
    return float((o1 - o2).abs().max()) / float(pool[0].float().max())


say(f"# transform3d_bench: {tuple(a.shape)} -> {SIZE}, batch {a.batch}, {a.reps} timed windows after {a.warmup} warm-up "
    f"of {a.batch} volumes each, {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
say(f"# the cpu rows are a far smaller sample: {a.cpu_reps} timed windows after 1 warm-up of {CPU_VOLS} volumes each on {a.cpu_threads} threads; "
    "their spread is not comparable to the GPU rows'")
say("# us/vol = median over the windows [min .. max]; bytes = raw volume x (2 train | 1 val) + float32 output; "
    f"HBM: {HBM_SPEC / 1e12:.1f} TB/s specified, {HBM_COPY / 1e12:.2f} TB/s float4 copy")
say(f"# x step = volumes/s over the {a.headline_vps:.0f} volumes/s one GPU's headline pre-training step consumes")
hdr = f"{'dtype':8s}{'pipe':6s}{'mode':8s}{'path':12s}{'us/vol':>11s}{'[min':>11s}{'max]':>11s}{'GB/s':>9s}{'%spec':>7s}{'%copy':>7s}{'vol/s':>10s}{'x step':>8s}"
results = {}
for dtype in (torch.uint8, torch.float32):
    name = "uint8" if dtype == torch.uint8 else "float32"
    pool_cpu = make_pool(dtype)
    pool = [x.to(dev) for x in pool_cpu]
    out = torch.empty((a.batch, 1, *SIZE), device=dev)
    out_cpu = torch.empty((a.batch, 1, *SIZE))
    vol_bytes = pool[0].numel() * pool[0].element_size()
    out_bytes = 4 * SIZE[0] * SIZE[1] * SIZE[2]
    for train in (True, False):
        pipe = "train" if train else "val"
        say()
        say(f"# {name} {pipe}: max |fused - ATen| / max|x| = {agree(pool, train):.2e}")
        say(hdr)
        nbytes = vol_bytes * (2 if train else 1) + out_bytes
        for batched in (False, True):
            mode = f"batch{a.batch}" if batched else "single"
            # the two GPU paths alternate, fused first and last, so that a drift of the clocks shows as a difference between the two fused rows
            rows = [("fused", fused, pool, out, a.reps, a.warmup), ("aten-gpu", aten, pool, out, a.reps, a.warmup),
                    ("fused(2nd)", fused, pool, out, a.reps, a.warmup)]
            if not batched:
                rows.append((f"cpu-{a.cpu_threads}thr", aten, pool_cpu[:CPU_VOLS], out_cpu, a.cpu_reps, 1))
            for path, chain, pl, o, reps, warm in rows:
                med, lo, hi = measure(chain, pl, o, train, batched, reps, warm, gpu=not path.startswith("cpu"))
                results[(name, pipe, mode, path)] = med
                say(f"{name:8s}{pipe:6s}{mode:8s}{path:12s}{med * 1e6:11.1f}{lo * 1e6:11.1f}{hi * 1e6:11.1f}{nbytes / med / 1e9:9.1f}"
                    f"{100 * nbytes / med / HBM_SPEC:7.2f}{100 * nbytes / med / HBM_COPY:7.2f}{1 / med:10.0f}{1 / med / a.headline_vps:8.1f}")
    del pool, out

say()
say("# fused against the ATen composition (ratio of medians; > 1: the fused path is faster)")
slower = []
for (name, pipe, mode, path), med in results.items():
    if path == "aten-gpu":
        f = max(results[(name, pipe, mode, "fused")], results[(name, pipe, mode, "fused(2nd)")])
        say(f"{name:8s}{pipe:6s}{mode:8s} ATen / fused = {med / f:6.2f}")
        if med < f:
            slower.append((name, pipe, mode))
say("# the fused path is " + ("SLOWER than the ATen composition at: " + ", ".join("/".join(s) for s in slower) if slower
                               else "not slower than the ATen composition in any case"))

# the public interface on top of the raw ops: what create_3d_transforms' .batch() adds (host-side flip draws, shape checks)
train_t, val_t = create_3d_transforms(SIZE[1:], num_frames=SIZE[0], normalize=True, generator=torch.Generator().manual_seed(0))
pool = [x.to(dev) for x in make_pool(torch.uint8)]
for t, pipe in ((train_t, "train"), (val_t, "val")):
    ts = []
    for r in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t.batch(pool)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / len(pool))
    ts = ts[a.warmup:]
    say(f"# create_3d_transforms(...).batch, uint8 {pipe}: {statistics.median(ts) * 1e6:.1f} us/vol [{min(ts) * 1e6:.1f} .. {max(ts) * 1e6:.1f}]")

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
