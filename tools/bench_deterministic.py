"""What deterministic mode (ops.set_deterministic, include/octmae.h: "deterministic") costs, default against deterministic in one
process:

    python tools/bench_deterministic.py [--out profiles/deterministic_bench.txt]

(a) the ViT-L pre-training step (models_mae.octcube_vit_large_3dmae, 75 % masking: forward, backward, gradient norm with clipping,
    fused AdamW) at --batches volumes per micro-batch (default 1, 4, 32 and the headline's 128);
(b) the four weight gradients of a ViT-L encoder Block alone -- the qkv + proj and the fc1 + fc2 pair, with their bias gradients, as
    ops.linear_wgrad_accum_pair issues them -- at the same volume counts (1281 rows per volume).
Per case: milliseconds from device events around --reps repetitions, median [min .. max] of --rounds windows with the two modes
ALTERNATING (a drift of the box hits both); x = deterministic / default of this run.  Before anything is timed the gradient arena of
two deterministic steps from the same state is compared bit for bit, and two default steps by their relative L2 distance -- the
1e-8 ... 4e-8 the mode removes.  "slabs" is what the k slices of the case's weight gradients park in the stream's split-K workspace
(the 64 MiB ops.py lends anyway: the mode allocates nothing but 4 bytes per 65536-element chunk for the gradient norm).
The tool writes its own output file and nothing else: the ratios quoted in README.md, INTEGRATION.md and DESIGN.md are copied from
that file by hand."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from octcubem_amd import misc, models_mae, ops, optim as foptim      # noqa: E402
from octcubem_amd._lib import load      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 32, 128])
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--wgrad-reps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--cases", nargs="+", default=["step", "wgrad"], choices=["step", "wgrad"])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deterministic_bench.txt"))
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_deterministic: needs an MI355X (a timing taken without one says nothing)")
dev = torch.device("cuda")
lib = load()
CUS = torch.cuda.get_device_properties(0).multi_processor_count
WS = lib.octmae_gemm_split_ws_kib() * 1024
MODES = (("default", False), ("deterministic", True))
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
    return e0.elapsed_time(e1) / reps


def in_mode(flag, fn):
    def run():
        prev = ops.set_deterministic(flag)
        try:
            return fn()
        finally:
            ops.set_deterministic(prev)
    return run


def pair_slices(first, second, M, det):
    """(k slices, slab bytes) of the pair's launch in the given mode"""
    out = (ctypes.c_int * 14)()
    prev = ops.set_deterministic(det)
    try:
        rc = lib.octmae_wgrad_pair_plan_ws(first[0], first[1], first[0], first[1], second[0], second[1], second[0], second[1], M, 0, WS, CUS, out)
    finally:
        ops.set_deterministic(prev)
    assert rc == 0, rc
    return out[2], (out[2] * (first[0] * first[1] + second[0] * second[1]) * 4 if det and out[5] == 3 else 0)


def timed(title, paths, reps, note=""):
    for fn in paths.values():
        for _ in range(a.warmup):
            fn()
    ts = {name: [] for name in paths}
    for _ in range(a.rounds):
        for name, fn in paths.items():
            ts[name].append(window(fn, reps))
    t0 = statistics.median(ts["default"])
    for name in paths:
        t = statistics.median(ts[name])
        say(f"  {title:34s} {name:13s} {t:10.3f} ms [{min(ts[name]):.3f} .. {max(ts[name]):.3f}]  x{t / t0:.3f}{note if name == 'deterministic' else ''}")


say(f"# tools/bench_deterministic.py  {torch.cuda.get_device_name(0)}  torch {torch.__version__}  operands {ops.BF16}  {CUS} CUs;  median "
    f"[min .. max] of {a.rounds} alternating windows after {a.warmup} warm-up per mode; x = deterministic / default of this run")

C, H = 1024, 4096
QKV, PROJ, FC1, FC2 = (3 * C, C), (C, C), (H, C), (C, H)

if "step" in a.cases:
    say("## (a) ViT-L 3-D MAE pre-training step: forward + backward + gradient norm (clip 1.0) + fused AdamW")
    torch.manual_seed(0)
    mae = models_mae.octcube_vit_large_3dmae().to(dev).train()
    opt = foptim.FusedAdamW(misc.add_weight_decay(mae, 0.05), lr=1e-4, betas=(0.9, 0.95))
    scaler = misc.NativeScalerWithGradNormCount(fp32=True)
    params = list(mae.parameters())
    for B in a.batches:
        try:
            vol = torch.randn(B, 1, 60, 256, 256, device=dev)
            noise = torch.rand(B, 20 * 16 * 16, device=dev)

            def backward_only():
                mae.arena.zero_grad()
                loss, _, _ = mae(vol, mask_ratio=0.75, noise=noise)
                loss.backward()
                return loss

            def step():
                opt.zero_grad()
                loss, _, _ = mae(vol, mask_ratio=0.75, noise=noise)
                scaler(loss, opt, parameters=params, clip_grad=1.0)

            with torch.no_grad():
                mae(vol, mask_ratio=0.75, noise=noise)      # binds the arena, warms the allocator
            for name, flag in MODES:
                runs = []
                for _ in range(2):
                    loss = in_mode(flag, backward_only)()
                    runs.append((loss.detach().clone(), mae.arena.grad.clone()))
                torch.cuda.synchronize()
                gn = float(runs[0][1].double().norm())
                d = float((runs[1][1].double() - runs[0][1].double()).norm()) / gn
                same = torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
                say(f"  B = {B:3d}  {name:13s} two backwards from one state: gradient arena {'BIT-EQUAL' if same else f'DIFFERS, rel L2 {d:.1e}'}")
                del runs
            rows = B * 1281
            slabs = [pair_slices(QKV, PROJ, rows, True), pair_slices(FC1, FC2, rows, True)]
            dflt = [pair_slices(QKV, PROJ, rows, False)[0], pair_slices(FC1, FC2, rows, False)[0]]
            note = (f"   encoder pairs: k slices {dflt[0]} / {dflt[1]} -> {slabs[0][0]} / {slabs[1][0]}, slabs "
                    f"{slabs[0][1] / 2 ** 20:.0f} / {slabs[1][1] / 2 ** 20:.0f} MiB of the lent {WS / 2 ** 20:.0f} MiB")
            timed(f"B = {B:3d}  step", {name: in_mode(flag, step) for name, flag in MODES}, a.reps, note)
            del vol, noise
        except torch.cuda.OutOfMemoryError:
            say(f"  B = {B:3d}  does not fit this device's memory beside the optimizer state: NOT MEASURED")
        torch.cuda.empty_cache()
    del mae, opt, scaler, params
    torch.cuda.empty_cache()

if "wgrad" in a.cases:
    say("## (b) the weight gradients of one ViT-L encoder Block alone (two ops.linear_wgrad_accum_pair calls, bias gradients included)")
    for B in a.batches:
        M = B * 1281
        g = torch.Generator().manual_seed(B)
        t = {}
        for name, (N, K) in (("qkv", QKV), ("proj", PROJ), ("fc1", FC1), ("fc2", FC2)):
            t[name] = (torch.randn(M, N, generator=g).to(ops.BF16).to(dev), torch.randn(M, K, generator=g).to(ops.BF16).to(dev),
                       torch.zeros(N, K, device=dev), torch.zeros(N, device=dev))
        for pair, first, second in (("qkv + proj", QKV, PROJ), ("fc1 + fc2", FC1, FC2)):
            names = pair.split(" + ")

            def launch():
                ops.linear_wgrad_accum_pair(t[names[0]], t[names[1]])

            s0, _ = pair_slices(first, second, M, False)
            s1, sb = pair_slices(first, second, M, True)
            note = f"   k slices {s0} -> {s1}, slabs {sb / 2 ** 20:.0f} MiB"
            timed(f"B = {B:3d}  {pair}", {name: in_mode(flag, launch) for name, flag in MODES}, a.wgrad_reps, note)
        del t
        torch.cuda.empty_cache()

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
