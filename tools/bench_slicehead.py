"""RETFound-all (slice-pooled ViT-L, models_vit_3dhead) and RETFound-center (models_vit_flash_attn) throughput, and the slice-pooling
kernels on their own.  One case per process, so that every GPU step can run under a time limit of its own:

    python tools/bench_slicehead.py --case train --batch 2 --slices 24      # fwd + bwd + clip + layer-decay AdamW, volumes/s
    python tools/bench_slicehead.py --case eval --batch 8 --slices 24       # no_grad forward, volumes/s
    python tools/bench_slicehead.py --case center2d --batch 24 [--eval]     # the 2-D flash ViT at the same B*S, images/s
    python tools/bench_slicehead.py --case pool --batch 8 --slices 24       # pool fwd / bwd alone: time and HBM rate of the dx write

--ktimer adds one timed step per train case (ops.KernelTimer, every launch) and reports the pooling kernels' share of it."""
import argparse, json, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octcubem_amd import lr_decay, misc, models_vit_3dhead, models_vit_flash_attn, ops
from octcubem_amd import optim as foptim

ap = argparse.ArgumentParser()
ap.add_argument("--case", choices=["train", "eval", "center2d", "pool"], required=True)
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--slices", type=int, default=24)
ap.add_argument("--img", type=int, default=224)
ap.add_argument("--classes", type=int, default=3)
ap.add_argument("--drop-path", type=float, default=0.2)
ap.add_argument("--steps", type=int, default=10)      # 5 steps after one warm-up left the 24-slice step 40 % high on one run
ap.add_argument("--eval", action="store_true")
ap.add_argument("--ktimer", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda")
torch.manual_seed(0)


def timed(fn, steps):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


if a.case == "pool":
    BS, T, D = a.batch * a.slices, (a.img // 16) ** 2 + 1, 1024
    x = torch.randn(BS, T, D, device=dev)
    g, b = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    dg, db, cs = torch.zeros(D, device=dev), torch.zeros(D, device=dev), torch.zeros(D, device=dev)
    out, pooled, mean, rstd = ops.slice_pool_fwd(x, g, b, 1e-6, a.slices, False)
    dout = torch.randn(a.batch, D, device=dev)
    del x
    res = {"workload": "slice pool kernels", "BS": BS, "T": T, "D": D}
    xs = torch.randn(BS, T, D, device=dev)
    for name, fn, nbytes in (
            ("fwd", lambda: ops.slice_pool_fwd(xs, g, b, 1e-6, a.slices, False), 4.0 * BS * (T - 1) * D),
            ("bwd_f32", lambda: ops.slice_pool_bwd(dout, pooled, mean, rstd, g, T, a.slices, False, dg, db), 4.0 * BS * T * D),
            ("bwd_f32_lp", lambda: ops.slice_pool_bwd(dout, pooled, mean, rstd, g, T, a.slices, False, dg, db, True, cs), 6.0 * BS * T * D)):
        fn(); torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
        for s, e in ev:
            s.record(); fn(); e.record()
        torch.cuda.synchronize()
        us = sorted(s.elapsed_time(e) for s, e in ev)[len(ev) // 2] * 1e3
        res[f"{name}_us"] = us
        res[f"{name}_tb_s"] = nbytes / us * 1e-6
    print(json.dumps(res))
    sys.exit(0)

if a.case == "center2d":
    m = models_vit_flash_attn.flash_attn_vit_large_patch16(img_size=a.img, num_classes=a.classes, global_pool=True,
                                                           drop_path_rate=a.drop_path).to(dev)
    x = torch.rand(a.batch, 3, a.img, a.img, device=dev)
    unit = "images"
else:
    m = models_vit_3dhead.flash_attn_vit_large_patch16_3DSliceHead(img_size=a.img, num_classes=a.classes, global_pool=True,
                                                                   drop_path_rate=a.drop_path).to(dev)
    x = torch.rand(a.batch, a.slices, 3, a.img, a.img, device=dev)
    unit = "volumes"
t = torch.randint(0, a.classes, (a.batch,), device=dev)
train = a.case == "train" or (a.case == "center2d" and not a.eval)
res = {"workload": f"{a.case} {'train step' if train else 'eval forward'}", "batch": a.batch, "img": a.img}
if a.case != "center2d":
    res["slices"] = a.slices
if train:
    m.train()
    opt = foptim.FusedAdamW(lr_decay.param_groups_lrd(m, 0.05, m.no_weight_decay(), 0.65), lr=1e-4)
    scaler = misc.NativeScalerWithGradNormCount()
    params = list(m.parameters())

    def step():
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(m(x), t)
        scaler(loss, opt, clip_grad=1.0, parameters=params, update_grad=True)
else:
    m.eval()

    def step():
        with torch.no_grad():
            m(x)
dt = timed(step, a.steps)
res.update({"ms_per_step": dt * 1e3, f"{unit}_per_s": a.batch / dt, "max_mem_gb": torch.cuda.max_memory_allocated() / 2**30})
if a.ktimer:
    ops.KTIMER = ops.KernelTimer(stride=1)
    step()
    s = ops.KTIMER.summary()
    ops.KTIMER = None
    pool_ms = sum(v["total_ms"] for k, v in s.items() if k.startswith("pool_"))
    res["pool_ms"] = pool_ms
    res["pool_share_of_step"] = pool_ms / (dt * 1e3)
    res["timed_kernels_ms"] = sum(v["total_ms"] for v in s.values())
    res["pool_kernels"] = {k: {"avg_us": v["avg_us"], "launches": v["launches"], "tb_s": v["bytes"] / v["avg_us"] * 1e-6 if v["avg_us"] else 0.0}
                           for k, v in s.items() if k.startswith("pool_")}
    res["attn_kernels"] = {k: {"avg_us": v["avg_us"], "tflops": v["flops"] / v["launches"] / v["avg_us"] * 1e-6}
                           for k, v in s.items() if k.startswith("attn")}
print(json.dumps(res))
