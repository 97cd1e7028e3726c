"""Times the low-rank adapter path (octcubem_amd.lora, csrc/lora.hip) on one MI355X, in one run:

    python tools/bench_lora.py [--out profiles/lora_bench.txt]

(a) kernels: ``ops.lora_wgrad`` for the four Linears of a ViT-L Block (C = 1024) at M = 5121, 4 x 5121 and 32 x 1281 token rows and ranks 8
    and 16, against the weight-gradient PAIR launch it replaces over the same operands (qkv + proj, fc1 + fc2); ``ops.lora_merge`` for
    one Block and for the 24 Blocks of the model.  Time: device events around --reps calls, median [min .. max] of --rounds windows,
    the two paths alternating.  The operands rotate through enough copies to exceed the 256 MiB Infinity Cache twice, so they come
    from HBM ("cold"); the bytes are the algorithm's (ops.lora_wgrad's own count: X and dY twice, T / U, the slabs, the gradients), the
    HBM share is those bytes over the time over the 8 TB/s of the data sheet.
(b) step: forward + backward + FusedAdamW step of the ViT-L spatio-temporal fine-tune model (60 x 256 x 256 volumes, 5121 tokens) at
    batch 1, 4 and 8: every weight trained against adapters (rank --rank on all four Linears) + head, alternating windows of one run;
    the memory one step adds, the bytes of the gradients and the optimizer state, the losses of the timed steps, checkpoint sizes."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from octcubem_amd import lora, lr_decay, models_vit_st, ops      # noqa: E402
from octcubem_amd import optim as foptim                          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--step-reps", type=int, default=2)
ap.add_argument("--step-rounds", type=int, default=3)
ap.add_argument("--rank", type=int, default=16)
ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 8])
ap.add_argument("--parts", nargs="+", default=["kernels", "step"], choices=["kernels", "step"])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_bench.txt"))
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_lora: needs an MI355X (a timing taken without one says nothing)")
dev = torch.device("cuda")
LP = ops.BF16
HBM = 8.0e12
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps       # milliseconds per call


def alternate(paths, reps, rounds):
    for fn in paths.values():
        fn(0)
        fn(1)
    ts = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            ts[k].append(window(fn, reps))
    return ts


def fmt(ts):
    return f"{statistics.median(ts):8.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]"


class Counter:
    """ops.KTIMER stand-in that only keeps the byte and flop counts the wrappers state"""

    def __init__(self):
        self.bytes = {}

    def launch(self, kind, flops, nbytes, fn, exec_flops=None):
        self.bytes[kind] = self.bytes.get(kind, 0.0) + nbytes
        fn()


say(f"# tools/bench_lora.py  {torch.cuda.get_device_name(0)}  torch {torch.__version__}  operands {LP}; the gradient kernel is the two-pass form")
C = 1024
PAIRS = {"attention": (("proj", C, C), ("qkv", C, 3 * C)), "mlp": (("fc2", 4 * C, C), ("fc1", C, 4 * C))}      # (name, I, O)

if "kernels" in a.parts:
    say(f"## (a) adapter gradients against the weight-gradient pair they replace; median [min .. max] of {a.rounds} alternating windows of "
        f"{a.reps} calls, cold operands")
    for M in (5121, 4 * 5121, 32 * 1281):
        for pair, layers in PAIRS.items():
            per_set = sum(2 * M * (I + O) for _, I, O in layers)
            nset = max(2, min(8, -(-(2 * 256 << 20) // per_set)))
            sets = []
            for k in range(nset):
                g = torch.Generator(device=dev).manual_seed(k)
                sets.append([(torch.randn((M, I), generator=g, device=dev).to(LP), (0.1 * torch.randn((M, O), generator=g, device=dev)).to(LP))
                             for _, I, O in layers])
            gW = [torch.zeros((O, I), device=dev) for _, I, O in layers]

            def full(i, sets=sets, gW=gW):
                (x0, d0), (x1, d1) = sets[i % len(sets)]
                ops.linear_wgrad_accum_pair((d0, x0, gW[0], None), (d1, x1, gW[1], None))
            paths = {"pair": full}
            counted = {}
            for r in (8, 16):
                rp = ops.lora_rp(r)
                ad = []
                for _, I, O in layers:
                    A, B = torch.randn((r, I), device=dev) / I ** 0.5, 0.1 * torch.randn((O, r), device=dev)
                    A_lp, B_lp = torch.empty((rp, I), dtype=LP, device=dev), torch.empty((O, rp), dtype=LP, device=dev)
                    ops.lora_merge(torch.zeros((O, I), device=dev), A, B, 2.0, torch.empty((O, I), dtype=LP, device=dev), A_lp, B_lp)
                    ad.append((A_lp, B_lp, torch.zeros((r, I), device=dev), torch.zeros((O, r), device=dev)))

                def adapters(i, sets=sets, ad=ad, r=r, only=None):
                    for k, ((x, d), (A_lp, B_lp, gA, gB)) in enumerate(zip(sets[i % len(sets)], ad)):
                        if only is None or only == k:
                            ops.lora_wgrad(x, d, A_lp, B_lp, 2.0, r, gA, gB)
                paths[f"r{r}"] = adapters
                for k, (name, I, O) in enumerate(layers):
                    paths[f"r{r}/{name}"] = lambda i, f=adapters, k=k: f(i, only=k)
                    ops.KTIMER = cnt = Counter()
                    adapters(0, only=k)
                    ops.KTIMER = None
                    counted[f"r{r}/{name}"] = cnt.bytes["lora_wgrad"]
                counted[f"r{r}"] = sum(counted[f"r{r}/{name}"] for name, _, _ in layers)
            ts = alternate(paths, a.reps, a.rounds)
            t_pair = statistics.median(ts["pair"])
            flop = sum(2.0 * M * I * O for _, I, O in layers)
            say(f"  M = {M:6d}  {pair:9s} ({' + '.join(n for n, _, _ in layers)}), {nset} operand sets of {per_set / 2 ** 20:.0f} MiB")
            say(f"    weight-gradient pair      {fmt(ts['pair'])}   {flop / t_pair / 1e9:7.1f} TFLOP/s")
            for k in [k for k in ts if k != "pair"]:
                t = statistics.median(ts[k])
                say(f"    adapters {k:16s} {fmt(ts[k])}   {counted[k] / 2 ** 20:8.1f} MiB, {counted[k] / (t * 1e-3) / 1e12:5.2f} TB/s = "
                    f"{100 * counted[k] / (t * 1e-3) / HBM:4.1f} % of 8 TB/s" + (f"   x{t / t_pair:.3f} of the pair" if "/" not in k else ""))
            del sets, gW, paths
            torch.cuda.empty_cache()
    say("## merge (W + s B A -> 16-bit operand + padded adapter copies), rank 16: one ViT-L Block (4 Linears), and 24 Blocks")
    Ws = [[torch.randn((O, I), device=dev) * 0.02 for I, O in ((C, 3 * C), (C, C), (C, 4 * C), (4 * C, C))] for _ in range(24)]
    As = [[(torch.randn((16, w.shape[1]), device=dev), torch.randn((w.shape[0], 16), device=dev), torch.empty(w.shape, dtype=LP, device=dev),
            torch.empty((16, w.shape[1]), dtype=LP, device=dev), torch.empty((w.shape[0], 16), dtype=LP, device=dev)) for w in blk] for blk in Ws]

    def merge(i, nblk):
        for b in range(nblk):
            for w, (A, B, out, A_lp, B_lp) in zip(Ws[(i + b) % 24], As[(i + b) % 24]):
                ops.lora_merge(w, A, B, 2.0, out, A_lp, B_lp)
    ts = alternate({"block": lambda i: merge(i, 1), "model": lambda i: merge(0, 24)}, a.reps, a.rounds)
    per_block = 6.0 * 12 * C * C
    for k, n in (("block", 1), ("model", 24)):
        t = statistics.median(ts[k])
        say(f"  {k:5s} {fmt(ts[k])}   {n * per_block / 2 ** 20:7.1f} MiB read + written, {n * per_block / (t * 1e-3) / 1e12:5.2f} TB/s")
    del Ws, As
    torch.cuda.empty_cache()

if "step" in a.parts:
    say(f"## (b) ViT-L spatio-temporal fine-tune step (flash blocks, 60 x 256 x 256, 5121 tokens per volume): forward + backward + FusedAdamW; "
        f"median [min .. max] of {a.step_rounds} alternating windows of {a.step_reps} steps; adapters of rank {a.rank} on qkv, proj, fc1, fc2 + head")

    def build(adapted):
        torch.manual_seed(0)
        m = models_vit_st.flash_attn_vit_large_patch16(num_frames=60, t_patch_size=3, img_size=256, in_chans=1, num_classes=8,
                                                       sep_pos_embed=True, cls_embed=True).to(dev).train()
        if adapted:
            lora.attach(m, rank=a.rank, alpha=2 * a.rank)
            lora.mark_only_lora_trainable(m)
            with torch.no_grad():
                for n, p in m.named_parameters():
                    if n.endswith("_B"):
                        p.normal_(0.0, 0.02)
        opt = foptim.FusedAdamW(lr_decay.param_groups_lrd(m, 0.05, m.no_weight_decay(), 0.75), lr=1e-5)
        return m, opt
    models = {"full": build(False), "adapted": build(True)}
    for k, (m, _) in models.items():
        n_train = sum(p.numel() for p in m.parameters() if p.requires_grad)
        sd = lora.lora_state_dict(m) if k == "adapted" else m.state_dict()
        ck = sum(v.numel() * v.element_size() for v in sd.values())
        say(f"  {k:8s} trainable parameters {n_train / 1e6:8.2f} M: gradients {4 * n_train / 2 ** 20:8.1f} MiB, AdamW moments {8 * n_train / 2 ** 20:8.1f} MiB, "
            f"checkpoint ({'adapters + head + norms' if k == 'adapted' else 'state dict'}) {ck / 2 ** 20:8.1f} MiB")
    for Bn in a.batches:
        g = torch.Generator(device=dev).manual_seed(Bn)
        x = torch.randn((Bn, 1, 60, 256, 256), generator=g, device=dev)
        tgt = torch.randint(0, 8, (Bn,), generator=g, device=dev)
        losses = {k: [] for k in models}

        def step(i, k):
            m, opt = models[k]
            opt.zero_grad()
            loss = torch.nn.functional.cross_entropy(m(x), tgt)
            loss.backward()
            opt.step()
            losses[k].append(loss.detach())
        paths = {k: (lambda i, k=k: step(i, k)) for k in models}
        mem = {}
        for k, fn in paths.items():
            fn(0)
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn(1)
            torch.cuda.synchronize()
            mem[k] = torch.cuda.max_memory_allocated() - before
        ts = alternate(paths, a.step_reps, a.step_rounds)
        t0 = statistics.median(ts["full"])
        for k in models:
            t = statistics.median(ts[k])
            ls = [float(v) for v in losses[k]]
            say(f"  B = {Bn}  {k:8s} {fmt(ts[k])}  x{t / t0:.3f}   added by one step {mem[k] / 2 ** 30:7.2f} GiB   loss first {ls[0]:.4f} last {ls[-1]:.4f} "
                f"({len(ls)} steps)")
        del x, tgt
        torch.cuda.empty_cache()

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
