#!/usr/bin/env python3
"""Which kernels the GEMM entry points launch: every Linear shape of the ViT-L 3-D MAE (encoder and decoder, 1 / 4 / 32 / 128 volumes)
and the shapes of tests/test_gpu_kernels.py, once each and in a fixed order, through every ops entry point and kernel variant, with the
split-K workspace lent and not.  Run it under a kernel trace and compare two traces (two commits, two option settings):

    rocprofv3 --kernel-trace --output-format csv -d OUT -o sweep -- python tools/gemm_dispatch_sweep.py [--variants a,b,...] [--volumes 1,4]
    python tools/gemm_dispatch_sweep.py --diff A_kernel_trace.csv B_kernel_trace.csv      (no GPU)

The run prints one line per case: its name and how far the small-launch counters moved.  --diff compares the sequence of (kernel, grid,
workgroup, LDS bytes) of every GEMM and column-sum launch and prints the launches that differ, grouped by (kernel before -> after)."""
import csv
import os
import re
import sys

VARIANTS = {"auto": (False, False, False, 0, 1), "tile128": (True, False, False, 0, 1), "twostage": (False, True, False, 0, 1),
            "phased": (False, False, True, 0, 1), "small4": (False, False, False, 4, 1), "small2": (False, False, False, 2, 1),
            "small4_split3": (False, False, False, 4, 3), "small2_split2": (False, False, False, 2, 2), "never_small": (False, False, False, -1, 1)}
DEFAULT_VARIANTS = "auto,tile128,small4,small2,small4_split3,small2_split2,never_small"
TEST_SHAPES = [(128, 128, 64), (256, 384, 128), (200, 136, 72), (1281, 384, 128), (64, 64, 64), (5121, 192, 64), (130, 768, 512),
               (600, 512, 256), (2000, 1024, 1024), (3000, 512, 256), (2562, 768, 512), (600, 4096, 256), (700, 512, 4096)]


def linears(volumes):
    """(name, M, N, K) of every Linear: y[M, N] = x[M, K] w[N, K]^T"""
    out = []
    for B in volumes:
        for part, M, D in (("enc", B * 1281, 1024), ("dec", B * 5121, 512)):
            out += [(f"B{B}_{part}_{ln}", M, N, K) for ln, N, K in (("qkv", 3 * D, D), ("proj", D, D), ("fc1", 4 * D, D), ("fc2", D, 4 * D))]
    return out + [(f"t_{M}x{N}x{K}", M, N, K) for M, N, K in TEST_SHAPES]


def run(variants, volumes):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from octcubem_amd import ops
    dev, BF, F32 = "cuda", ops.BF16, torch.float32
    z = lambda *s, dt=BF: torch.zeros(*s, dtype=dt, device=dev)      # noqa: E731  (values do not matter: only what is launched)
    ctr = lambda: tuple(ops.set_option(k, 0) for k in ("gemm_small_launches", "gemm_small_split_launches", "gemm_small_wgrad_launches"))  # noqa: E731
    for name, M, N, K in linears(volumes):
        x, w, b, dy, pre = z(M, K), z(N, K), z(N, dt=F32), z(M, N), z(M, K)
        res, sc, cs = z(M, N, dt=F32), torch.ones(M, dtype=F32, device=dev), z(K, dt=F32)
        gw, gw2, gb = z(N, K, dt=F32), z(N, K, dt=F32), z(N, dt=F32)
        hd = 64 if K % 64 == 0 else 32
        cases = [("fwd_" + m, lambda m=m: ops.linear_fwd(x, w, b, m, res=res if m == "resid" else None)) for m in ("bf16", "f32", "gelu", "resid")]
        cases += [("fwd_rowscale", lambda: ops.linear_fwd(x, w, b, "resid", res=res, rowscale=sc, rows_per_scale=1)),
                  ("dgrad", lambda: ops.linear_dgrad(dy, w)),
                  ("dgrad_pre", lambda: ops.linear_dgrad(dy, w, pre=pre)),
                  ("dgrad_pre_colsum", lambda: ops.linear_dgrad(dy, w, pre=pre, colsum=cs)),
                  ("wgrad", lambda: ops.linear_wgrad_accum(dy, x, gw, gb)),
                  ("wgrad_pair", lambda: ops.linear_wgrad_accum_pair((dy, x, gw, gb), (dy, x, gw2, None)))]
        if K % hd == 0:
            cases.insert(8, ("dgrad_delta", lambda: ops.linear_dgrad_delta(dy, w, pre, K // hd, hd)))
        for ws in (True, False):
            ops.SPLIT_WS = ws
            for v in variants:
                ops.FORCE_SMALL_TILE, ops.FORCE_TWO_STAGE, ops.FORCE_PHASED, ops.FORCE_SMALL_LAUNCH, ops.FORCE_SPLITK = VARIANTS[v]
                for cname, fn in cases:
                    c0 = ctr()
                    fn()
                    print(f"{name} ws={int(ws)} {v} {cname} small+{'/'.join(str(a - b) for a, b in zip(ctr(), c0))}", flush=True)
        torch.cuda.synchronize()
        del x, w, b, dy, pre, res, sc, cs, gw, gw2, gb, cases
    # the weight-gradient pairs as the Blocks launch them: fc2 + fc1 and proj + qkv over the same token rows
    ops.FORCE_SMALL_TILE, ops.FORCE_TWO_STAGE, ops.FORCE_PHASED, ops.FORCE_SMALL_LAUNCH, ops.FORCE_SPLITK = VARIANTS["auto"]
    for B in volumes:
        for part, M, D in (("enc", B * 1281, 1024), ("dec", B * 5121, 512)):
            y1, act, dpre, dqkv = z(M, D), z(M, 4 * D), z(M, 4 * D), z(M, 3 * D)
            gw2, gw1, gwp, gwq = z(D, 4 * D, dt=F32), z(4 * D, D, dt=F32), z(D, D, dt=F32), z(3 * D, D, dt=F32)
            gb2, gb1, gbp, gbq = z(D, dt=F32), z(4 * D, dt=F32), z(D, dt=F32), z(3 * D, dt=F32)
            for pname, first, second in (("fc2+fc1", (y1, act, gw2, gb2), (dpre, y1, gw1, gb1)), ("proj+qkv", (y1, y1, gwp, gbp), (dqkv, y1, gwq, gbq))):
                c0 = ctr()
                ops.linear_wgrad_accum_pair(first, second)
                print(f"B{B}_{part}_{pname} pair small+{'/'.join(str(a - b) for a, b in zip(ctr(), c0))}", flush=True)
            torch.cuda.synchronize()
            del y1, act, dpre, dqkv, gw2, gw1, gwp, gwq


def launches(path):
    """[(kernel, grid, workgroup, LDS bytes)] of the GEMM and column-sum launches of a rocprofv3 kernel trace, in start order"""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    out = []
    for r in rows:
        m = re.search(r"(gemm\w*_kernel|colsum\w*)(<[^(]*>)?", r["Kernel_Name"])
        if m:
            out.append((m.group(1) + (m.group(2) or ""), "x".join(r[f"Grid_Size_{a}"] for a in "XYZ"),
                        "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ"), r.get("LDS_Block_Size", r.get("LDS_Block_Size_v", "?"))))
    return out


def diff(a_path, b_path):
    a, b = launches(a_path), launches(b_path)
    print(f"{a_path}: {len(a)} GEMM / column-sum launches\n{b_path}: {len(b)} GEMM / column-sum launches")
    if len(a) != len(b):
        print("DIFFERENT NUMBER OF LAUNCHES")
    changed = {}
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            key = (re.sub(r"<.*", "", x[0]), re.sub(r"<.*", "", y[0]))
            changed.setdefault(key, []).append(i)
    for (ka, kb), idx in sorted(changed.items()):
        print(f"{len(idx):6d} launches  {ka} -> {kb}   (first: #{idx[0]} {a[idx[0]]} -> {b[idx[0]]})")
    print("IDENTICAL SEQUENCES" if not changed and len(a) == len(b) else f"{sum(len(v) for v in changed.values())} launches differ")
    return 0 if not changed and len(a) == len(b) else 1


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--diff"]:
        sys.exit(diff(args[1], args[2]))
    opt = dict(zip(args[::2], args[1::2]))
    run(opt.get("--variants", DEFAULT_VARIANTS).split(","), [int(v) for v in opt.get("--volumes", "1,4,32,128").split(",")])
