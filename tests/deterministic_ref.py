"""Shared helpers of the deterministic-mode tests (a helper, not a conftest): the numpy model of the fold order, the plan queries,
and the shapes of the planner sweep.

Deterministic mode (include/octmae.h, "deterministic") specifies the result of a k-split weight gradient by its order of additions:

    gW[a][b] = (...((gW[a][b] + P_0[a][b]) + P_1[a][b]) ... + P_{S-1}[a][b])        fp32, slices ascending, onto the old value

-- by definition what S unsplit launches over the slices' row ranges, issued in order, leave.  fold() is that sentence in numpy; the GPU
tests build P_z from unsplit launches of the same kernel family and compare bits.  chunk_sum() is the same sentence for the gradient
norm: sumsq[t] = (...((0 + p_0) + p_1) ...) over the per-chunk sums of tensor t."""
import ctypes

import numpy as np

EPS32 = 2.0 ** -23
TK = 64                      # rows of dY / X per k-tile of a weight gradient (csrc/gemm_plan.hpp)
ROUTE_SLABS = 3              # atomic1 slot of a plan whose launch stores slabs and is followed by the fold
COLSUM_FUSED = 1


def fold(gw0, partials):
    """fp32 [NA, NB] <- ((gw0 + P_0) + P_1) ... in float32, one rounding per addition"""
    acc = np.asarray(gw0, dtype=np.float32).copy()
    for p in partials:
        acc = (acc + np.asarray(p, dtype=np.float32)).astype(np.float32)
    return acc


def fold_bound(gw0, partials):
    """|fold - exact sum| <= gamma_n (|gw0| + sum |P_z|), gamma_n = n u / (1 - n u), u = 2^-24, n = S + 1: the textbook bound of a
    recursive fp32 sum (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2) with one addition to spare; + the
    smallest subnormal, for sums that underflow"""
    mag = np.abs(np.asarray(gw0, dtype=np.float64))
    for p in partials:
        mag = mag + np.abs(np.asarray(p, dtype=np.float64))
    n, u = len(partials) + 1, EPS32 / 2.0
    return n * u / (1.0 - n * u) * mag + float(np.finfo(np.float32).smallest_subnormal)


def chunk_sum(parts, start=0.0):
    s = np.float32(start)
    for p in parts:
        s = np.float32(s + np.float32(p))
    return s


def slice_rows(bounds, M):
    """[(first row, end row)] of the k slices whose first k-tiles are bounds[0 .. S]"""
    return [(TK * bounds[z], min(TK * bounds[z + 1], M)) for z in range(len(bounds) - 1)]


# ---- plan queries ----------------------------------------------------------------------------------------------------------------
GEMM_PLAN_KEYS = ("kernel", "grid", "tiles_a", "tiles_b", "cgroup", "slices", "per", "kstagger", "atomic1", "nst", "small_split", "ws_rows",
                  "colsum")
PAIR_PLAN_KEYS = ("kernel", "grid", "slices", "per", "kstagger", "atomic1", "nst", "colsum", "ta0", "tb0", "cg0", "ta1", "tb1", "cg1")


def gemm_plan(lib, kind, N, K, M, ws_bytes, cus=256, variant=0, splitk=0, ldy=None, ldx=None):
    """octmae_gemm_plan_ws of the weight gradient gW[N][K] += dY[M][N]^T X[M][K] (kind 5; 6 with the bias gradient) -> (rc, dict)"""
    out = (ctypes.c_int * 13)()
    rc = lib.octmae_gemm_plan_ws(kind, N, K, M, ldy or N, ldx or K, variant, splitk, ws_bytes, cus, out)
    return rc, dict(zip(GEMM_PLAN_KEYS, out))


def gemm_plan_old(lib, kind, N, K, M, have_ws, cus=256, variant=0, splitk=0):
    out = (ctypes.c_int * 13)()
    rc = lib.octmae_gemm_plan(kind, N, K, M, N, K, variant, splitk, have_ws, cus, out)
    return rc, dict(zip(GEMM_PLAN_KEYS, out))


def pair_plan(lib, first, second, M, ws_bytes, cus=256, splitk=0):
    """octmae_wgrad_pair_plan_ws of (N0, K0) + (N1, K1) over M rows -> (rc, dict)"""
    out = (ctypes.c_int * 14)()
    rc = lib.octmae_wgrad_pair_plan_ws(first[0], first[1], first[0], first[1], second[0], second[1], second[0], second[1], M, splitk,
                                       ws_bytes, cus, out)
    return rc, dict(zip(PAIR_PLAN_KEYS, out))


def pair_plan_old(lib, first, second, M, cus=256, splitk=0):
    out = (ctypes.c_int * 14)()
    rc = lib.octmae_wgrad_pair_plan(first[0], first[1], first[0], first[1], second[0], second[1], second[0], second[1], M, splitk, cus, out)
    return rc, dict(zip(PAIR_PLAN_KEYS, out))


def split_bounds(lib, M, slices, tiles):
    """the first k-tile of every slice of the launch a plan with `slices` slices runs (octmae_wgrad_split_plan) -> (stagger, [S + 1])"""
    n = ctypes.c_int(0)
    b = (ctypes.c_int * (slices + 1))()
    d = lib.octmae_wgrad_split_plan(M, slices, tiles, ctypes.byref(n), b)
    assert d >= 0 and n.value == slices, (d, n.value, slices)
    return d, list(b)


def ws_bytes_for(lib, N0, K0, N1, K1, M, want_bias, slices):
    """octmae_wgrad_det_ws_bytes: the workspace to lend for `slices` slices (column-sum rows at the head + slabs)"""
    b = ctypes.c_longlong(-1)
    assert lib.octmae_wgrad_det_ws_bytes(N0, K0, N1, K1, M, int(want_bias), slices, ctypes.byref(b)) == 0
    return b.value


def colsum_head(lib, M, N):
    """bytes of the column-sum rows at the head of a lent workspace (include/octmae.h: octmae_wgrad_det_ws_bytes)"""
    return (lib.octmae_colsum_ws_rows(M) * N * 4 + 255) // 256 * 256


def split_ws_bytes(lib):
    return lib.octmae_gemm_split_ws_kib() * 1024


# ---- the planner sweep -----------------------------------------------------------------------------------------------------------
# ViT-L weight gradients (N, K) of the encoder (width 1024) and the decoder (width 512): qkv, proj, fc1, fc2; rows per volume 1281 / 5121
VITL = {1024: [(3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096)], 512: [(1536, 512), (512, 512), (2048, 512), (512, 2048)]}
ROWS_PER_VOLUME = {1024: 1281, 512: 5121}
VOLUMES = (1, 4, 32, 128)
RAGGED_NK = (136, 200, 256, 264)
RAGGED_M = (520, 1000, 4100, 8192)


def sweep_singles():
    """(N, K, M) of every single weight-gradient launch of the sweep"""
    out = []
    for width, shapes in VITL.items():
        for v in VOLUMES:
            out += [(N, K, v * ROWS_PER_VOLUME[width]) for N, K in shapes]
    out += [(N, K, M) for N in RAGGED_NK for K in RAGGED_NK for M in RAGGED_M]
    return out


def sweep_pairs():
    """((N0, K0), (N1, K1), M): qkv + proj and fc1 + fc2 of both widths, and the ragged widths that take the pair (>= 256 each way)"""
    out = []
    for width, (qkv, proj, fc1, fc2) in VITL.items():
        for v in VOLUMES:
            out += [(qkv, proj, v * ROWS_PER_VOLUME[width]), (fc1, fc2, v * ROWS_PER_VOLUME[width])]
    out += [((256, 264), (264, 256), M) for M in RAGGED_M] + [((256, 512), (512, 256), M) for M in (1024, 4096)]
    return out
