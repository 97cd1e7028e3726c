"""Every output element of every GEMM epilogue against a bound derived from the arithmetic, and every finite 16-bit input of the two
activation formulas through every kernel that evaluates them -- on whichever library OCTMAE_LIB selects (bfloat16 in the normal
session, IEEE half in the child of tests/test_gpu_f16_kernels.py; the bounds are written in U, so the same file serves both).

tests/gemm_elem.py holds the bounds (tests/test_cpu_gemm_elem.py shows on the CPU what they let through and what they do not):
fp32 accumulation of n products in any order (n + 4) 2^-23 sum |a b|, one rounding into the 16-bit type 2 U |ref| + tiny, and the
two activation formulas' own errors.  References are float64 products of the same rounded operands, computed once per shape on the
CPU and shared by the nine kernel variants of tests/test_gpu_kernels.py::tile_variant.  The shapes are the smallest at which each
dispatch rule of csrc/gemm_plan.hpp is still on its far side; none comes from the workload.

Two things the epilogues do that the bounds spell out (read in csrc/gemm.hip, gemm_epilogue and the LDS-transposing epilogue):
  * dgrad x GELU': the kernels with the LDS-transposing epilogue (256-tile kernels, small-launch kernel) round X = dy @ w to 16 bits on
    its way through the transpose and multiply the ROUNDED value by gelu'(pre) -- two roundings, as oracle/bf16_points.py models
    them; the 128-tile register-staged kernel multiplies its fp32 accumulator and rounds once.  The bound takes its second
    lp_round_bound from the plan (octmae_gemm_plan) of the very launch: the one-rounding bound holds wherever one rounding is made.
  * the column sums that ride along with dgrad x GELU' are sums of the STORED, rounded dx in all three forms (per-slab workspace +
    fold, fp32 atomics, the stand-alone pass over the output after the 128-tile kernel): the reference is the sum of the kernel's
    own output.

Measured on an MI355X, worst ratio to the bound per family (bfloat16 build / half build): MEASURED below.  The fp32-limited families
sit at 0.01 ... 0.07 of their bound (random rounding errors add like sqrt(n), the bound like n), the 16-bit ones at 0.7 ... 0.99 (a
rounding error does reach half a spacing), and the two sweeps reproduce the CPU restatement of the formulas to all digits shown.
The whole module, nine variants included, takes 3.1 s per build.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import ops
    from octcubem_amd._lib import load
    LP = ops.BF16
else:
    LP = torch.bfloat16
from tests import gemm_elem as GE
from tests.conftest import parity
from tests.test_gpu_kernels import tile_variant  # noqa: F401  (the GEMM kernel-choice fixture)

# worst |got - ref| / bound per family on an MI355X (bfloat16 build, half build), recorded after the run that introduced this module
MEASURED = {
    "fwd_f32": (0.0127, 0.0137), "fwd_resid": (0.0141, 0.0141), "fwd_rowscale": (0.0133, 0.0133), "fwd_bits": (0.0, 0.0),
    "dgrad_bits": (0.0, 0.0), "dgrad_f32": (0.0480, 0.0723), "gelu_act": (0.965, 0.859), "gelu_stored_prime": (0.993, 0.885),
    "dgelu_1r": (0.988, 0.871), "dgelu_stored_1r": (0.922, 0.772), "dgelu_2r": (0.924, 0.783), "dgelu_stored_2r": (0.853, 0.699),
    "dgelu_colsum": (0.0548, 0.0547), "wgrad": (0.0103, 0.0160), "wgrad_bias": (0.0023, 0.0048), "wgrad_pair": (0.0066, 0.0065),
    "wgrad_pair_bias": (0.0010, 0.0022), "delta_do": (0.954, 0.750), "delta": (0.0135, 0.0175),
    "gelu_sweep": (0.965, 0.859), "dgelu_sweep": (0.993, 0.885), "dgelu_fwd_sweep": (0.993, 0.885),
    "gelu_sweep_poly_excess": (2.7e-6, 0.0),      # of 2e-5: (|act - gelu| - rounding allowance) / |x| at |x| >= 1
}

DEV = "cuda"
IS_F16 = LP == torch.float16
TAG = "f16" if IS_F16 else "bf16"
U = GE.LP_U[LP]
TINY = torch.finfo(LP).tiny

# (M, N, K): y[M, N] = x[M, K] @ w[N, K]^T and its dgrad dx[M, K] = dy[M, N] @ w[N, K]
SHAPES = [
    (300, 264, 192),    # 2 x 2 ragged 256-tiles, 3 x 3 ragged 128-tiles, N % 8 == 0 (small launch admitted), 3 k-tiles
    (333, 260, 64),     # N % 8 != 0: the small launch declines; one k-tile.  (The dgrad reduces over N: its operands are padded with
                        #   zeros to 264, the library's 8-element granularity -- a ragged k tail on the register-staged kernel, whose
                        #   column sums are the pass after the GEMM)
    (200, 136, 72),     # K % 64 != 0 and below 256 each way: register-staged kernel only, ragged k tail
    (257, 256, 1024),   # 16 k-tiles: the cost model's and the forced k splits are admitted (>= 8 k-tiles per slice); one row past a tile
    (300, 4096, 64),    # 16 column tiles: the column-grouped tile order
    (64, 64, 64), (1, 264, 128), (129, 8, 64),      # a single tile, a single row, the narrowest admitted N
]
_CASES = {}
_WORST = {}


def _report(family, ratio, where, variant, what=""):
    """assert ratio <= 1 with the worst element and the variant in the message; the ledger keeps each family's running maximum"""
    label = f"gemm_elem/{family}/{TAG}"
    assert ratio <= 1.0, f"{label} [{variant}] {what}: |got - ref| = {ratio:.3f} x bound at element {where}"
    if ratio > _WORST.get(label, -1.0):
        _WORST[label] = ratio
        parity(label, ratio, 1.0)


def _case(M, N, K):
    """operands (16-bit, CPU), float64 references and bounds of one Linear shape -- computed once, read-only afterwards"""
    key = (M, N, K)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    c = {"x": torch.randn(M, K, generator=g).to(LP), "w": (torch.randn(N, K, generator=g) * K ** -0.5).to(LP),
         "b": torch.randn(N, generator=g), "res": torch.randn(M, N, generator=g),
         "dy": torch.randn(M, N, generator=g).to(LP), "pre": torch.randn(M, K + 16, generator=g).to(LP)}
    xd, wd, dyd = c["x"].double(), c["w"].double(), c["dy"].double()
    c["y"] = xd @ wd.t()                                                          # without the bias
    c["y_abs"] = xd.abs() @ wd.abs().t()
    c["X"] = dyd @ wd                                                             # the dgrad product [M, K]
    c["X_acc"] = GE.acc_bound(dyd.abs(), wd.abs().t(), N)
    c["g1"] = GE.dgelu64(c["pre"][:, :K])
    _CASES[key] = c
    return c


def _dgrad_operands(c):
    """dy [M, N8] and w [N8, K] on the device, the reduction padded with zeros to a multiple of 8 (exact: zero products)"""
    M, N = c["dy"].shape
    K = c["w"].shape[1]
    N8 = (N + 7) // 8 * 8
    dy = torch.zeros(M, N8, dtype=LP); dy[:, :N] = c["dy"]
    w = torch.zeros(N8, K, dtype=LP); w[:N] = c["w"]
    return dy.to(DEV), w.to(DEV)


def _plan(kind, NA, NB, K, lda, ldb, splitk=0):
    """octmae_gemm_plan of a launch under the current variant (have_ws as ops.py lends it, the device's CU count)"""
    out = (ctypes.c_int * 13)()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rc = load().octmae_gemm_plan(kind, NA, NB, K, lda, ldb, ops._variant_bits(), splitk, 1, cus, out)
    return rc, list(out)


def _dgelu_roundings(M, N8, K, ldw, ldy):
    """2 where the dgrad x GELU' launch rounds twice (LDS-transposing epilogue), 1 on the register-staged kernel"""
    rc, out = _plan(2, K, M, N8, ldw, ldy)
    assert rc == 0
    return 1 if out[0] == 0 else 2


# ------------------------------------------------------------------------------------------------ forward, fp32 outputs
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_forward_fp32_epilogues_per_element(M, N, K, tile_variant):
    """f32 (with and without bias), resid, resid with rowscale: |y - ref| <= (K + 4) 2^-23 (|x| |w|^T + |b| + |res|) per element, the
    rowscale form scaled by the row's |scale|; dropped rows pass the residual through bit for bit."""
    c = _case(M, N, K)
    x, w, b, res = (c[k].to(DEV) for k in ("x", "w", "b", "res"))
    bd, resd = c["b"].double(), c["res"].double()
    v = tile_variant
    r, at = GE.worst(ops.linear_fwd(x, w, b, "f32"), c["y"] + bd, (K + 4) * GE.EPS32 * (c["y_abs"] + bd.abs()))
    _report("fwd_f32", r, at, v, "bias")
    r, at = GE.worst(ops.linear_fwd(x, w, None, "f32"), c["y"], (K + 4) * GE.EPS32 * c["y_abs"])
    _report("fwd_f32", r, at, v, "no bias")
    bound = (K + 4) * GE.EPS32 * (c["y_abs"] + bd.abs() + resd.abs())
    r, at = GE.worst(ops.linear_fwd(x, w, b, "resid", res=res), resd + c["y"] + bd, bound)
    _report("fwd_resid", r, at, v)
    g = torch.Generator().manual_seed(M + N)
    for rows_per in (d for d in (1, 3, M) if M % d == 0):
        sc = torch.tensor([0.0, 1.25, 2.0])[torch.randint(0, 3, (M // rows_per,), generator=g)]
        if rows_per == 1 and M >= 3:
            sc[:3] = torch.tensor([0.0, 1.25, 2.0])                               # every kind of row is there
        ys = ops.linear_fwd(x, w, b, "resid", res=res, rowscale=sc.to(DEV), rows_per_scale=rows_per)
        rows = sc.double().repeat_interleave(rows_per).unsqueeze(1)
        kept = (rows != 0).expand(M, N)
        # a dropped row's bound would be zero: it is held to equality below, and to the unscaled bound here
        r, at = GE.worst(ys, resd + rows * (c["y"] + bd), torch.where(kept, rows.abs() * bound, bound))
        _report("fwd_rowscale", r, at, v, f"rows_per_scale {rows_per}")
        dropped = (rows == 0).flatten()
        assert torch.equal(ys.cpu()[dropped], c["res"][dropped]), f"[{v}] rows_per_scale {rows_per}: a dropped row is not the residual, bit for bit"


# ------------------------------------------------------------------------------------------------ 16-bit outputs = casts of the fp32 ones
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_16bit_outputs_are_the_cast_of_the_fp32_ones(M, N, K, tile_variant):
    """Forward bf16 and the pre of gelu (one instance each), and the plain dgrad: the 16-bit output equals torch's round-to-nearest-even
    cast of the fp32 output of the same launch plan (EPI_F32 of the same layout), bit for bit; the fp32 dgrad is held per element to
    (N + 4) 2^-23 |dy| |w|."""
    c = _case(M, N, K)
    x, w, b = (c[k].to(DEV) for k in ("x", "w", "b"))
    v = tile_variant
    y32 = ops.linear_fwd(x, w, b, "f32")
    y16 = ops.linear_fwd(x, w, b, "bf16")
    r, at = GE.bit_exact(y16, y32.to(LP))
    _report("fwd_bits", r, at, v, "bf16 output vs cast of f32")
    pre, _ = ops.linear_fwd(x, w, b, "gelu")
    r, at = GE.bit_exact(pre, y16)
    _report("fwd_bits", r, at, v, "pre of gelu vs bf16 output")
    dy, wp = _dgrad_operands(c)
    out32 = torch.empty(M, K, dtype=torch.float32, device=DEV)
    ops._gemm(wp, dy, out32, K, M, dy.shape[1], wp.stride(0), dy.stride(0), K, 1, 0, ops.EPI_F32)
    dx = ops.linear_dgrad(dy, wp)
    r, at = GE.bit_exact(dx, out32.to(LP))
    _report("dgrad_bits", r, at, v, "dgrad vs cast of the fp32 dgrad")
    r, at = GE.worst(out32, c["X"], c["X_acc"])
    _report("dgrad_f32", r, at, v)


# ------------------------------------------------------------------------------------------------ GELU forward
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gelu_forward_per_element(M, N, K, tile_variant):
    """act against gelu of the STORED pre-activation in float64: one rounding + 2e-5 |pre| at pre >= -4.2, |act| <= 6e-5 below; with
    store_dgelu the first output holds gelu'(pre) rounded once (+ 1e-6) and the activation is the same, bit for bit."""
    c = _case(M, N, K)
    x, w, b = (c[k].to(DEV) for k in ("x", "w", "b"))
    pre, act = ops.linear_fwd(x, w, b, "gelu")
    ref, bound = GE.gelu_bounds(pre, U, TINY)
    r, at = GE.worst(act, ref, bound)
    _report("gelu_act", r, at, tile_variant)
    dg, act2 = ops.linear_fwd(x, w, b, "gelu", store_dgelu=True)
    r, at = GE.bit_exact(act2, act)
    _report("gelu_act", r, at, tile_variant, "act with store_dgelu vs without")
    ref, bound = GE.dgelu_bounds(pre, U, TINY)
    r, at = GE.worst(dg, ref, bound)
    _report("gelu_stored_prime", r, at, tile_variant)


# ------------------------------------------------------------------------------------------------ dgrad x GELU'
def _dgelu_bound(c, K, roundings, stored=None):
    """|dx - X g'| <= lp_round_bound(X g') + |g'| acc_bound + |X| 1e-6 [+ |g'| lp_round_bound(X) where X is rounded before the product]
    [+ |X| lp_round_bound(g') on the stored-GELU' route: g' itself was rounded once]"""
    X, g1 = c["X"], c["g1"]
    bound = GE.lp_round_bound(X * g1, U, TINY) + g1.abs() * c["X_acc"] + X.abs() * 1e-6
    if roundings == 2:
        bound = bound + g1.abs() * GE.lp_round_bound(X, U, TINY)
    if stored is not None:
        bound = bound + X.abs() * GE.lp_round_bound(g1, U, TINY)
    return bound


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_dgrad_times_gelu_prime_per_element(M, N, K, tile_variant):
    """dx = (dy @ w) * gelu'(pre), pre with its own leading dimension, and the stored-GELU' route (pre_is_dgelu: the operand holds
    gelu'(pre) rounded to 16 bits).  The one-rounding bound of the issue holds on the register-staged kernel; the LDS-transposing
    epilogues round X first (module docstring) and get one more lp_round_bound, scaled by |g'|."""
    c = _case(M, N, K)
    dy, w = _dgrad_operands(c)
    pre = c["pre"].to(DEV)[:, :K]                                                # ldaux = K + 16
    n = _dgelu_roundings(M, dy.shape[1], K, w.stride(0), dy.stride(0))
    ref = c["X"] * c["g1"]
    dx = ops.linear_dgrad(dy, w, pre=pre)
    r, at = GE.worst(dx, ref, _dgelu_bound(c, K, n))
    _report(f"dgelu_{n}r", r, at, tile_variant)
    stored = c["g1"].float().to(LP)
    dxs = ops.linear_dgrad(dy, w, pre=stored.to(DEV), pre_is_dgelu=True)
    r, at = GE.worst(dxs, ref, _dgelu_bound(c, K, n, stored))
    _report(f"dgelu_stored_{n}r", r, at, tile_variant)


@pytest.mark.parametrize("M", [1, 63, 64, 65, 300])
def test_dgelu_column_sums_per_column(M, tile_variant):
    """cs += column sums of dx, in all three forms: |cs - (cs0 + sum_m dx[m, k])| <= (M + 8) 2^-23 (|cs0| + sum_m |dx[m, k]|) with dx the
    kernel's own stored output (the epilogues sum what they store: csrc/gemm.hip).  A slab boundary (64 rows) on each side of M; 264
    columns = ragged column tiles of both sizes; M = 300 takes the 256-tile kernels, the others the small-launch kernel or -- under
    the variants that bar it -- the register-staged kernel with its pass after the GEMM."""
    N, K = 128, 264
    c = _case(M, N, K)
    dy, w = _dgrad_operands(c)
    pre = c["pre"].to(DEV)[:, :K]
    g = torch.Generator().manual_seed(M)
    cs0 = torch.randn(K, generator=g)
    n = _dgelu_roundings(M, N, K, w.stride(0), dy.stride(0))
    dx = ops.linear_dgrad(dy, w, pre=pre)
    r, at = GE.worst(dx, c["X"] * c["g1"], _dgelu_bound(c, K, n))
    _report(f"dgelu_{n}r", r, at, tile_variant, f"M = {M}")
    dxd = dx.double().cpu()
    ref = cs0.double() + dxd.sum(0)
    bound = (M + 8) * GE.EPS32 * (cs0.double().abs() + dxd.abs().sum(0))
    for form, kw in (("workspace", {}), ("atomic", {"atomic_colsum": True})):
        cs = cs0.clone().to(DEV)
        dx2 = ops.linear_dgrad(dy, w, pre=pre, colsum=cs, **kw)
        assert torch.equal(dx2, dx), f"[{tile_variant}] {form}: dx differs from the launch without column sums"
        r, at = GE.worst(cs, ref, bound)
        _report("dgelu_colsum", r, at, tile_variant, f"{form}, M = {M}")
    stored = c["g1"].float().to(LP).to(DEV)
    cs = cs0.clone().to(DEV)
    dxs = ops.linear_dgrad(dy, w, pre=stored, colsum=cs, pre_is_dgelu=True)
    dsd = dxs.double().cpu()
    r, at = GE.worst(cs, cs0.double() + dsd.sum(0), (M + 8) * GE.EPS32 * (cs0.double().abs() + dsd.abs().sum(0)))
    _report("dgelu_colsum", r, at, tile_variant, f"stored gelu', M = {M}")


# ------------------------------------------------------------------------------------------------ weight gradient
def _wgrad_case(N, K, M):
    key = ("wgrad", N, K, M)
    if key not in _CASES:
        g = torch.Generator().manual_seed(N + 3 * K + 7 * M)
        c = {"dy": torch.randn(M, N, generator=g).to(LP), "x": torch.randn(M, K, generator=g).to(LP),
             "gw0": torch.randn(N, K, generator=g), "gb0": torch.randn(N, generator=g)}
        dyd, xd = c["dy"].double(), c["x"].double()
        c["gw"] = c["gw0"].double() + dyd.t() @ xd
        c["gw_abs"] = dyd.abs().t() @ xd.abs() + c["gw0"].double().abs()
        c["gb"] = c["gb0"].double() + dyd.sum(0)
        c["gb_abs"] = c["gb0"].double().abs() + dyd.abs().sum(0)
        _CASES[key] = c
    return _CASES[key]


def _check_wgrad(c, gw, gb, M, slices, variant, what, family="wgrad"):
    r, at = GE.worst(gw, c["gw"], (M + slices + 4) * GE.EPS32 * c["gw_abs"])
    _report(family, r, at, variant, what)
    if gb is not None:
        r, at = GE.worst(gb, c["gb"], (M + slices + 4) * GE.EPS32 * c["gb_abs"])
        _report(family + "_bias", r, at, variant, what)


@pytest.mark.parametrize("N,K,M", [(256, 256, 65),       # one 256-tile with a ragged reduction
                                   (264, 520, 513),      # ragged tiles, and 9 k-tiles so that a split is real
                                   (136, 200, 130)])     # register-staged
def test_wgrad_per_element(N, K, M, tile_variant):
    """gw[N, K] += dy^T x and gb += dy.sum(0) on non-zero accumulators, the planner's split and splitk = 1, 2, 3:
    |gw - ref| <= (M + slices + 4) 2^-23 (|dy|^T |x| + |gw0|), |gb - ref| <= (M + slices + 4) 2^-23 (|gb0| + sum |dy|); slices as the
    plan of the launch reports them (each slice adds its partial sum to the accumulator: one more addition per slice)."""
    c = _wgrad_case(N, K, M)
    dy, x = c["dy"].to(DEV), c["x"].to(DEV)
    for splitk in (0, 1, 2, 3):
        rc, out = _plan(6, N, K, M, N, K, splitk)
        assert rc == 0 and (splitk == 0 or out[5] <= splitk)
        gw, gb = c["gw0"].clone().to(DEV), c["gb0"].clone().to(DEV)
        if splitk == 0:
            ops.linear_wgrad_accum(dy, x, gw, gb)
        else:
            ops._gemm(dy, x, gw, N, K, M, N, K, K, 1, 1, ops.EPI_ACCUM, C2=gb, splitk=splitk)
        _check_wgrad(c, gw, gb, M, out[5], tile_variant, f"splitk {splitk} ({out[5]} slices)")


@pytest.mark.parametrize("M,kernel", [(130, 3), (1281, 2)])
def test_wgrad_pair_per_element(M, kernel, tile_variant):
    """One linear_wgrad_accum_pair of (512, 256) + (256, 512), the bias gradient on the second: M = 130 takes gemm128d_wgrad_kernel
    (plan kernel 3), M = 1281 the 256-tile pair (2) -- except under the variant that forces the register-staged kernel, where the
    pair runs as two single launches."""
    cs = [_wgrad_case(512, 256, M), _wgrad_case(256, 512, M)]
    out = (ctypes.c_int * 14)()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert load().octmae_wgrad_pair_plan(512, 256, 512, 256, 256, 512, 256, 512, M, 0, cus, out) == 0
    assert out[0] == kernel, f"the pair at M = {M} was meant to reach plan kernel {kernel}, the planner says {out[0]}"
    slices = out[2]
    if tile_variant == "tile128":
        slices = max(_plan(6, 512, 256, M, 512, 256)[1][5], _plan(6, 256, 512, M, 256, 512)[1][5])
    probs = []
    for i, c in enumerate(cs):
        probs.append((c["dy"].to(DEV), c["x"].to(DEV), c["gw0"].clone().to(DEV), c["gb0"].clone().to(DEV) if i == 1 else None))
    n0 = ops.set_option("gemm_small_wgrad_launches", 0)
    ops.linear_wgrad_accum_pair(probs[0], probs[1])
    took128 = ops.set_option("gemm_small_wgrad_launches", 0) - n0
    assert took128 == (1 if kernel == 3 and tile_variant != "tile128" else 0), (tile_variant, took128)
    for c, (_, _, gw, gb) in zip(cs, probs):
        _check_wgrad(c, gw, gb, M, slices, tile_variant, f"pair, M = {M}", "wgrad_pair")


# ------------------------------------------------------------------------------------------------ delta epilogue
@pytest.mark.parametrize("M,H,HD", [(257, 8, 32), (300, 4, 64), (513, 16, 32)])
def test_dgrad_delta_per_row_and_head(M, H, HD, tile_variant):
    """octmae_linear_dgrad_delta: per (row, head) |delta + sum_j do o| <= (HD + 4) 2^-23 sum_j |do o| with do the kernel's own stored
    output, and do itself inside the plain dgrad's bound.  Where the wrapper falls back (delta is None) it is a case the planner
    declines: the forced register-staged kernel, or EPI_DELTA answered with -2."""
    C = H * HD
    c = _case(M, C, C)                                                          # dy [M, C] @ w [C, C]
    dy, w = _dgrad_operands(c)
    g = torch.Generator().manual_seed(M + H)
    o = torch.randn(M, C, generator=g).to(LP)
    do, delta = ops.linear_dgrad_delta(dy, w, o.to(DEV), H, HD)
    r, at = GE.worst(do, c["X"], GE.lp_round_bound(c["X"], U, TINY) + c["X_acc"])
    _report("delta_do", r, at, tile_variant)
    if delta is None:
        assert tile_variant == "tile128" or _plan(4, C, M, C, w.stride(0), dy.stride(0))[0] == -2, \
            f"[{tile_variant}] no delta although the planner takes the problem"
        return
    assert tile_variant != "tile128"
    prod = (do.double().cpu() * o.double()).view(M, H, HD)
    r, at = GE.worst(delta, -prod.sum(-1), (HD + 4) * GE.EPS32 * prod.abs().sum(-1).clamp_min(1e-30))
    _report("delta", r, at, tile_variant)


# ------------------------------------------------------------------------------------------------ every finite 16-bit input
_SWEEP = {}


def _same_bits_as_first_variant(name, t, variant):
    """the packed two-at-a-time forms and the scalar ones give the same bits: every variant against the first one that ran (`auto` in a
    whole run; a single variant run alone compares with itself)"""
    t = t.detach().cpu()
    first_variant, first = _SWEEP.setdefault(name, (variant, t))
    r, at = GE.bit_exact(t, first)
    assert r == 0.0, f"{name}: [{variant}] differs from [{first_variant}] at element {at}: {float(t[at])} vs {float(first[at])}"


def test_gelu_on_every_finite_input(tile_variant):
    """x = every finite value of the type as a [256, 256] matrix, w = the identity, bias = 0: every product is exact, so pre is x bit
    for bit -- except the one -0, which the fp32 sum of a -0 product and +0 products turns into +0 -- and act is gelu_f of every
    value: one rounding + 2e-5 |x| at x >= -4.2, |act| <= 6e-5 below, no NaN, finite everywhere (|gelu(x)| <= |x|).
    The ledger also keeps the worst (|act - gelu(x)| - the rounding allowance) / |x| at |x| >= 1: what of the polynomial's own error
    shows through the 16-bit store (the fp32 value is not observable; its restatement is pinned in tests/test_cpu_gemm_elem.py)."""
    xa = GE.all_finite_lp(LP)
    w = torch.eye(256).to(LP).to(DEV)
    pre, act = ops.linear_fwd(xa.to(DEV), w, torch.zeros(256, device=DEV), "gelu")
    neg0 = (xa.view(torch.int16) == -32768)
    assert int(neg0.sum()) == 1 and float(pre.cpu()[neg0].abs().max()) == 0.0
    r, at = GE.bit_exact(torch.where(neg0, xa, pre.cpu()), xa)
    assert r == 0.0, f"[{tile_variant}] pre differs from x at element {at}: x = {float(xa[at])}, pre = {float(pre[at])}"
    a = act.double().cpu()
    assert not bool(torch.isnan(a).any()) and bool(torch.isfinite(a).all()), f"[{tile_variant}] NaN or inf in act"
    ref, bound = GE.gelu_bounds(xa, U, TINY)
    r, at = GE.worst(act, ref, bound)
    _report("gelu_sweep", r, at, tile_variant, f"x = {float(xa[at])}")
    xd = xa.double()
    big = (xd.abs() >= 1) & (xd >= -4.2)
    excess = (((a - ref).abs() - GE.lp_round_bound(ref, U, TINY)) / xd.abs().clamp_min(1.0))[big].clamp_min(0.0)
    label = f"gemm_elem/gelu_sweep_poly_excess/{TAG}"
    if float(excess.max()) > _WORST.get(label, -1.0):
        _WORST[label] = float(excess.max())
        parity(label, float(excess.max()), 2e-5)
    _same_bits_as_first_variant("gelu_sweep_act", act, tile_variant)


def test_gelu_prime_on_every_finite_input(tile_variant):
    """pre = every finite value, dy[:, 0] = 1 and w[0, :] = 1 (zero elsewhere) so that X = dy @ w is 1 exactly: dx is gelu'(x) rounded
    once, |dx - gelu'(x)| <= lp_round_bound(gelu'(x)) + 1e-6 (dgelu_exact_f: 3e-7, and an ulp each for the hardware reciprocal and
    exp2).  The same values through the forward's store_dgelu (x through the identity): gelu' of the rounded pre-activation,
    rounded once.  Every variant the same bits."""
    xa = GE.all_finite_lp(LP)
    dy = torch.zeros(256, 256, dtype=LP); dy[:, 0] = 1
    w = torch.zeros(256, 256, dtype=LP); w[0, :] = 1
    ref, bound = GE.dgelu_bounds(xa, U, TINY)
    dx = ops.linear_dgrad(dy.to(DEV), w.to(DEV), pre=xa.to(DEV))
    r, at = GE.worst(dx, ref, bound)
    _report("dgelu_sweep", r, at, tile_variant, f"x = {float(xa[at])}")
    _same_bits_as_first_variant("dgelu_sweep_dx", dx, tile_variant)
    dg, _ = ops.linear_fwd(xa.to(DEV), torch.eye(256).to(LP).to(DEV), torch.zeros(256, device=DEV), "gelu", store_dgelu=True)
    r, at = GE.worst(dg, ref, bound)
    _report("dgelu_fwd_sweep", r, at, tile_variant, f"x = {float(xa[at])}")
    _same_bits_as_first_variant("dgelu_sweep_stored", dg, tile_variant)
    r, at = GE.bit_exact(dg.cpu(), dx.cpu())
    assert r == 0.0, f"[{tile_variant}] the forward's stored gelu' and the dgrad's differ at {at}: x = {float(xa[at])}"
