"""The GEMM entry points on operands and outputs past 2^31 and 2^32 bytes -- `pytest -m gpu` on an MI355X.

The largest GEMM of the other tests is 84 MB; production hands these kernels 2.7 GB activations (the decoder's MLP at micro-batch
128).  The LDS-DMA kernels address their operands with 32-bit unsigned buffer offsets (csrc/gemm.hip: va[], vb[], a_bytes, b_bytes),
the planner admits an operand below 0xFFF00000 bytes and hands everything else to the register-staged kernel with 64-bit pointers
(csrc/gemm_plan.hpp: dma_operands_ok), and every epilogue forms its output address from an int row index.  With rows of 1024 16-bit
elements (2048 bytes) the four tiers of tests/bigoffset_ref.py::GEMM_M are: past 2^31 bytes with a ragged last tile, the last row
count the DMA kernels admit, the first they decline (the plan must name kernel 0 and the result must still be right), past 2^32.

Three placements of the large tensor: the activation OPERAND (forward x [M, 1024] @ w [256, 1024]^T, dgrad dy [M, 1024] @ w [1024, 256],
with the fused dgrad + delta or its fallback where the planner answers -2, and once as a column slice of a wider tensor), the OUTPUT
and the epilogue's `aux` (reduction length 64: epilogues 0 and 2 on [M, 1024] 16-bit outputs, 1, 3 and the rowscale form on
[M / 2, 1024] fp32 ones, dgrad x GELU' with its column sums in both forms, dgrad + delta), and both k-strided operands of the WEIGHT
GRADIENT (with the bias gradient, the planner's split and splitk = 1; the pair once).

References are float64 products of the same 16-bit operands, chunk by chunk on the device; the bounds are those of
tests/test_gpu_gemm_elements.py (tests/gemm_elem.py, restated for device tensors in tests/bigoffset_ref.py).  The weight gradients
use integer operands in {-2 .. 2}: every fp32 partial sum is an integer below 2^24, so the result must EQUAL the float64 one.  The
column sums over M rows keep the (M + 8) 2^-23 factor of the small tests: at M = 2^21 that is 0.25 of the sum of magnitudes -- twice
the textbook gamma_n = n u / (1 - n u) = 0.143 for n = 2^21, u = 2^-24, so the factor still covers any order of the additions.  At
that size the bound only catches a gross fault of the sums (a NaN, a SENTINEL, a wrong magnitude): a lost band of rows moves a sum
of ~1e6 random terms by less than it.  What guards the rows is dx itself, which the sums are taken from and which is checked element
by element, in both forms.

Every output lies between two guard bands and starts as SENTINEL; the worst |got - ref| / bound is kept per band of byte offsets
(below 2^31, up to 2^32, beyond) and goes to the parity ledger.

Variants: every case runs under all nine variants of tests/test_gpu_kernels.py::tile_variant, the forced small-launch ones included
(that kernel shares the 32-bit operand offsets and the admission limit of the 256-tile kernels: csrc/gemm_plan.hpp, gemm128_ok).
Measured on an MI355X a case takes 0.3 ... 0.7 s under `auto`; most of that is the float64 reference, which is recomputed per
variant because no float64 copy of an operand may be kept."""
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
from tests import bigoffset_ref as BR
from tests import gemm_elem as GE
from tests.test_gpu_kernels import tile_variant  # noqa: F401  (the GEMM kernel-choice fixture)

DEV = "cuda"
U = GE.LP_U[LP]
TINY = torch.finfo(LP).tiny
TAG = "f16" if LP == torch.float16 else "bf16"
F64 = torch.float64
STEP = 32768                                  # rows per reference chunk of the [*, 1024] outputs (256 MiB per float64 temporary)
TEMPS = 12 * STEP * 1024 * 8                  # stated room for a chunk's float64 temporaries
TIERS = list(BR.GEMM_M)
tiers = pytest.mark.parametrize("tier", TIERS)


def _plan(kind, NA, NB, K, lda, ldb, splitk=0):
    out = (ctypes.c_int * 13)()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rc = load().octmae_gemm_plan(kind, NA, NB, K, lda, ldb, ops._variant_bits(), splitk, 1, cus, out)
    return rc, list(out)


def _expect_kernel(plan, tier, variant, what, wgrad=False):
    """the large operand decides: an LDS-DMA kernel up to the last admitted row count (the 256-tile ones, or the small-launch kernel
    where a variant forces it: forward and dgrad only), the register-staged one with 64-bit pointers beyond"""
    rc, out = plan
    assert rc == 0, (what, tier, variant, rc)
    if tier not in ("past_2g", "last_admitted") or variant == "tile128":
        want = (0,)
    else:
        want = (3,) if variant.startswith("small") and not wgrad else (1, 2)
    assert out[0] in want, f"{what} [{tier}, {variant}]: plan kernel {out[0]}, expected one of {want}"
    return out[0]


def _expect_output_kernel(plan, tier, variant, what):
    """the large-output cases exist to run the stores (and the `aux` reads) of the LDS-DMA kernels through their per-wave descriptors
    past 2^31 and 2^32 bytes: their operands are small at every tier, so the plan must name a 256-tile kernel, or the small-launch
    kernel where a variant forces it, everywhere but under the forced register-staged kernel"""
    rc, out = plan
    assert rc == 0, (what, tier, variant, rc)
    want = (0,) if variant == "tile128" else (3,) if variant.startswith("small") else (1, 2)
    assert out[0] in want, f"{what} [{tier}, {variant}]: plan kernel {out[0]}, expected one of {want}"
    return out[0]


def _finish(label, buf_outs, per_band_by_name):
    for name, (buf, out) in buf_outs.items():
        assert BR.guards_intact(buf, out), f"{label}: a store outside {name} (guard band overwritten)"
    fails = []
    for name, pb in per_band_by_name.items():
        print(f"{label}/{name}: worst ratio per band {pb}")
        try:
            BR.record(f"{label}/{name}", pb)
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ the large tensor is the activation operand
@tiers
def test_forward_large_activation(tier, tile_variant):
    """y bf16 [M, 256] = x [M, 1024] @ w^T + b: |y - ref| <= one rounding + (K + 4) 2^-23 (|x| |w|^T + |b|) per element"""
    M, K, N = BR.GEMM_M[tier], 1024, 256
    BR.require(2 * M * K + 2 * M * N + TEMPS)
    try:
        x = BR.draw((M, K), LP, DEV, 101)
        w = BR.draw((N, K), LP, DEV, 102, scale=K ** -0.5)
        b = torch.randn(N, device=DEV)
        buf, y = BR.guarded((M, N), LP, DEV)
        _expect_kernel(_plan(0, N, M, K, K, K), tier, tile_variant, "forward")
        ops._gemm(w, x, y, N, M, K, K, K, N, 0, 0, ops.EPI_BF16, bias=b)
        wd, bd = w.double(), b.double()

        def chunk(r0, r1):
            xd = x[r0:r1].double()
            ref = xd @ wd.t() + bd
            return ref, BR.lp_round_bound(ref, U, TINY) + BR.acc_bound(xd.abs(), wd.abs(), K, bd.abs())

        pb = BR.compare(y, 2 * K, chunk)
        _finish(f"bigoffset_gemm/{TAG}/fwd_operand/{tier}/{tile_variant}", {"y": (buf, y)}, {"y": pb})
    finally:
        x = w = b = buf = y = wd = bd = chunk = None
        BR.release()


def test_forward_activation_is_a_column_slice(tile_variant):
    """the same forward with x = columns 64 .. 1087 of a [M, 1088] tensor (ld != width): rows 2176 bytes apart, past 2^31 bytes"""
    M, K, N, LD = BR.GEMM_M["past_2g"], 1024, 256, 1088
    BR.require(2 * M * LD + 2 * M * N + TEMPS)
    try:
        wide = BR.draw((M, LD), LP, DEV, 111)
        x = wide[:, 64:]
        w = BR.draw((N, K), LP, DEV, 112, scale=K ** -0.5)
        buf, y = BR.guarded((M, N), LP, DEV)
        rc, out = _plan(0, N, M, K, K, LD)
        _expect_kernel((rc, out), "past_2g", tile_variant, "forward on a column slice")
        ops._gemm(w, x, y, N, M, K, K, LD, N, 0, 0, ops.EPI_BF16)
        wd = w.double()

        def chunk(r0, r1):
            xd = x[r0:r1].double()
            ref = xd @ wd.t()
            return ref, BR.lp_round_bound(ref, U, TINY) + BR.acc_bound(xd.abs(), wd.abs(), K)

        pb = BR.compare(y, 2 * LD, chunk)
        _finish(f"bigoffset_gemm/{TAG}/fwd_operand_slice/{tile_variant}", {"y": (buf, y)}, {"y": pb})
    finally:
        wide = x = w = buf = y = wd = chunk = None
        BR.release()


@tiers
def test_dgrad_large_activation_and_delta(tier, tile_variant):
    """dx bf16 [M, 256] = dy [M, 1024] @ w [1024, 256], then octmae_linear_dgrad_delta on the same operands (H = 4, head_dim 64): where
    the planner answers -2 (an operand beyond the DMA range, the forced register-staged kernel) the entry point must leave its
    outputs untouched, and the fallback -- the plain dgrad -- is what is checked."""
    M, Nr, K, H, HD = BR.GEMM_M[tier], 1024, 256, 4, 64
    BR.require(2 * M * Nr + 3 * 2 * M * K + 4 * M * H + TEMPS)
    try:
        dy = BR.draw((M, Nr), LP, DEV, 121)
        w = BR.draw((Nr, K), LP, DEV, 122, scale=Nr ** -0.5)
        o = BR.draw((M, K), LP, DEV, 123)
        buf, dx = BR.guarded((M, K), LP, DEV)
        _expect_kernel(_plan(1, K, M, Nr, K, Nr), tier, tile_variant, "dgrad")
        ops._gemm(w, dy, dx, K, M, Nr, K, Nr, K, 1, 0, ops.EPI_BF16)
        wd = w.double()

        def chunk(r0, r1):
            dyd = dy[r0:r1].double()
            ref = dyd @ wd
            return ref, BR.lp_round_bound(ref, U, TINY) + BR.acc_bound(dyd.abs(), wd.abs().t(), Nr)

        pbs = {"dx": BR.compare(dx, 2 * Nr, chunk)}
        bufs = {"dx": (buf, dx)}
        # the fused dgrad + delta
        buf2, dx2 = BR.guarded((M, K), LP, DEV)
        bufd, delta = BR.guarded((M, H), torch.float32, DEV)
        bufs.update({"dx_delta": (buf2, dx2), "delta": (bufd, delta)})
        st = ops._stream()
        rc = load().octmae_linear_dgrad_delta(w.data_ptr(), dy.data_ptr(), dx2.data_ptr(), o.data_ptr(), delta.data_ptr(), M, Nr, K, K, Nr,
                                              K, K, H, HD, ops._variant_bits(), *ops._split_ws_for(st), st)
        prc, _ = _plan(4, K, M, Nr, K, Nr)
        takes = tier in ("past_2g", "last_admitted") and tile_variant != "tile128"
        assert rc == prc == (0 if takes else -2), (rc, prc, tier, tile_variant)
        if rc == -2:
            torch.cuda.synchronize()
            assert bool((buf2 == BR.SENTINEL).all()) and bool((bufd == BR.SENTINEL).all()), "a declined call wrote to its outputs"
            ops._gemm(w, dy, dx2, K, M, Nr, K, Nr, K, 1, 0, ops.EPI_BF16)                 # the fallback of ops.linear_dgrad_delta
            assert torch.equal(dx2, dx)
            delta = None
        else:
            pbs["dx_delta"] = BR.compare(dx2, 2 * Nr, chunk)

            def dchunk(r0, r1):
                prod = (dx2[r0:r1].double() * o[r0:r1].double()).view(r1 - r0, H, HD)
                return -prod.sum(-1), (HD + 4) * GE.EPS32 * prod.abs().sum(-1).clamp_min(1e-30)

            pbs["delta"] = BR.compare(delta, 2 * Nr, dchunk)
        _finish(f"bigoffset_gemm/{TAG}/dgrad_operand/{tier}/{tile_variant}", bufs, pbs)
    finally:
        dy = w = o = buf = dx = buf2 = dx2 = bufd = delta = wd = chunk = dchunk = bufs = None
        BR.release()


# ------------------------------------------------------------------------------------------------ the large tensors are the outputs and aux
@tiers
def test_large_16bit_outputs_of_the_forward_epilogues(tier, tile_variant):
    """epilogue 0: y [M, 1024]; epilogue 2: pre (= y, bit for bit) and act = gelu(pre) under the activation's own bound"""
    M, K, N = BR.GEMM_M[tier], 64, 1024
    BR.require(2 * M * K + 3 * 2 * M * N + TEMPS)
    try:
        x = BR.draw((M, K), LP, DEV, 131)
        w = BR.draw((N, K), LP, DEV, 132, scale=K ** -0.5)
        b = torch.randn(N, device=DEV)
        (bufy, y), (bufp, pre), (bufa, act) = (BR.guarded((M, N), LP, DEV) for _ in range(3))
        _expect_output_kernel(_plan(0, N, M, K, K, K), tier, tile_variant, "forward, 16-bit output")
        ops._gemm(w, x, y, N, M, K, K, K, N, 0, 0, ops.EPI_BF16, bias=b)
        ops._gemm(w, x, pre, N, M, K, K, K, N, 0, 0, ops.EPI_GELU, C2=act, bias=b)
        wd, bd = w.double(), b.double()

        def chunk(r0, r1):
            xd = x[r0:r1].double()
            ref = xd @ wd.t() + bd
            return ref, BR.lp_round_bound(ref, U, TINY) + BR.acc_bound(xd.abs(), wd.abs(), K, bd.abs())

        pbs = {"y": BR.compare(y, 2 * N, chunk, step=STEP),
               "pre_vs_y": BR.compare(pre, 2 * N, lambda r0, r1: (y[r0:r1], None), step=STEP),
               "act": BR.compare(act, 2 * N, lambda r0, r1: BR.gelu_bounds(pre[r0:r1], U, TINY), step=STEP)}
        _finish(f"bigoffset_gemm/{TAG}/out16/{tier}/{tile_variant}", {"y": (bufy, y), "pre": (bufp, pre), "act": (bufa, act)}, pbs)
    finally:
        x = w = b = bufy = y = bufp = pre = bufa = act = wd = bd = chunk = None
        BR.release()


@tiers
def test_large_fp32_outputs_of_the_forward_epilogues(tier, tile_variant):
    """epilogue 1 (f32), 3 (residual `aux` [M', 1024] fp32) and octmae_linear_resid_rowscale at M' = M / 2 rows of 4096 bytes:
    |y - ref| <= (K + 4) 2^-23 (|x| |w|^T + |b| [+ |res|]), the rowscale form scaled by the row's |scale|; a dropped row is the
    residual bit for bit."""
    M, K, N = BR.f32_rows(BR.GEMM_M[tier]), 64, 1024
    BR.require(2 * M * K + 2 * 4 * M * N + TEMPS)
    try:
        x = BR.draw((M, K), LP, DEV, 141)
        w = BR.draw((N, K), LP, DEV, 142, scale=K ** -0.5)
        b = torch.randn(N, device=DEV)
        res = BR.draw((M, N), torch.float32, DEV, 143)
        sc = torch.tensor([0.0, 1.25, 2.0], device=DEV)[torch.randint(0, 3, (M,), device=DEV)]
        buf, out = BR.guarded((M, N), torch.float32, DEV)
        wd, bd = w.double(), b.double()
        state = {}

        def chunk(r0, r1):
            xd = x[r0:r1].double()
            yd, ya = xd @ wd.t() + bd, xd.abs() @ wd.abs().t() + bd.abs()
            rd = res[r0:r1].double()
            if state["form"] == "f32":
                return yd, (K + 4) * GE.EPS32 * ya
            bound = (K + 4) * GE.EPS32 * (ya + rd.abs())
            if state["form"] == "resid":
                return rd + yd, bound
            s = sc[r0:r1].double().unsqueeze(1)
            return rd + s * yd, torch.where(s != 0, s.abs() * bound, torch.full_like(bound, 1e-300))      # dropped rows: equality

        pbs = {}
        st = ops._stream()
        _expect_output_kernel(_plan(0, N, M, K, K, K), tier, tile_variant, "forward, fp32 output")
        for form in ("f32", "resid", "rowscale"):
            buf.fill_(BR.SENTINEL)
            if form == "f32":
                ops._gemm(w, x, out, N, M, K, K, K, N, 0, 0, ops.EPI_F32, bias=b)
            elif form == "resid":
                ops._gemm(w, x, out, N, M, K, K, K, N, 0, 0, ops.EPI_RESID, bias=b, aux=res, ldaux=N)
            else:
                ops.call("octmae_linear_resid_rowscale", w.data_ptr(), x.data_ptr(), out.data_ptr(), b.data_ptr(), res.data_ptr(),
                         sc.data_ptr(), 1, N, M, K, K, K, N, N, ops._variant_bits(), *ops._split_ws_for(st), st)
            state["form"] = form
            pbs[form] = BR.compare(out, 4 * N, chunk, step=STEP)
            assert BR.guards_intact(buf, out), f"{form}: a store outside the output"
        _finish(f"bigoffset_gemm/{TAG}/out32/{tier}/{tile_variant}", {"out": (buf, out)}, pbs)
    finally:
        x = w = b = res = sc = buf = out = wd = bd = chunk = None
        BR.release()


@tiers
def test_large_output_of_dgrad_times_gelu_prime_with_column_sums(tier, tile_variant):
    """dx [M, 1024] = (dy [M, 64] @ w [64, 1024]) * gelu'(pre [M, 1024]) through epilogue 4 with the column sums by atomics and through
    octmae_linear_dgrad_dgelu (per-slab workspace + fold): dx under the bound of tests/test_gpu_gemm_elements.py (two roundings where
    the plan names an LDS-transposing kernel), both forms the same dx, the column sums against the sums of the stored dx."""
    M, Nr, K = BR.GEMM_M[tier], 64, 1024
    rows_ws = load().octmae_dgelu_colsum_ws_rows(M)
    BR.require(2 * M * Nr + 3 * 2 * M * K + 4 * rows_ws * K + TEMPS)
    try:
        dy = BR.draw((M, Nr), LP, DEV, 151)
        w = BR.draw((Nr, K), LP, DEV, 152, scale=Nr ** -0.5)
        pre = BR.draw((M, K), LP, DEV, 153)
        (buf1, dx1), (buf2, dx2) = (BR.guarded((M, K), LP, DEV) for _ in range(2))
        cs0 = torch.randn(K, device=DEV)
        cs_atomic, cs_ws = cs0.clone(), cs0.clone()
        kernel = _expect_output_kernel(_plan(2, K, M, Nr, K, Nr), tier, tile_variant, "dgrad times gelu'")
        roundings = 1 if kernel == 0 else 2
        ops._gemm(w, dy, dx1, K, M, Nr, K, Nr, K, 1, 0, ops.EPI_DGELU, C2=cs_atomic, aux=pre, ldaux=K)
        ws = torch.empty((max(rows_ws, 1), K), dtype=torch.float32, device=DEV)
        st = ops._stream()
        ops.call("octmae_linear_dgrad_dgelu", w.data_ptr(), dy.data_ptr(), dx2.data_ptr(), pre.data_ptr(), ws.data_ptr(), cs_ws.data_ptr(),
                 M, Nr, K, K, Nr, K, K, ops._variant_bits(), *ops._split_ws_for(st), st)
        wd = w.double()
        sums = {"s": torch.zeros(K, dtype=F64, device=DEV), "a": torch.zeros(K, dtype=F64, device=DEV)}

        def chunk(r0, r1):
            dyd = dy[r0:r1].double()
            X, g1 = dyd @ wd, BR.dgelu64(pre[r0:r1])
            Xacc = BR.acc_bound(dyd.abs(), wd.abs().t(), Nr)
            bound = BR.lp_round_bound(X * g1, U, TINY) + g1.abs() * Xacc + X.abs() * 1e-6
            if roundings == 2:
                bound = bound + g1.abs() * BR.lp_round_bound(X, U, TINY)
            got = dx1[r0:r1].double()
            sums["s"] += got.sum(0)
            sums["a"] += got.abs().sum(0)
            return X * g1, bound

        pbs = {f"dx_{roundings}r": BR.compare(dx1, 2 * K, chunk, step=STEP),
               "dx_ws_vs_atomic": BR.compare(dx2, 2 * K, lambda r0, r1: (dx1[r0:r1], None), step=STEP)}
        _finish(f"bigoffset_gemm/{TAG}/dgelu_out/{tier}/{tile_variant}", {"dx_atomic": (buf1, dx1), "dx_ws": (buf2, dx2)}, pbs)
        ref = cs0.double() + sums["s"]
        bound = (M + 8) * GE.EPS32 * (cs0.double().abs() + sums["a"])
        for name, cs in (("atomic", cs_atomic), ("workspace", cs_ws)):
            r, at = GE.worst(cs, ref, bound)
            BR.record(f"bigoffset_gemm/{TAG}/dgelu_colsum_{name}/{tier}/{tile_variant}", [r, None, None])
    finally:
        dy = w = pre = buf1 = dx1 = buf2 = dx2 = cs0 = cs_atomic = cs_ws = ws = wd = sums = chunk = None
        BR.release()


@tiers
def test_large_output_of_dgrad_delta(tier, tile_variant):
    """octmae_linear_dgrad_delta with dX [M, 1024] and O [M, 1024] large (H = 16, head_dim 64, reduction 64): dX under the plain
    dgrad's bound, delta [M, 16] per (row, head) under (HD + 4) 2^-23 sum |dX O|.  The forced register-staged kernel has no such
    epilogue: -2, outputs untouched."""
    M, Nr, K, H, HD = BR.GEMM_M[tier], 64, 1024, 16, 64
    BR.require(2 * M * Nr + 2 * 2 * M * K + 4 * M * H + TEMPS)
    try:
        dy = BR.draw((M, Nr), LP, DEV, 161)
        w = BR.draw((Nr, K), LP, DEV, 162, scale=Nr ** -0.5)
        o = BR.draw((M, K), LP, DEV, 163)
        buf, dx = BR.guarded((M, K), LP, DEV)
        bufd, delta = BR.guarded((M, H), torch.float32, DEV)
        st = ops._stream()
        rc = load().octmae_linear_dgrad_delta(w.data_ptr(), dy.data_ptr(), dx.data_ptr(), o.data_ptr(), delta.data_ptr(), M, Nr, K, K, Nr,
                                              K, K, H, HD, ops._variant_bits(), *ops._split_ws_for(st), st)
        prc, pout = _plan(4, K, M, Nr, K, Nr)
        assert rc == prc == (-2 if tile_variant == "tile128" else 0), (rc, prc)
        if prc == 0:
            _expect_output_kernel((prc, pout), tier, tile_variant, "dgrad with delta")
        torch.cuda.synchronize()
        if rc == -2:
            assert bool((buf == BR.SENTINEL).all()) and bool((bufd == BR.SENTINEL).all()), "a declined call wrote to its outputs"
            return
        wd = w.double()

        def chunk(r0, r1):
            dyd = dy[r0:r1].double()
            ref = dyd @ wd
            return ref, BR.lp_round_bound(ref, U, TINY) + BR.acc_bound(dyd.abs(), wd.abs().t(), Nr)

        def dchunk(r0, r1):
            prod = (dx[r0:r1].double() * o[r0:r1].double()).view(r1 - r0, H, HD)
            return -prod.sum(-1), (HD + 4) * GE.EPS32 * prod.abs().sum(-1).clamp_min(1e-30)

        pbs = {"dx": BR.compare(dx, 2 * K, chunk, step=STEP), "delta": BR.compare(delta, 2 * K, dchunk, step=STEP)}
        _finish(f"bigoffset_gemm/{TAG}/delta_out/{tier}/{tile_variant}", {"dx": (buf, dx), "delta": (bufd, delta)}, pbs)
    finally:
        dy = w = o = buf = dx = bufd = delta = wd = chunk = dchunk = None
        BR.release()


# ------------------------------------------------------------------------------------------------ weight gradient
def _wgrad_reference(dy, x):
    """float64 dy^T @ x and the column sums of dy, chunk by chunk"""
    gw = torch.zeros((dy.shape[1], x.shape[1]), dtype=F64, device=DEV)
    gb = torch.zeros(dy.shape[1], dtype=F64, device=DEV)
    for r0, r1 in BR.chunks(dy.shape[0]):
        d = dy[r0:r1].double()
        gw += d.t() @ x[r0:r1].double()
        gb += d.sum(0)
    return gw, gb


def _exact(label, got, ref):
    wrong = got.double() != ref
    n = int(wrong.sum())
    print(f"{label}: {n} of {wrong.numel()} elements differ from float64")
    from tests.conftest import parity
    parity(label, float(n), 0.0)


@tiers
def test_wgrad_large_operands_equal_float64(tier, tile_variant):
    """gw f32 [1024, 1024] += dy [M, 1024]^T @ x [M, 1024] and gb += column sums of dy, on accumulators that start at 3 and 5, with the
    planner's split and with splitk = 1: integer operands, so every element EQUALS the float64 result."""
    M, N, K = BR.GEMM_M[tier], 1024, 1024
    assert BR.exact_sum_limit_ok(M)
    BR.require(2 * M * N + 2 * M * K + 3 * 8 * BR.CHUNK * 1024 + (64 << 20))
    try:
        dy = BR.draw_int((M, N), LP, DEV, 171)
        x = BR.draw_int((M, K), LP, DEV, 172)
        gw_ref, gb_ref = _wgrad_reference(dy, x)
        assert float(gw_ref.abs().max()) + 3 < 1 << 24
        for splitk in (0, 1):
            k = _expect_kernel(_plan(6, N, K, M, N, K, splitk), tier, tile_variant, f"wgrad splitk {splitk}", wgrad=True)
            (bufw, gw), (bufb, gb) = BR.guarded((N, K), torch.float32, DEV), BR.guarded((N,), torch.float32, DEV)
            gw.fill_(3.0)
            gb.fill_(5.0)
            ops._gemm(dy, x, gw, N, K, M, N, K, K, 1, 1, ops.EPI_ACCUM, C2=gb, splitk=splitk)
            label = f"bigoffset_gemm/{TAG}/wgrad/{tier}/{tile_variant}/splitk{splitk}_kernel{k}"
            assert BR.guards_intact(bufw, gw) and BR.guards_intact(bufb, gb), f"{label}: a store outside the accumulators"
            _exact(label + "/gw_mismatches", gw, gw_ref + 3.0)
            _exact(label + "/gb_mismatches", gb, gb_ref + 5.0)
    finally:
        dy = x = gw_ref = gb_ref = bufw = gw = bufb = gb = None
        BR.release()


def test_wgrad_pair_large_operands_equal_float64(tile_variant):
    """octmae_wgrad_accum_pair once, past 2^31 bytes: (dy, x) and (x, dy) as the two problems of one launch, the bias gradient on the
    second.  Under the forced register-staged kernel the pair runs as two single launches (ops.linear_wgrad_accum_pair)."""
    M, N = BR.GEMM_M["past_2g"], 1024
    BR.require(2 * 2 * M * N + 3 * 8 * BR.CHUNK * 1024 + (64 << 20))
    try:
        dy = BR.draw_int((M, N), LP, DEV, 181)
        x = BR.draw_int((M, N), LP, DEV, 182)
        gw_ref, gb_ref = _wgrad_reference(dy, x)
        out = (ctypes.c_int * 14)()
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert load().octmae_wgrad_pair_plan(N, N, N, N, N, N, N, N, M, 0, cus, out) == 0 and out[0] == 2, list(out)
        (buf0, gw0), (buf1, gw1), (bufb, gb1) = (BR.guarded(s, torch.float32, DEV) for s in ((N, N), (N, N), (N,)))
        gw0.fill_(3.0)
        gw1.fill_(-2.0)
        gb1.fill_(5.0)
        ops.linear_wgrad_accum_pair((dy, x, gw0, None), (x, dy, gw1, gb1))
        label = f"bigoffset_gemm/{TAG}/wgrad_pair/past_2g/{tile_variant}"
        for b, t in ((buf0, gw0), (buf1, gw1), (bufb, gb1)):
            assert BR.guards_intact(b, t), f"{label}: a store outside the accumulators"
        _exact(label + "/gw0_mismatches", gw0, gw_ref + 3.0)
        _exact(label + "/gw1_mismatches", gw1, gw_ref.t() - 2.0)
        xsum = torch.zeros(N, dtype=F64, device=DEV)
        for r0, r1 in BR.chunks(M):
            xsum += x[r0:r1].double().sum(0)
        _exact(label + "/gb1_mismatches", gb1, xsum + 5.0)
    finally:
        dy = x = gw_ref = gb_ref = buf0 = gw0 = buf1 = gw1 = bufb = gb1 = xsum = None
        BR.release()


def test_wgrad_entry_points_decline_an_accumulator_beyond_the_descriptor_range():
    """-1 before any launch where the fp32 accumulator [NA][ldc] would pass 2^32 bytes (the unsplit epilogue reaches it through one
    buffer descriptor): real small buffers, the status code, outputs that keep their sentinel"""
    lib, st = load(), ops._stream()
    a = torch.ones((8, 64), dtype=LP, device=DEV)
    gw = torch.full((64, 64), BR.SENTINEL, device=DEV)
    p = lambda t: t.data_ptr()      # noqa: E731
    calls = [lib.octmae_gemm_bf16(p(a), p(a), p(gw), None, None, None, 32768, 64, 8, 32768, 64, 32768, 0, 1, 1, ops.EPI_ACCUM, 1, st),
             lib.octmae_gemm_bf16(p(a), p(a), p(gw), None, None, None, 64, 64, 8, 64, 64, 1 << 24, 0, 1, 1, ops.EPI_ACCUM, 0, st),
             lib.octmae_wgrad_accum_pair(p(a), p(a), p(gw), None, 32768, 256, 32768, 256, 32768, p(a), p(a), p(gw), None, 256, 256, 256, 256, 256,
                                         8, 0, st)]
    torch.cuda.synchronize()
    assert calls == [-1, -1, -1], calls
    assert bool((gw == BR.SENTINEL).all())
    assert lib.octmae_gemm_bf16(p(a), p(a), p(gw), None, None, None, 64, 64, 8, 64, 64, 64, 0, 1, 1, ops.EPI_ACCUM, 1, st) == 0
    torch.cuda.synchronize()
    assert not bool((gw == BR.SENTINEL).any())
