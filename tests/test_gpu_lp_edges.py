"""Edges of the 16-bit operand type, kernel by kernel, on whichever library OCTMAE_LIB selects (bfloat16 in the normal session, IEEE
half in the child of tests/test_gpu_f16_kernels.py).

Every bound is written in units of the operand's unit roundoff U (2^-9 bfloat16, 2^-12 half), so the same test is as sharp on both
builds.  Three groups:
  * range: every 16-bit output equals torch's round-to-nearest-even cast of the kernel's own fp32 value, bit for bit, on values that
    straddle the type's largest number (half 65 504 / 65 519 / 65 520 / 7e4; bfloat16 the matching ones near 3.39e38) -- inf included;
  * subnormal operands: the MFMA keeps them (probe), and a GEMM / an attention whose operands / P mostly lie below the type's smallest
    normal number stay at fp64 on the same rounded operands;
  * the optimistic attention forward on rows whose logits all sit far below (or above) zero, and one ragged shape per kernel family at
    the u scale, recorded in the parity ledger (tests/conftest.py::parity).  Bounds = the larger of the two builds' measured values
    x 1.5 (MI355X): operand-limited quantities measure the same number of U on both builds (half 8 x below bfloat16 in absolute
    terms); fp32-limited ones (epilogues 1 / 3 / 5, LayerNorm dx, slice pool, AdamW) the same absolute error, so 8 x more U on half.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import ops
    from octcubem_amd._lib import call, load
    from octcubem_amd.optim import _MultiTensorTable
    LP = ops.BF16
else:
    LP = torch.bfloat16
from oracle import mae3d_ref as O
from tests.conftest import parity
from tests.test_gpu_kernels import attn_ref, rel, tile_variant  # noqa: F401  (tile_variant: the GEMM kernel-choice fixture)

DEV = "cuda"
IS_F16 = LP == torch.float16
TAG = "f16" if IS_F16 else "bf16"
U = 2.0 ** -12 if IS_F16 else 2.0 ** -9           # unit roundoff of the operand type
LP_MAX = torch.finfo(LP).max
LP_TINY = torch.finfo(LP).tiny                    # smallest normal number
F32_MAX = torch.finfo(torch.float32).max


def _f32_bits(b):
    return torch.tensor([b], dtype=torch.int32).view(torch.float32).item()


def edge_values():
    """fp32 values that straddle the type's largest number (both signs), plus ordinary and small ones."""
    if IS_F16:
        big = [65504.0, 65519.0, 65520.0, 65535.0, 65536.0, 7e4, 65488.0, 65500.0, 1e5]
        small = [2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26, 2.0 ** -15, 6.0e-5, 1e-7]
    else:
        big = [LP_MAX, _f32_bits(0x7F7F7FFF), _f32_bits(0x7F7F8000), F32_MAX, 3.0e38, _f32_bits(0x7F7E8000), 1e38]
        small = [1.2e-38, 2.0 ** -125, 3.0e-38]
    vals = big + small + [1.0, 0.1, 3.14159, 0.0]
    return torch.tensor(vals + [-v for v in vals], dtype=torch.float32)


def bits_equal(a, b):
    assert a.dtype == b.dtype == LP
    return torch.equal(a.contiguous().view(torch.int16).cpu(), b.contiguous().view(torch.int16).cpu())


def _show(got, exp):
    bad = (got.float().cpu() != exp.float().cpu()).nonzero()[:8]
    return f"{len(bad)} differing, first at {bad.tolist()}"


def _straddles(t):
    """the tensor of 16-bit outputs reaches inf and the type's largest finite number: the test did test the edge"""
    t = t.float()
    return bool(torch.isinf(t).any()) and bool((t.abs() == LP_MAX).any())


def _tiled(n, g):
    e = edge_values()
    x = torch.randn(n, generator=g)
    x[: min(n, e.numel())] = e[: min(n, e.numel())]
    return x


# ------------------------------------------------------------------------------------------------ range of every 16-bit output
@pytest.mark.parametrize("n", [len(edge_values()), 1001, 65536 * 2 + 7])
def test_cast_rounds_to_nearest_even_into_inf(n):
    x = _tiled(n, torch.Generator().manual_seed(n)).to(DEV)
    got = ops.cast_bf16(x)
    exp = x.to(LP)
    assert bits_equal(got, exp), _show(got, exp)
    assert _straddles(got)


def test_cast_rowscale_rounds_to_nearest_even_into_inf():
    e = edge_values()
    R, D, per = 12, 64, 2
    x = torch.randn(R, D, generator=torch.Generator().manual_seed(1))
    x[:, : e.numel()] = e
    x = x.to(DEV)
    sc = torch.tensor([1.0, 0.5, 1.0 / 0.8, 0.0, 1.0, 2.0], device=DEV)
    got = ops.cast_bf16_rowscale(x, sc, per)
    exp = (x * sc.repeat_interleave(per).unsqueeze(1)).to(LP)
    assert bits_equal(got, exp), _show(got, exp)
    assert _straddles(got)


def _guarded_lp(n, guard=4096):
    """(whole buffer, the n 16-bit elements in its middle): guard zones of a sentinel on either side"""
    buf = torch.full((n + 2 * guard,), 0x5A5A, dtype=torch.int16, device=DEV)
    return buf, buf[guard:guard + n].view(LP)


def _guards_intact(buf, n, guard=4096):
    return bool((buf[:guard] == 0x5A5A).all()) and bool((buf[guard + n:] == 0x5A5A).all())


def test_cast_past_the_grid_cap_takes_the_unrolled_loop_and_both_tails():
    """octmae_cast_f32_bf16 runs at most 512 workgroups of 256 lanes, 8 elements per lane and trip.  n / 8 = 7 x 512 x 256 + 77: the 77
    lowest lanes take two trips of the loop that keeps four loads in flight and none of the single-load loop, every other lane one
    trip of the first and three of the second; 5 elements after the last whole 8 are the scalar tail."""
    lanes = 512 * 256
    n = 8 * (4 * lanes + 3 * lanes + 77) + 5
    x = _tiled(n, torch.Generator().manual_seed(3)).to(DEV)
    buf, out = _guarded_lp(n)
    call("octmae_cast_f32_bf16", x.data_ptr(), out.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    exp = x.to(LP)
    assert _guards_intact(buf, n)
    assert bits_equal(out, exp), _show(out, exp)
    assert bits_equal(ops.cast_bf16(x), exp)


def test_cast_rowscale_past_the_grid_cap():
    """octmae_cast_rowscale_f32_bf16: at most 4096 workgroups of 256 lanes, one 8-element chunk per lane and trip.  Rows of one chunk
    (D = 8), 300 more rows than lanes: a second trip for one workgroup and 44 lanes of the next, with another row's scale."""
    R, D, per = 4096 * 256 + 300, 8, 4
    g = torch.Generator().manual_seed(4)
    x = _tiled(R * D, g).view(R, D).to(DEV)
    sc = (torch.rand(R // per, generator=g) + 0.5).to(DEV)
    buf, out = _guarded_lp(R * D)
    call("octmae_cast_rowscale_f32_bf16", x.data_ptr(), sc.data_ptr(), out.data_ptr(), R, D, per, torch.cuda.current_stream().cuda_stream)
    exp = (x * sc.repeat_interleave(per).unsqueeze(1)).to(LP)
    assert _guards_intact(buf, R * D)
    assert bits_equal(out.view(R, D), exp), _show(out.view(R, D), exp)
    assert bits_equal(ops.cast_bf16_rowscale(x, sc, per), exp)


def test_gather_rows_cast_rounds_to_nearest_even_into_inf():
    e = edge_values()
    B, rows, D, n = 3, 9, 64, 6
    g = torch.Generator().manual_seed(5)
    src = torch.randn(B, rows, D, generator=g)
    src.view(-1)[: e.numel()] = e
    src[1, 1:1 + e.numel() // D + 1].view(-1)[: e.numel()] = e.flip(0)
    src = src.to(DEV)
    ids = torch.stack([torch.randperm(rows - 1, generator=g)[:n] for _ in range(B)])
    ids[:, 0] = -1                                                   # the cls row (source row 0)
    ids[1, 1] = 0
    ids = ids.to(DEV)
    out = torch.empty(B * n, D, dtype=LP, device=DEV)
    call("octmae_gather_rows_cast", src.data_ptr(), ids.data_ptr(), out.data_ptr(), B, n, rows, D, torch.cuda.current_stream().cuda_stream)
    exp = torch.gather(src, 1, (1 + ids).unsqueeze(-1).expand(-1, -1, D)).reshape(B * n, D).to(LP)
    assert bits_equal(out, exp), _show(out, exp)
    assert _straddles(out)


def _overflow_gemm(M, N, K, g):
    """x @ w.T + bias whose fp32 results straddle the type's largest number: the bias carries the edge values, every third row of x is
    zero (those rows are the edge values exactly), the others add a small product"""
    e = edge_values()
    bias = e.repeat(N // e.numel() + 1)[:N].clone()
    x = (torch.randn(M, K, generator=g) * 1e-2).to(LP)
    x[::3] = 0
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(LP)
    return x.to(DEV), w.to(DEV), bias.to(DEV)


@pytest.mark.parametrize("M,N,K", [(333, 264, 64), (1281, 384, 128)])
def test_gemm_16bit_epilogues_round_into_inf_and_fp32_ones_stay_finite(M, N, K, tile_variant):
    """Epilogue 0 (C16 = the 16-bit cast of C32, bit for bit, inf included), epilogue 2 (pre = the same cast; act = gelu of that
    pre-activation: +inf above the type, zero below it -- not -inf), and the fp32 epilogues 1, 3 and 5 of the same problem: finite and
    at fp32 accuracy."""
    g = torch.Generator().manual_seed(M + N)
    x, w, bias = _overflow_gemm(M, N, K, g)
    ref = x.double() @ w.double().t() + bias.double()
    y32 = ops.linear_fwd(x, w, bias, "f32")
    assert torch.isfinite(y32).all() and rel(y32, ref) < 2e-6
    y16 = ops.linear_fwd(x, w, bias, "bf16")
    assert bits_equal(y16, y32.to(LP)), _show(y16, y32.to(LP))
    assert _straddles(y16)
    pre, act = ops.linear_fwd(x, w, bias, "gelu")
    assert bits_equal(pre, y16)
    a, p = act.double().cpu(), pre.double().cpu()
    assert not torch.isnan(a).any()
    assert bool((a[p == math.inf] == math.inf).all())
    assert float(a[p < -4.2].abs().max()) <= 1e-4                    # |gelu(x)| < 6e-5 below -4.2; -inf or -|x| 1e-5 is a bug
    fin = torch.isfinite(p) & (p >= -4.2)
    gref = torch.nn.functional.gelu(p[fin])                          # one rounding + the polynomial's |Phi error| <= 1.4e-5
    assert float(((a[fin] - gref).abs() - 2 * U * gref.abs() - 6e-5 * (1 + p[fin].abs())).max()) <= 0
    res = torch.zeros(M, N, device=DEV)
    yr = ops.linear_fwd(x, w, bias, "resid", res=res)
    assert torch.isfinite(yr).all() and rel(yr, ref) < 2e-6
    # epilogue 5 (weight gradient, fp32 accumulate) into an accumulator that holds the edge values
    dy = (torch.randn(M, N, generator=g) * 1e-2).to(LP).to(DEV)
    gw0 = bias.repeat(K, 1).t().contiguous()
    gw = gw0.clone()
    ops.linear_wgrad_accum(dy, x, gw)
    gref_w = gw0.double() + dy.double().t() @ x.double()
    assert torch.isfinite(gw).all() and rel(gw, gref_w) < 2e-6


def test_layernorm_backward_16bit_copy_rounds_into_inf():
    e = edge_values()
    M, D = 9, 256
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(M, D, generator=g) + 0.5).to(DEV)
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).to(DEV)
    beta = torch.zeros(D, device=DEV)
    dy = (torch.randn(M, D, generator=g) * 1e-3).to(LP).to(DEV)
    dres = torch.randn(M, D, generator=g)
    dres.view(-1)[: e.numel()] = e
    dres[5, : e.numel()] = e.flip(0)
    dres = dres.to(DEV)
    _, mean, rstd = ops.layernorm_fwd(x, gamma, beta, 1e-6)
    dx, dxb = ops.layernorm_bwd(dy, x, mean, rstd, gamma, None, None, dres=dres, want_bf16=True)
    assert bits_equal(dxb, dx.to(LP)), _show(dxb, dx.to(LP))
    assert _straddles(dxb)


@pytest.mark.parametrize("cls", [False, True], ids=["mean", "cls"])
def test_slice_pool_backward_16bit_copy_rounds_into_inf(cls):
    """dout scaled so that |dx| reaches 1.3 x the type's largest number (at most fp32's); small-variance rows keep rstd near 1e3, so
    the kernel's own reductions stay far inside fp32 on both builds."""
    S, T, D, B = 2, 2, 64, 2          # T = 2: in mean mode dx of the one patch token is dpooled itself (no larger intermediate)
    g = torch.Generator().manual_seed(3 + int(cls))
    x = (0.5 + 1e-4 * torch.randn(B * S, T, D, generator=g)).to(DEV)
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).to(DEV)
    beta = torch.zeros(D, device=DEV)
    dout = torch.randn(B, D, generator=g).to(DEV)
    _, pooled, mean, rstd = ops.slice_pool_fwd(x, gamma, beta, 1e-6, S, cls)
    dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    dx1, _ = ops.slice_pool_bwd(dout, pooled, mean, rstd, gamma, T, S, cls, dg, db)
    target = min(1.3 * LP_MAX, 3.40e38)                  # bfloat16: above its rounding midpoint 3.3961e38, below FLT_MAX 3.4028e38
    dout = dout * (target / float(dx1.abs().max()))
    dx, dxb = ops.slice_pool_bwd(dout, pooled, mean, rstd, gamma, T, S, cls, dg, db, want_bf16=True)
    assert torch.isfinite(dx).all()
    assert bits_equal(dxb, dx.to(LP)), _show(dxb, dx.to(LP))
    assert bool(torch.isinf(dxb.float()).any()) and bool((dxb.float().abs() < LP_MAX).logical_and(dxb.float().abs() > 0.5 * LP_MAX).any())


def test_mse_backward_dpred_rounds_into_inf():
    """dpred = coef * mask * (pred - target) with coef = mask = 1 and a zero image: the fp32 value is pred itself"""
    B, C, T, H, W, u, p = 2, 1, 6, 32, 32, 3, 16
    L = (T // u) * (H // p) * (W // p)
    PD = u * p * p * C
    g = torch.Generator().manual_seed(2)
    pred = torch.randn(B, L + 1, PD, generator=g)
    e = edge_values()
    pred[0, 1:].reshape(-1)[: e.numel()] = e
    pred[1, 3, : e.numel()] = e.flip(0)
    pred = pred.to(DEV)
    imgs = torch.zeros(B, C, T, H, W, device=DEV)
    mask = torch.ones(B, L, device=DEV)
    coef = torch.ones(1, device=DEV)
    dpred = torch.full((B, L + 1, PD), 7.0, dtype=LP, device=DEV)
    call("octmae_mse_bwd", pred.data_ptr(), imgs.data_ptr(), None, mask.data_ptr(), coef.data_ptr(), dpred.data_ptr(), B, C, T, H, W, u, p,
         L, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bits_equal(dpred[:, 1:], pred[:, 1:].to(LP)), _show(dpred[:, 1:], pred[:, 1:].to(LP))
    assert float(dpred[:, 0].float().abs().max()) == 0.0
    assert _straddles(dpred)


def test_adamw_operand_copy_rounds_into_inf():
    """the 16-bit copy octmae_mt_adamw_fused writes through lp_table = the cast of the updated fp32 parameter, bit for bit"""
    g = torch.Generator().manual_seed(4)
    e = edge_values()
    ps = [torch.randn(3000, generator=g), torch.randn(64, 33, generator=g)]
    ps[0][: e.numel()] = e
    ps[1].view(-1)[: e.numel()] = e.flip(0)
    ps = [p.to(DEV) for p in ps]
    gs = [torch.randn(p.shape, generator=g).to(DEV) for p in ps]
    ms = [torch.zeros_like(p) for p in ps]
    vs = [torch.zeros_like(p) for p in ps]
    lps = [torch.full(p.shape, 7.0, dtype=LP, device=DEV) for p in ps]
    tab = _MultiTensorTable(ps, gs, ms, vs, [lp.data_ptr() for lp in lps])
    for step in (1, 2):
        call("octmae_mt_adamw_fused", tab.table.data_ptr(), tab.chunk_tensor.data_ptr(), tab.chunk_off.data_ptr(), tab.n_chunks, None,
             tab.lp_table.data_ptr(), None, 1e-3, 0.9, 0.95, 1e-8, 0.0, step, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for p, lp in zip(ps, lps):
            assert torch.isfinite(p).all()
            assert bits_equal(lp, p.to(LP)), _show(lp, p.to(LP))
    assert _straddles(torch.cat([lp.view(-1) for lp in lps]))


# ------------------------------------------------------------------------------------------------ subnormal operands
def test_mfma_keeps_subnormal_operands():
    """v_mfma_f32_32x32x16_{f16,bf16} with every A entry subnormal in the operand type (half: 2^-24 ... 2^-15; bfloat16: 2^-133 ...
    2^-127) and B chosen so that every product and every sum is exact in fp32: D equals the exact product, as in torch's reference
    arithmetic -- the MFMA does not flush subnormal inputs (measured on gfx950: DESIGN.md section 2)."""
    g = torch.Generator().manual_seed(1)
    mant = torch.randint(1, 1024 if IS_F16 else 128, (32, 16), generator=g).double()
    sign = torch.randint(0, 2, (32, 16), generator=g).double() * 2 - 1
    A = sign * mant * (2.0 ** -24 if IS_F16 else 2.0 ** -133)
    Bm = torch.randint(-3, 4, (16, 32), generator=g).double() * (2.0 ** 4 if IS_F16 else 2.0 ** 100)
    a16, b16 = A.float().to(LP), Bm.float().to(LP)
    assert torch.equal(a16.double(), A) and torch.equal(b16.double(), Bm)               # exact in the operand type
    assert bool((a16.double().abs() < LP_TINY).all())                                   # ... and every A entry subnormal
    af = torch.empty(64, 8, dtype=LP); bfr = torch.empty(64, 8, dtype=LP)
    for l in range(64):
        r, h = l & 31, l >> 5
        af[l] = a16[r, 8 * h:8 * h + 8]
        bfr[l] = b16[8 * h:8 * h + 8, r]
    d = torch.empty(64, 16, device=DEV)
    a_dev, b_dev = af.to(DEV), bfr.to(DEV)
    call("octmae_probe_mfma32", a_dev.data_ptr(), b_dev.data_ptr(), d.data_ptr(), None)
    torch.cuda.synchronize()
    D = A @ Bm
    exp = torch.empty(64, 16, dtype=torch.float64)
    for l in range(64):
        r, h = l & 31, l >> 5
        for gi in range(16):
            exp[l, gi] = D[(gi & 3) + 8 * (gi >> 2) + 4 * h, r]
    got = d.double().cpu()
    flushed = bool((got == 0).all())
    assert torch.equal(got, exp), "the MFMA flushed the subnormal operands to zero" if flushed else f"max |D - exact| {float((got - exp).abs().max()):.3e}"


def test_gemm_with_subnormal_operands(tile_variant):
    """x mostly below the type's smallest normal number (|x| ~ tiny / 4), w scaled by 1 / tiny: fp32 output at fp32 accuracy, 16-bit
    output one rounding, against fp64 on the same rounded operands"""
    M, N, K = 600, 512, 256
    g = torch.Generator().manual_seed(6)
    x = (torch.randn(M, K, generator=g) * (LP_TINY / 4)).to(LP)
    w = (torch.randn(N, K, generator=g) * (K ** -0.5 / LP_TINY)).to(LP)
    assert float((x.double().abs() < LP_TINY).double().mean()) > 0.9 and bool((x != 0).any())
    x, w = x.to(DEV), w.to(DEV)
    ref = x.double() @ w.double().t()
    y32 = ops.linear_fwd(x, w, None, "f32")
    assert rel(y32, ref) < 2e-6
    y16 = ops.linear_fwd(x, w, None, "bf16")
    assert rel(y16, ref) < 1.3 * U and bits_equal(y16, y32.to(LP))


@pytest.mark.parametrize("HD", [64, 32])
def test_attention_with_most_of_p_below_the_smallest_normal(HD):
    """Logits spread so widely (q scaled by 5: logits ~ N(0, 25)) that most of P = exp(s - max) lies below 2^-14 of the row maximum:
    forward and both backward forms against fp64 on the same rounded operands, in units of U"""
    B, H, N = 1, 2, 300
    g = torch.Generator().manual_seed(HD)
    x = torch.randn(B * N, 3, H, HD, generator=g)
    x[:, 0] *= 5.0
    qkv = x.reshape(B * N, -1).to(LP).to(DEV)
    do = torch.randn(B * N, H * HD, generator=g).to(LP).to(DEV)
    q, k, _ = qkv.double().view(B, N, 3, H, HD).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * HD ** -0.5
    frac = float(((s - s.amax(-1, keepdim=True)).exp() < 2.0 ** -14).double().mean())
    assert frac > 0.5, frac
    o, lse = ops.attn_fwd(qkv, B, N, H, HD, HD ** -0.5)
    qd = qkv.double().requires_grad_(True)
    o_ref, _ = attn_ref(qd, B, N, H, HD)
    parity(f"{TAG}/u/attn_subnormal_p_hd{HD}/o", rel(o, o_ref) / U, 3.5)
    o_ref.backward(do.double())
    for fused in (True, False):
        d = ops.attn_bwd(qkv, o, do, lse, B, N, H, HD, HD ** -0.5, fused=fused)
        parity(f"{TAG}/u/attn_subnormal_p_hd{HD}/dqkv_{'fused' if fused else 'pair'}", rel(d, qd.grad) / U, 12.0)


# ------------------------------------------------------------------------------------------------ optimistic forward, far-off rows
@pytest.mark.parametrize("HD", [64, 32])
@pytest.mark.parametrize("logit", [-12.0, -20.0, -40.0, 12.0, 20.0])
def test_attention_optimistic_forward_on_uniformly_shifted_rows(HD, logit):
    """Every query of head 1 meets every key at a logit of `logit` (natural units, +- a little noise): softmax is shift-free, so o is
    the plain mean of v there.  P = e^-20 rounds to zero in half (e^-12 passes through its subnormals) and e^12 overflows it, while
    the fp32 row sum stays inside the optimistic kernel's [2^-100, 2^100] window.  optimistic=True must be within c U of fp64, or else
    bit-equal to the safe kernel (it gave up)."""
    B, H, N = 1, 2, 200
    g = torch.Generator().manual_seed(13)
    x = torch.randn(B * N, 3, H, HD, generator=g)
    a = (abs(logit) * HD ** 0.5) ** 0.5 / HD ** 0.5
    x[:, 0, 1] = a + 0.01 * x[:, 0, 1]                                      # q . k * scale = -+ a^2 HD / sqrt(HD) = logit
    x[:, 1, 1] = math.copysign(a, logit) + 0.01 * x[:, 1, 1]
    qkv = x.reshape(B * N, -1).to(LP).to(DEV)
    o, lse = ops.attn_fwd(qkv, B, N, H, HD, HD ** -0.5, optimistic=True)
    o_safe, lse_safe = ops.attn_fwd(qkv, B, N, H, HD, HD ** -0.5, optimistic=False)
    o_ref, lse_ref = attn_ref(qkv, B, N, H, HD)

    def err(t):                                       # per head: head 1 (the shifted rows) must not hide behind head 0
        return max(rel(t[:, h * HD:(h + 1) * HD], o_ref[:, h * HD:(h + 1) * HD]) for h in range(H)) / U

    e_safe = err(o_safe)
    parity(f"{TAG}/u/attn_shifted_rows_hd{HD}_{logit:+.0f}/safe", e_safe, 2.3)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    gave_up = torch.equal(o, o_safe) and torch.equal(lse, lse_safe)
    e_opt = err(o)
    assert gave_up or e_opt <= 2.3, f"optimistic forward: {e_opt:.2f} U from fp64 (safe kernel {e_safe:.2f} U), and it did not give up"
    assert float((lse.double() - lse_ref).abs().max()) <= 4 * U * (1.0 + float(lse_ref.abs().max()))


# ------------------------------------------------------------------------------------------------ accuracy at the u scale
def test_gemm_family_at_the_u_scale(tile_variant):
    """one ragged problem, every epilogue and the delta / dgelu entry points, against fp64 on the same rounded operands"""
    M, N, K = 333, 264, 200
    g = torch.Generator().manual_seed(7)
    x = torch.randn(M, K, generator=g).to(LP).to(DEV)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(LP).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    res = torch.randn(M, N, generator=g).to(DEV)
    ref = x.double() @ w.double().t() + b.double()
    v = tile_variant
    parity(f"{TAG}/u/gemm_{v}/epi0", rel(ops.linear_fwd(x, w, b, "bf16"), ref) / U, 1.3)
    parity(f"{TAG}/u/gemm_{v}/epi1", rel(ops.linear_fwd(x, w, b, "f32"), ref) / U, 4.5e-4)
    pre, act = ops.linear_fwd(x, w, b, "gelu")
    parity(f"{TAG}/u/gemm_{v}/epi2_act", rel(act, torch.nn.functional.gelu(pre.double())) / U, 1.25)
    parity(f"{TAG}/u/gemm_{v}/epi3", rel(ops.linear_fwd(x, w, b, "resid", res=res), ref + res.double()) / U, 4.5e-4)
    dy = torch.randn(M, N, generator=g).to(LP).to(DEV)
    prek = torch.randn(M, K, generator=g).to(LP).to(DEV)
    dref = dy.double() @ w.double()
    parity(f"{TAG}/u/gemm_{v}/dgrad", rel(ops.linear_dgrad(dy, w), dref) / U, 1.3)
    xg = prek.double().requires_grad_(True)
    torch.nn.functional.gelu(xg).backward(dref)
    parity(f"{TAG}/u/gemm_{v}/dgelu", rel(ops.linear_dgrad(dy, w, pre=prek), xg.grad) / U, 1.3)
    gw0 = torch.randn(N, K, generator=g).to(DEV)
    gw = gw0.clone()
    ops.linear_wgrad_accum(dy, x, gw)
    parity(f"{TAG}/u/gemm_{v}/epi5", rel(gw, gw0.double() + dy.double().t() @ x.double()) / U, 7.5e-4)
    # the delta epilogue of the proj dgrad (heads of 32): delta = -rowsum_head(dO * O) of the dO it stores
    HD, C = 32, 256
    Md = 1281
    w2 = (torch.randn(C, C, generator=g) * C ** -0.5).to(LP).to(DEV)
    dy2 = torch.randn(Md, C, generator=g).to(LP).to(DEV)
    o2 = torch.randn(Md, C, generator=g).to(LP).to(DEV)
    do, delta = ops.linear_dgrad_delta(dy2, w2, o2, C // HD, HD)
    parity(f"{TAG}/u/gemm_{v}/delta_do", rel(do, dy2.double() @ w2.double()) / U, 1.3)
    if delta is not None:
        dref2 = -(do.double() * o2.double()).view(Md, C // HD, HD).sum(-1)
        parity(f"{TAG}/u/gemm_{v}/delta", rel(delta, dref2) / U, 3.5e-4)


def test_layernorm_at_the_u_scale():
    M, D = 333, 768
    g = torch.Generator().manual_seed(8)
    x = (torch.randn(M, D, generator=g) * 2 + 0.5).to(DEV)
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(D, generator=g)).to(DEV)
    dy = torch.randn(M, D, generator=g).to(LP).to(DEV)
    y, mean, rstd = ops.layernorm_fwd(x, gamma, beta, 1e-6)
    xd = x.double().requires_grad_(True); gd = gamma.double().requires_grad_(True); bd = beta.double().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(xd, (D,), gd, bd, 1e-6)
    parity(f"{TAG}/u/layernorm/y", rel(y, yr) / U, 1.3)
    yr.backward(dy.double())
    dgamma = torch.zeros(D, device=DEV); dbeta = torch.zeros(D, device=DEV)
    dx, dxb = ops.layernorm_bwd(dy, x, mean, rstd, gamma, dgamma, dbeta, want_bf16=True)
    parity(f"{TAG}/u/layernorm/dx", rel(dx, xd.grad) / U, 4e-4)
    parity(f"{TAG}/u/layernorm/dx16", rel(dxb, xd.grad) / U, 1.3)
    parity(f"{TAG}/u/layernorm/dgamma", rel(dgamma, gd.grad) / U, 7.5e-4)


@pytest.mark.parametrize("HD", [64, 32])
def test_attention_at_the_u_scale(HD):
    B, H, N = 2, 3, 333
    g = torch.Generator().manual_seed(HD + 1)
    qkv = torch.randn(B * N, 3 * H * HD, generator=g).to(LP).to(DEV)
    do = torch.randn(B * N, H * HD, generator=g).to(LP).to(DEV)
    o, lse = ops.attn_fwd(qkv, B, N, H, HD, HD ** -0.5)
    qd = qkv.double().requires_grad_(True)
    o_ref, _ = attn_ref(qd, B, N, H, HD)
    parity(f"{TAG}/u/attn_hd{HD}/o", rel(o, o_ref) / U, 2.25)
    o_ref.backward(do.double())
    for fused in (True, False):
        d = ops.attn_bwd(qkv, o, do, lse, B, N, H, HD, HD ** -0.5, fused=fused)
        parity(f"{TAG}/u/attn_hd{HD}/dqkv_{'fused' if fused else 'pair'}", rel(d, qd.grad) / U, 2.5)


def test_slice_pool_at_the_u_scale():
    B, S, T, D = 2, 3, 37, 320
    g = torch.Generator().manual_seed(10)
    x = (torch.randn(B * S, T, D, generator=g) * 2 + 0.5).to(DEV)
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(D, generator=g)).to(DEV)
    dout = torch.randn(B, D, generator=g).to(DEV)
    for cls in (False, True):
        xg = x.clone().requires_grad_(True)
        gp, bp = torch.nn.Parameter(gamma.clone()), torch.nn.Parameter(beta.clone())
        out = ops.SlicePoolFn.apply(xg, gp, bp, 1e-6, S, cls)
        out.backward(dout)
        xd = x.double().requires_grad_(True)
        p = xd[:, 0] if cls else xd[:, 1:].mean(dim=1)
        ref = torch.nn.functional.layer_norm(p, (D,), gamma.double(), beta.double(), 1e-6).view(B, S, D).mean(dim=1)
        ref.backward(dout.double())
        tag = "cls" if cls else "mean"
        parity(f"{TAG}/u/slice_pool_{tag}/out", rel(out, ref) / U, 1e-3)
        parity(f"{TAG}/u/slice_pool_{tag}/dx", rel(xg.grad, xd.grad) / U, 4.5e-4)


def test_adamw_update_at_the_u_scale():
    """the UPDATE p_new - p_old against the oracle's update in fp64 (rel(p, ref) would hide a 6e-4 error in a 1.6e-3 step)"""
    g = torch.Generator().manual_seed(12)
    shapes = [(128, 64), (7,), (65536 + 3,)]
    ps = [torch.randn(s, generator=g).to(DEV) for s in shapes]
    ms = [torch.zeros_like(p) for p in ps]
    vs = [torch.zeros_like(p) for p in ps]
    ref_m = [torch.zeros(s, dtype=torch.float64) for s in shapes]
    ref_v = [torch.zeros(s, dtype=torch.float64) for s in shapes]
    for step in (1, 2, 3):
        gs = [torch.randn(p.shape, generator=g).to(DEV) for p in ps]
        tab = _MultiTensorTable(ps, gs, ms, vs)
        old = [p.clone() for p in ps]
        call("octmae_mt_adamw_fused", tab.table.data_ptr(), tab.chunk_tensor.data_ptr(), tab.chunk_off.data_ptr(), tab.n_chunks, None, None,
             None, 1.6e-3, 0.9, 0.95, 1e-8, 0.05, step, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        worst = 0.0
        for i, (p, p0, gr) in enumerate(zip(ps, old, gs)):
            pr, ref_m[i], ref_v[i] = O.adamw_step(p0.double().cpu(), gr.double().cpu(), ref_m[i], ref_v[i], step, 1.6e-3, 0.9, 0.95, 1e-8, 0.05)
            worst = max(worst, rel(p.double() - p0.double(), pr - p0.double().cpu()))
        parity(f"{TAG}/u/adamw_update/step{step}", worst / U, 0.18)
