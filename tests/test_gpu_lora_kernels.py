"""The adapter kernels (csrc/lora.hip) against tests/lora_ref.py -- `pytest -m gpu` on an MI355X.

Every operand is a view into a NaN-filled buffer (rows further apart than they are wide, NaN in front, between and behind), so a read
past an edge shows as a non-finite result; every output is a view into a pre-filled buffer that must keep its bits around the view.
Shapes are the smallest that can go wrong: one rank, ranks that are no multiple of 16, one to four column tiles of 16 ranks, widths
below and above the 64 columns of a workgroup and no multiple of them, row counts around the 16 rows of a wave, the 32 rows of an MFMA
step and the row chunk of octmae_lora_plan (one, two and three chunks)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import ops
    LP = ops.BF16
else:
    LP = torch.bfloat16
from tests import bigoffset_ref as BR
from tests import gemm_elem as GE
from tests import lora_ref as LR

DEV = "cuda"
F32 = torch.float32
U = GE.LP_U[LP]
TINY = torch.finfo(LP).tiny
LAYERS = [(96, 32, 1), (192, 64, 4), (64, 256, 16), (256, 64, 17), (128, 128, 64)]          # (O, I, r)
S = 0.5


def _view(shape, dtype, fill, extra=24, lead=40):
    """[rows, cols] view with a row stride of cols + extra into a buffer filled with `fill`; 16-byte aligned, `lead` elements in"""
    rows, cols = shape
    ld = cols + extra
    buf = torch.full((lead + rows * ld + 64,), fill, dtype=dtype, device=DEV)
    return buf, buf[lead:lead + rows * ld].view(rows, ld)[:, :cols]


def _operand(t, dtype):
    buf, v = _view(tuple(t.shape), dtype, float("nan"))
    v.copy_(t)
    return buf, v


def _layer(O, I, r, seed):
    g = torch.Generator().manual_seed(seed)
    W = 0.05 * torch.randn((O, I), generator=g)
    A = torch.randn((r, I), generator=g) / I ** 0.5
    B = 0.3 * torch.randn((O, r), generator=g)
    return W, A, B


@pytest.fixture(scope="module")
def merged():
    """per layer: the CPU parameters and the kernel's padded operand copies (the operands of the gradient tests)"""
    out = {}
    for O, I, r in LAYERS:
        W, A, B = _layer(O, I, r, 7 * O + r)
        rp = ops.lora_rp(r)
        A_lp = torch.full((rp, I), float("nan"), dtype=LP, device=DEV)
        B_lp = torch.full((O, rp), float("nan"), dtype=LP, device=DEV)
        w_lp = torch.full((O, I), float("nan"), dtype=LP, device=DEV)
        ops.lora_merge(W.to(DEV), A.to(DEV), B.to(DEV), S, w_lp, A_lp, B_lp)
        out[(O, I, r)] = (W, A, B, w_lp, A_lp, B_lp)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("O,I,r", LAYERS)
def test_merge(O, I, r, merged):
    W, A, B, w_lp, A_lp, B_lp = merged[(O, I, r)]
    rp = ops.lora_rp(r)
    Wd, Ad, Bd = W.to(DEV), A.to(DEV), B.to(DEV)
    w32 = torch.full((O, I), float("nan"), dtype=F32, device=DEV)
    ops.lora_merge(Wd, Ad, Bd, S, w32)
    ref, bound = LR.merge_ref(W, A, B, S)
    w, idx = GE.worst(w32, ref, bound)
    print(f"merge {(O, I, r)}: worst {w:.3f} at {idx}")
    assert w <= 1.0, (w, idx)
    assert torch.equal(w32.to(LP).view(torch.int16), w_lp.view(torch.int16)), "the 16-bit output is not the cast of the f32 output"
    # the operand copies: the adapter rounded once, +0 bits in the padding
    assert torch.equal(A_lp[:r].cpu(), A.to(LP)) and torch.equal(B_lp[:, :r].cpu(), B.to(LP))
    assert not bool(A_lp[r:].view(torch.int16).any()) and not bool(B_lp[:, r:].view(torch.int16).any())
    exp_A, exp_B = LR.pad_operands(A, B, LP)
    assert torch.equal(A_lp.cpu().view(torch.int16), exp_A.view(torch.int16)) and torch.equal(B_lp.cpu().view(torch.int16), exp_B.view(torch.int16))
    # B = 0: the value of cvt(W)
    w0 = torch.full((O, I), float("nan"), dtype=LP, device=DEV)
    ops.lora_merge(Wd, Ad, torch.zeros_like(Bd), S, w0)
    assert torch.equal(w0.cpu(), W.to(LP))


def test_merge_past_the_grid_cap():
    """4104 x 2560 weights: 2 626 560 quads for the 2 097 152 threads of the capped grid (docs/GRID_CAPS.md), so some threads make a second
    trip and the last round is ragged"""
    O, I, r = 4104, 2560, 4
    W, A, B = _layer(O, I, r, 13)
    Wd, Ad, Bd = W.to(DEV), A.to(DEV), B.to(DEV)
    w32 = torch.full((O, I), float("nan"), dtype=F32, device=DEV)
    w_lp = torch.full((O, I), float("nan"), dtype=LP, device=DEV)
    ops.lora_merge(Wd, Ad, Bd, S, w32)
    ops.lora_merge(Wd, Ad, Bd, S, w_lp)
    ref, bound = LR.merge_ref(W, A, B, S)
    w, idx = GE.worst(w32, ref, bound)
    assert w <= 1.0, (w, idx)
    assert torch.equal(w32.to(LP).view(torch.int16), w_lp.view(torch.int16))


def _m_values():
    chunk = 256          # octmae_lora_plan's rows per chunk at these widths (asserted in the test)
    return [1, 15, 16, 17, 65, chunk - 1, chunk, chunk + 1, 2 * chunk + 1]


def _grad_views(O, I, r, seed):
    """gA [rp, I] and gB [O, rp] views (the kernel is handed the first r rows / columns) into pre-filled buffers, and their copies"""
    rp = ops.lora_rp(r)
    g = torch.Generator().manual_seed(seed)
    bufa, gA = _view((rp + 1, I), F32, 3.0)
    bufb, gB = _view((O, rp + 1), F32, -5.0)
    gA.copy_(torch.randn((rp + 1, I), generator=g))
    gB.copy_(torch.randn((O, rp + 1), generator=g))
    return bufa, gA, bufb, gB


def _run(x, dy, A_lp, B_lp, r, O, I, seed, want_a=True, want_b=True):
    bufa, gA, bufb, gB = _grad_views(O, I, r, seed)
    before = (bufa.clone(), bufb.clone())
    ops.lora_wgrad(x, dy, A_lp, B_lp, S, r, gA[:r] if want_a else None, gB[:, :r] if want_b else None)
    torch.cuda.synchronize()
    return bufa, gA, bufb, gB, before


@pytest.mark.parametrize("M", _m_values())
@pytest.mark.parametrize("O,I,r", LAYERS)
def test_wgrad(O, I, r, M, merged):
    _, _, _, _, A_lp, B_lp = merged[(O, I, r)]
    rp = ops.lora_rp(r)
    chunk, nchunks, _, _ = ops.lora_plan(M, I, O, rp)
    assert chunk == 256 and nchunks == -(-M // 256)
    g = torch.Generator().manual_seed(1000 * r + M)
    _, x = _operand(torch.randn((M, I), generator=g).to(LP), LP)
    _, dy = _operand((0.1 * torch.randn((M, O), generator=g)).to(LP), LP)
    seed = 31 * M + r
    bufa, gA, bufb, gB, (bufa0, bufb0) = _run(x, dy, A_lp, B_lp, r, O, I, seed)
    _, gA0, _, gB0 = _grad_views(O, I, r, seed)                                     # the same pre-fill
    (ra, ba), (rb, bb) = LR.wgrad_ref(x, dy, A_lp, B_lp, S, r, gA0[:r], gB0[:, :r], U, TINY)
    wa, ia, _ = LR.check(gA[:r], ra, ba, gA0[:r], r, 0)
    wb, ib, _ = LR.check(gB[:, :r], rb, bb, gB0[:, :r], r, 1)
    print(f"wgrad {(O, I, r)} M={M}: worst gA {wa:.3f} at {ia}, gB {wb:.3f} at {ib}")
    assert wa <= 1.0 and wb <= 1.0, (wa, ia, wb, ib)
    # nothing but the first r rows / columns changed: the rows / columns behind, the space between the rows, the bands around
    for buf, buf0, view in ((bufa, bufa0, gA[:r]), (bufb, bufb0, gB[:, :r])):
        probe = buf.clone()
        view0 = probe[view.storage_offset():].as_strided(view.shape, view.stride())
        view0.copy_(buf0[view.storage_offset():].as_strided(view.shape, view.stride()))
        assert torch.equal(probe.view(torch.int32), buf0.view(torch.int32)), "a store outside the gradient view"
    # two calls give the same bits
    _, gA2, _, gB2, _ = _run(x, dy, A_lp, B_lp, r, O, I, seed)
    assert torch.equal(gA2.view(torch.int32), gA.view(torch.int32)) and torch.equal(gB2.view(torch.int32), gB.view(torch.int32))
    # one gradient alone: the same bits, the other buffer untouched
    bufa3, gA3, bufb3, gB3, (_, bufb30) = _run(x, dy, A_lp, B_lp, r, O, I, seed, want_b=False)
    assert torch.equal(gA3.view(torch.int32), gA.view(torch.int32)) and torch.equal(bufb3.view(torch.int32), bufb30.view(torch.int32))
    bufa4, gA4, bufb4, gB4, (bufa40, _) = _run(x, dy, A_lp, B_lp, r, O, I, seed, want_a=False)
    assert torch.equal(gB4.view(torch.int32), gB.view(torch.int32)) and torch.equal(bufa4.view(torch.int32), bufa40.view(torch.int32))


@pytest.mark.parametrize("M", [65, 257])
@pytest.mark.parametrize("O,I,r", LAYERS)
def test_wgrad_planted_nan_reaches_what_uses_it(O, I, r, M, merged):
    """one NaN in dY[m][o]: U[m] and so every element of gA, and row o of gB; every other row of gB has the bits of the clean run"""
    _, _, _, _, A_lp, B_lp = merged[(O, I, r)]
    g = torch.Generator().manual_seed(77 * r + M)
    _, x = _operand(torch.randn((M, I), generator=g).to(LP), LP)
    _, dy = _operand((0.1 * torch.randn((M, O), generator=g)).to(LP), LP)
    _, gA, _, gB, _ = _run(x, dy, A_lp, B_lp, r, O, I, 5)
    m, o = M - 2, O // 3
    dy[m, o] = float("nan")
    _, gAn, _, gBn, _ = _run(x, dy, A_lp, B_lp, r, O, I, 5)
    assert not bool(torch.isfinite(gAn[:r]).any())
    assert not bool(torch.isfinite(gBn[o, :r]).any())
    rows = [i for i in range(O) if i != o]
    assert torch.equal(gBn[rows].view(torch.int32), gB[rows].view(torch.int32))
    assert bool(torch.isfinite(gA[:r]).all()) and bool(torch.isfinite(gB[:, :r]).all())


def test_wgrad_rows_past_4_gib():
    """X and dY as row views of one untouched allocation with rows 2^27 bytes apart: the last rows begin past 2^32 bytes, so a row offset
    kept in 32 bits reads another row (docs/OFFSET_RANGES.md)"""
    O, I, r, M = 192, 64, 4, 35
    ld = 1 << 26                                           # elements: 128 MiB per row
    BR.require(2 * M * ld + (1 << 30))
    try:
        big = torch.empty((M * ld,), dtype=LP, device=DEV)
        rows = big.view(M, ld)
        x, dy = rows[:, :I], rows[:, 128:128 + O]
        assert (M - 1) * ld * 2 > BR.B32 and big.data_ptr() % 16 == 0
        g = torch.Generator().manual_seed(5)
        x.copy_(torch.randn((M, I), generator=g).to(LP))
        dy.copy_((0.1 * torch.randn((M, O), generator=g)).to(LP))
        W, A, B = _layer(O, I, r, 3)
        rp = ops.lora_rp(r)
        A_lp, B_lp = torch.empty((rp, I), dtype=LP, device=DEV), torch.empty((O, rp), dtype=LP, device=DEV)
        ops.lora_merge(W.to(DEV), A.to(DEV), B.to(DEV), S, torch.empty((O, I), dtype=LP, device=DEV), A_lp, B_lp)
        _, gA, _, gB, _ = _run(x, dy, A_lp, B_lp, r, O, I, 9)
        _, gA0, _, gB0 = _grad_views(O, I, r, 9)
        (ra, ba), (rb, bb) = LR.wgrad_ref(x, dy, A_lp, B_lp, S, r, gA0[:r], gB0[:, :r], U, TINY)
        wa, wb = GE.worst(gA[:r], ra, ba)[0], GE.worst(gB[:, :r], rb, bb)[0]
        print(f"rows past 4 GiB: worst gA {wa:.3f}, gB {wb:.3f}")
        assert wa <= 1.0 and wb <= 1.0
        # the same rows packed densely give the same bits: the arithmetic does not depend on where the rows lie
        _, gAd, _, gBd, _ = _run(x.contiguous(), dy.contiguous(), A_lp, B_lp, r, O, I, 9)
        assert torch.equal(gAd.view(torch.int32), gA.view(torch.int32)) and torch.equal(gBd.view(torch.int32), gB.view(torch.int32))
    finally:
        big = rows = x = dy = None
        BR.release()
