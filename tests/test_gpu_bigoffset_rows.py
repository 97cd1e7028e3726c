"""The row and token kernels of the training path on tensors past 2^31 and 2^32 bytes -- `pytest -m gpu` on an MI355X.

These kernels reach memory through 64-bit pointer arithmetic on int row indices ((size_t)row * D and the like: csrc/layernorm.hip,
csrc/tokens.hip, csrc/recompute.hip); one forgotten cast is invisible below 2^31 elements or bytes, and no other test goes there.
Every kernel runs where its largest tensor passes 2^31 bytes and again past 2^32; the three entry points whose ABI takes a 64-bit count
(octmae_cast_f32_bf16, octmae_cast_rowscale_f32_bf16, octmae_gelu_apply) and the LayerNorm forward (with octmae_ln_apply) also past
2^31 ELEMENTS.  docs/OFFSET_RANGES.md lists every entry point with its index types.

Inputs are random and drawn on the device; every output lies between guard bands and starts as SENTINEL; references are float64
(or, for the kernels that only move and round, the same fp32 / 16-bit operations in torch) chunk by chunk; the worst error is kept per
band of byte offsets of the case's largest tensor and goes to the parity ledger.  Bounds:
  LayerNorm     tests/test_gpu_layernorm_rows.py's for plain rows: y rows 2.1 U; mean, rstd max(1e-5, 4 Y); dx rows max(2e-5, 4 Y); dgamma,
                dbeta, dxsum max(1e-4, 4 Y), Y = the same formulas in fp32 torch on the device against float64 (tests/lnrows.py::yardstick,
                chunked); the 16-bit dx is the cast of dx and ln_apply's y is layernorm_fwd's, bit for bit
  casts         torch's round-to-nearest-even cast (of the fp32 product with the row's scale), bit for bit
  gelu_apply    the same kernel on each chunk alone (a launch far below 2^31, which tests/test_gpu_recompute.py holds bit-equal to the GEMM
                epilogue), bit for bit -- and tests/gemm_elem.py::gelu_bounds against float64
  column sums   integer inputs in {-2 .. 2}: every partial sum is an integer below 2^24, the result EQUALS float64
  assemblies, row and patch gather   one widening / one fp32 add / one rounding: torch.equal (tests/test_gpu_tokens.py)
  MSE           tests/test_gpu_tokens.py's: per-token loss within 1e-5 of float64, dpred within one unit in the last place, and equal to the
                fp32 torch formula without norm_pix_loss"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import ops
    from octcubem_amd._lib import call, load
    LP = ops.BF16
else:
    LP = torch.bfloat16
from tests import bigoffset_ref as BR
from tests import gemm_elem as GE
from tests.conftest import parity

DEV = "cuda"
F64, F32 = torch.float64, torch.float32
U = GE.LP_U[LP]
TINY = torch.finfo(LP).tiny
TAG = "f16" if LP == torch.float16 else "bf16"
EPS = 1e-6
B31, B32 = BR.B31, BR.B32
LN_STEP = 32768                           # rows per chunk of the LayerNorm reference
LN_FLOOR = {"mean": 1e-5, "rstd": 1e-5, "dx": 2e-5, "dgamma": 1e-4, "dbeta": 1e-4, "dxsum": 1e-4}      # tests/test_gpu_layernorm_rows.py


def _st():
    return ops._stream()


def _eq(label, per_band):
    print(f"{label}: {per_band}")
    BR.record(label, per_band, 0.0)


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
def _ln_inputs(M, D, seed, backward, slim=False):
    """plain rows of tests/lnrows.py::draw: randn * s_n + o_n with the offset ramping over [-1.5, 1.5] and the scale cycling through
    [0.5, 2]; dy (16 bits) with a row scale of its own"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.empty((M, D), dtype=F32, device=DEV)
    dy = torch.empty((M, D), dtype=LP, device=DEV) if backward else None
    dres = torch.empty((M, D), dtype=F32, device=DEV) if backward and not slim else None
    for r0, r1 in BR.chunks(M):
        n = torch.arange(r0, r1, dtype=F64, device=DEV)
        off = (3.0 * (n + 0.5) / M - 1.5).float().unsqueeze(1)
        sc = (2.0 ** (2.0 * ((n * 0.381966) % 1.0) - 1.0)).float().unsqueeze(1)
        x[r0:r1] = torch.randn((r1 - r0, D), generator=g, device=DEV) * sc + off
        if backward:
            s2 = (2.0 ** (2.0 * (((n + 0.5) * 0.618034) % 1.0) - 1.0)).float().unsqueeze(1)
            dy[r0:r1] = (torch.randn((r1 - r0, D), generator=g, device=DEV) * s2).to(LP)
            if dres is not None:
                dres[r0:r1] = torch.randn((r1 - r0, D), generator=g, device=DEV)
    gamma = 1 + 0.1 * torch.randn(D, generator=g, device=DEV)
    beta = 0.1 * torch.randn(D, generator=g, device=DEV)
    return x, gamma, beta, dy, dres


def _ln_formulas(x, gamma, beta, dy, dres, dtype):
    """layer_norm (eps 1e-6) and its backward in `dtype` for one chunk: the reference in float64, the yardstick in float32"""
    xd, gd, bd = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    y, mean, rstd = torch.native_layer_norm(xd, (x.shape[1],), gd, bd, EPS)
    out = {"y": y, "mean": mean.flatten(), "rstd": rstd.flatten()}
    if dy is not None:
        dyd = dy.to(dtype)
        xhat = (xd - mean) * rstd
        gy = dyd * gd
        dx = rstd * (gy - gy.mean(-1, keepdim=True) - xhat * (gy * xhat).mean(-1, keepdim=True))
        if dres is not None:
            dx = dx + dres.to(dtype)
        out.update({"dx": dx, "dgamma": (dyd * xhat).sum(0), "dbeta": dyd.sum(0), "dxsum": dx.sum(0)})
    return out


class _RowStore:
    """per-row numerators and reference norms of tests/lnrows.py::row_err / vec_err, kept for all M rows (8 bytes each) so that the RMS
    floor is the whole tensor's, as in the small tests; then split into bands"""

    def __init__(self, M):
        self.num = torch.zeros(M, dtype=F64, device=DEV)
        self.ref = torch.zeros(M, dtype=F64, device=DEV)

    def put(self, r0, r1, got, ref):
        d = got.to(F64) - ref
        self.num[r0:r1] = d.norm(dim=-1) if d.dim() == 2 else d.abs()
        self.ref[r0:r1] = ref.norm(dim=-1) if ref.dim() == 2 else ref.abs()

    def per_band(self, row_bytes):
        floor = self.ref.pow(2).mean().sqrt()
        e = self.num / torch.maximum(self.ref, floor).clamp_min(1e-300)
        w = BR.Worst(row_bytes, DEV)
        w.add(0, e)
        return w.result()


def _vec_err(got, ref):
    got, ref = got.to(F64), ref.to(F64)
    e = (got - ref).abs() / torch.maximum(ref.abs(), ref.pow(2).mean().sqrt()).clamp_min(1e-300)
    return float(torch.where(torch.isfinite(e), e, torch.full_like(e, math.inf)).max())


def _ln_case(name, backward):
    """slim (the backward past 2^31 ELEMENTS): dres and the 16-bit copy are NULL, both optional in the ABI, and y is freed once the
    forward has left mean and rstd -- x, dy and dx alone are 10 bytes per element, 21.5 GB; with dres and the copy the case would keep
    34 GB alive.  The forward case of the same shape checks y."""
    M, D, _, _ = BR.ROW_CASES[name]
    slim = backward and name.endswith("elements")
    need = (10 if slim else 18 if backward else 8) * M * D + 12 * 8 * LN_STEP * D + 8 * 8 * M
    BR.require(need)
    label = f"bigoffset_rows/{TAG}/{name}/{'bwd' if backward else 'fwd'}"
    try:
        x, gamma, beta, dy, dres = _ln_inputs(M, D, 7 * D + M % 1000, backward, slim)
        bufy, y = BR.guarded((M, D), LP, DEV)
        (bufm, mean), (bufr, rstd) = BR.guarded((M,), F32, DEV), BR.guarded((M,), F32, DEV)
        bufs = {"y": (bufy, y), "mean": (bufm, mean), "rstd": (bufr, rstd)}
        call("octmae_layernorm_fwd", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), M, D, EPS, _st())
        sums = {}
        if not backward:                                             # the forward cases hold ln_apply to layernorm_fwd
            bufa, ya = bufs["y_apply"] = BR.guarded((M, D), LP, DEV)
            call("octmae_ln_apply", x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ya.data_ptr(), M, D, _st())
        else:
            if slim:
                torch.cuda.synchronize()
                assert BR.guards_intact(bufy, y), f"{label}: a store outside y (guard band overwritten)"
                del bufs["y"]
                bufy = y = None
                BR.release()
            bufx, dx = bufs["dx"] = BR.guarded((M, D), F32, DEV)
            if not slim:
                bufb, dxb = bufs["dxb"] = BR.guarded((M, D), LP, DEV)
            for k in ("dgamma", "dbeta", "dxsum"):
                bufs[k] = BR.guarded((D,), F32, DEV)
                bufs[k][1].zero_()
            nws = load().octmae_layernorm_bwd_ws_floats(M, D)
            assert nws > 0, nws
            ws = torch.empty((nws,), dtype=F32, device=DEV)
            call("octmae_layernorm_bwd", dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                 None if slim else dres.data_ptr(), dx.data_ptr(), None if slim else dxb.data_ptr(), bufs["dgamma"][1].data_ptr(), bufs["dbeta"][1].data_ptr(), bufs["dxsum"][1].data_ptr(),
                 ws.data_ptr(), M, D, _st())
            sums = {k: [torch.zeros(D, dtype=F64, device=DEV), torch.zeros(D, dtype=F32, device=DEV)] for k in ("dgamma", "dbeta", "dxsum")}
        torch.cuda.synchronize()
        for k, (b, t) in bufs.items():
            assert BR.guards_intact(b, t), f"{label}: a store outside {k} (guard band overwritten)"
        rows = (() if slim else ("y",)) + ("mean", "rstd") + (("dx",) if backward else ())
        got_all = {"y": y, "mean": mean, "rstd": rstd, "dx": dx if backward else None}
        kern, yard = {q: _RowStore(M) for q in rows}, {q: _RowStore(M) for q in rows}
        for r0, r1 in BR.chunks(M, LN_STEP):
            sl = slice(r0, r1)
            dyc, drc = dy[sl] if backward else None, dres[sl] if dres is not None else None
            ref = _ln_formulas(x[sl], gamma, beta, dyc, drc, F64)
            f32 = _ln_formulas(x[sl], gamma, beta, dyc, drc, F32)
            for q in rows:
                kern[q].put(r0, r1, got_all[q][sl], ref[q])
                yard[q].put(r0, r1, f32[q], ref[q])
            for k in sums:
                sums[k][0] += ref[k]
                sums[k][1] += f32[k]
        row_bytes = 4 * D
        fails = []
        for q in rows:
            Y = max(v for v in yard[q].per_band(row_bytes) if v is not None)
            bound = 2.1 * U if q == "y" else max(LN_FLOOR[q], 4 * Y)
            pb = kern[q].per_band(row_bytes)
            print(f"{label}/{q}: per band {pb}, yardstick {Y:.2e}, bound {bound:.2e}")
            try:
                BR.record(f"{label}/{q}", pb, bound)
            except AssertionError as e:
                fails.append(str(e))
        for k, (r64, r32) in sums.items():
            Y, e = _vec_err(r32, r64), _vec_err(bufs[k][1], r64)
            print(f"{label}/{k}: {e:.2e}, yardstick {Y:.2e}")
            try:
                parity(f"{label}/{k}", e, max(LN_FLOOR[k], 4 * Y))
            except AssertionError as err:
                fails.append(str(err))
        if slim:
            pass
        elif backward:
            _eq(f"{label}/dxb_vs_cast_of_dx", BR.compare(dxb, row_bytes, lambda r0, r1: (dx[r0:r1].to(LP), None)))
        else:
            _eq(f"{label}/ln_apply_vs_fwd", BR.compare(ya, row_bytes, lambda r0, r1: (y[r0:r1], None)))
        assert not fails, "\n".join(fails)
    finally:
        x = gamma = beta = dy = dres = bufy = y = bufa = ya = bufm = mean = bufr = rstd = bufs = bufx = dx = bufb = dxb = ws = None
        kern = yard = got_all = sums = ref = f32 = dyc = drc = None
        BR.release()


@pytest.mark.parametrize("name", list(BR.ROW_CASES))
def test_layernorm_forward_and_ln_apply(name):
    _ln_case(name, backward=False)


@pytest.mark.parametrize("name", list(BR.ROW_CASES))
def test_layernorm_backward_with_dres_copy_and_column_sums(name):
    _ln_case(name, backward=True)


# ------------------------------------------------------------------------------------------------------------------ casts, GELU
FLAT_STEP = 1 << 22                       # rows of 8 elements per chunk of the flat comparisons


@pytest.mark.parametrize("name", list(BR.CAST_CASES))
def test_cast_f32_to_16_bits(name):
    n, _ = BR.CAST_CASES[name]
    BR.require(4 * n + 2 * n + (1 << 30))
    try:
        src = BR.draw((n // 8, 8), F32, DEV, 201)
        buf, dst = BR.guarded((n // 8, 8), LP, DEV)
        call("octmae_cast_f32_bf16", src.data_ptr(), dst.data_ptr(), n, _st())
        torch.cuda.synchronize()
        assert BR.guards_intact(buf, dst)
        _eq(f"bigoffset_rows/{TAG}/cast/{name}", BR.compare(dst, 32, lambda r0, r1: (src[r0:r1].to(LP), None), step=FLAT_STEP))
    finally:
        src = buf = dst = None
        BR.release()


@pytest.mark.parametrize("name", list(BR.CAST_CASES))
def test_cast_rowscale_f32_to_16_bits(name):
    """dst [R, 1024] = 16-bit(rowscale[r // 5] * src): R a multiple of 5 (samples of 5 rows), scales 0, 1.25 and 2"""
    n, _ = BR.CAST_CASES[name]
    D, per = 1024, 5
    R = (n // D + per) // per * per
    BR.require(6 * R * D + (1 << 30))
    try:
        src = BR.draw((R, D), F32, DEV, 211)
        sc = torch.tensor([0.0, 1.25, 2.0], device=DEV)[torch.randint(0, 3, (R // per,), device=DEV)]
        buf, dst = BR.guarded((R, D), LP, DEV)
        call("octmae_cast_rowscale_f32_bf16", src.data_ptr(), sc.data_ptr(), dst.data_ptr(), R, D, per, _st())
        torch.cuda.synchronize()
        assert BR.guards_intact(buf, dst)
        rows = sc.repeat_interleave(per).unsqueeze(1)
        _eq(f"bigoffset_rows/{TAG}/cast_rowscale/{name}", BR.compare(dst, 4 * D, lambda r0, r1: ((src[r0:r1] * rows[r0:r1]).to(LP), None)))
    finally:
        src = sc = buf = dst = rows = None
        BR.release()


@pytest.mark.parametrize("name", list(BR.CAST_CASES))
def test_gelu_apply(name):
    """n 16-bit values (2^31 and 2^32 BYTES, then 2^31 elements): bit-equal to the same kernel on each chunk alone, and inside the
    activation's bound against float64 -- over every element at the first tier; at the two larger ones (float64 erfc takes 3 s per
    2^30 elements) over the first and the last chunk of 2^25 elements and the chunks that hold the elements at 2^31 and 2^32 bytes, so
    that every band is held to a reference that is not the kernel"""
    n = {"2g": B31 // 2 + 8 * 131, "4g": B32 // 2 + 8 * 67, "2g_elements": B31 + 8 * 1031}[name]
    BR.require(4 * n + (2 << 30))
    try:
        pre = BR.draw((n // 8, 8), LP, DEV, 221, scale=2.0)
        buf, act = BR.guarded((n // 8, 8), LP, DEV)
        call("octmae_gelu_apply", pre.data_ptr(), act.data_ptr(), n, _st())
        torch.cuda.synchronize()
        assert BR.guards_intact(buf, act)

        def alone(r0, r1):
            return ops.gelu_apply(pre[r0:r1].clone()), None

        _eq(f"bigoffset_rows/{TAG}/gelu_apply_vs_chunk_alone/{name}", BR.compare(act, 16, alone, step=FLAT_STEP))
        rows = n // 8
        if name == "2g":
            spans = [(0, rows)]
        else:      # the chunks that hold row 0, the rows at 2^31 and 2^32 bytes (16 bytes a row), and the last row
            starts = sorted({0, B31 // 16 // FLAT_STEP * FLAT_STEP, B32 // 16 // FLAT_STEP * FLAT_STEP, (rows - 1) // FLAT_STEP * FLAT_STEP})
            spans = [(r, min(r + FLAT_STEP, rows)) for r in starts if r < rows]
        pb = [None, None, None]
        for s0, s1 in spans:
            part = BR.compare(act[s0:s1], 16, lambda r0, r1: BR.gelu_bounds(pre[s0 + r0:s0 + r1], U, TINY), step=FLAT_STEP, r_base=s0)
            pb = [b if a is None else a if b is None else max(a, b) for a, b in zip(pb, part)]
        assert all(v is not None for v in pb[:2 if name == "2g" else 3]), pb
        print(f"gelu_apply {name}: {pb}")
        BR.record(f"bigoffset_rows/{TAG}/gelu_apply_vs_float64/{name}", pb)
    finally:
        pre = buf = act = alone = None
        BR.release()


# ------------------------------------------------------------------------------------------------------------------ column sums
@pytest.mark.parametrize("dtype_name,M", [("f32", B31 // 4096 + 131), ("f32", B32 // 4096 + 67), ("lp", B31 // 2048 + 131), ("lp", B32 // 2048 + 67)])
def test_colsum_accum_ws_equals_float64(dtype_name, M):
    """out[c] += sum_r in[r][c] over [M, 1024] integers in {-2 .. 2}, through the workspace form (octmae_colsum_accum_ws) and the
    workspace-free one (octmae_colsum_accum): exact"""
    N = 1024
    dt = F32 if dtype_name == "f32" else LP
    es = 4 if dtype_name == "f32" else 2
    assert M * N * es > B31 and BR.exact_sum_limit_ok(M, 2)
    rows = load().octmae_colsum_ws_rows(M)
    BR.require(es * M * N + 4 * rows * N + (1 << 30))
    try:
        a = BR.draw_int((M, N), dt, DEV, 231)
        buf, out = BR.guarded((N,), F32, DEV)
        out.fill_(3.0)
        ws = torch.empty((max(rows, 1), N), dtype=F32, device=DEV)
        call("octmae_colsum_accum_ws", a.data_ptr(), 1 if dt == LP else 0, out.data_ptr(), ws.data_ptr(), M, N, N, _st())
        ref = torch.zeros(N, dtype=F64, device=DEV)
        for r0, r1 in BR.chunks(M):
            ref += a[r0:r1].double().sum(0)
        torch.cuda.synchronize()
        assert BR.guards_intact(buf, out)
        wrong = int((out.double() != ref + 3.0).sum())
        parity(f"bigoffset_rows/{TAG}/colsum_ws/{dtype_name}/M{M}/mismatches", float(wrong), 0.0)
        # the workspace-free form (one workgroup per 8 columns walks all the rows): the entry point the GEMM's own column-sum passes take
        buf2, out2 = BR.guarded((N,), F32, DEV)
        out2.fill_(-1.0)
        call("octmae_colsum_accum", a.data_ptr(), 1 if dt == LP else 0, out2.data_ptr(), M, N, N, _st())
        torch.cuda.synchronize()
        assert BR.guards_intact(buf2, out2)
        wrong = int((out2.double() != ref - 1.0).sum())
        parity(f"bigoffset_rows/{TAG}/colsum/{dtype_name}/M{M}/mismatches", float(wrong), 0.0)
    finally:
        a = buf = out = ws = ref = buf2 = out2 = None
        BR.release()


# ------------------------------------------------------------------------------------------------------------------ assemblies, row gather
def _crosses(elements, esize, tier):
    """the three tiers of the sample-count cases: the tensor passes 2^31 bytes, 2^32 bytes, 2^31 ELEMENTS"""
    return {"2g": elements * esize > B31, "4g": elements * esize > B32, "2g_elements": elements > B31}[tier]


def _perm_prefix(B, L, n):
    return torch.rand((B, L), device=DEV).argsort(1)[:, :n].contiguous()


@pytest.mark.parametrize("B,tier", [(128, "2g"), (256, "4g"), (520, "2g_elements")])
def test_enc_assemble(B, tier):
    """x f32 [B, 1 + 4099, 1024]: 2.15 GB at B = 128, 4.3 GB at 256, 2^31 + 3.6e7 elements at 520; x[b, 0] = cls + pos_cls, x[b, 1 + i] = float(tok[b, i]) + pos[ids[b, i]]"""
    nkeep, D = 4099, 1024
    L = 2 * nkeep
    assert _crosses(B * (nkeep + 1) * D, 4, tier)
    BR.require(6 * B * (nkeep + 1) * D + 4 * L * D + (2 << 30))
    try:
        tok = BR.draw((B * nkeep, D), LP, DEV, 241)
        pos, cls, pos_cls = torch.randn((L, D), device=DEV), torch.randn(D, device=DEV), torch.randn(D, device=DEV)
        ids = _perm_prefix(B, L, nkeep)
        buf, x = BR.guarded((B, nkeep + 1, D), F32, DEV)
        call("octmae_enc_assemble", tok.data_ptr(), pos.data_ptr(), cls.data_ptr(), pos_cls.data_ptr(), ids.data_ptr(), x.data_ptr(), B, nkeep, D, _st())
        torch.cuda.synchronize()
        assert BR.guards_intact(buf, x)

        def exp(b0, b1):
            t = tok[b0 * nkeep:b1 * nkeep].float().view(b1 - b0, nkeep, D) + pos[ids[b0:b1]]
            return torch.cat([(cls + pos_cls).expand(b1 - b0, 1, D), t], 1), None

        _eq(f"bigoffset_rows/{TAG}/enc_assemble/B{B}", BR.compare(x, (nkeep + 1) * D * 4, exp, step=8))
    finally:
        tok = pos = cls = pos_cls = ids = buf = x = exp = None
        BR.release()


@pytest.mark.parametrize("B,emb_has_cls,tier", [(256, 0, "2g"), (256, 1, "2g"), (512, 0, "4g"), (512, 1, "4g"), (1030, 0, "2g_elements"),
                                                (1030, 1, "2g_elements")])
def test_dec_assemble(B, emb_has_cls, tier):
    """x f32 [B, 1 + 4100, 512]: 2.15 GB at B = 256, 4.3 GB at 512, 2^31 + 1.5e7 elements at 1030"""
    nkeep, L, D = 1025, 4100, 512
    assert _crosses(B * (L + 1) * D, 4, tier)
    erows = nkeep + emb_has_cls
    BR.require(4 * B * (L + 1) * D + 2 * B * erows * D + (2 << 30))
    try:
        emb = BR.draw((B * erows, D), LP, DEV, 251)
        mask_token, dcls, dpos_cls = (torch.randn(D, device=DEV) for _ in range(3))
        dpos = torch.randn((L, D), device=DEV)
        ids_restore = torch.rand((B, L), device=DEV).argsort(1).argsort(1).contiguous()
        buf, x = BR.guarded((B, L + 1, D), F32, DEV)
        call("octmae_dec_assemble", emb.data_ptr(), mask_token.data_ptr(), dpos.data_ptr(), None if emb_has_cls else dcls.data_ptr(),
             dpos_cls.data_ptr(), ids_restore.data_ptr(), x.data_ptr(), B, nkeep, L, D, emb_has_cls, _st())
        torch.cuda.synchronize()
        assert BR.guards_intact(buf, x)

        def exp(b0, b1):
            n = b1 - b0
            e = emb[b0 * erows:b1 * erows].float().view(n, erows, D)
            seq = torch.cat([e[:, emb_has_cls:], mask_token.expand(n, L - nkeep, D)], 1)
            body = torch.gather(seq, 1, ids_restore[b0:b1].unsqueeze(-1).expand(-1, -1, D)) + dpos
            first = (e[:, 0] if emb_has_cls else dcls.expand(n, D)) + dpos_cls
            return torch.cat([first.unsqueeze(1), body], 1), None

        _eq(f"bigoffset_rows/{TAG}/dec_assemble/B{B}_cls{emb_has_cls}", BR.compare(x, (L + 1) * D * 4, exp, step=16))
    finally:
        emb = mask_token = dcls = dpos_cls = dpos = ids_restore = buf = x = exp = None
        BR.release()


@pytest.mark.parametrize("B,tier", [(128, "2g"), (256, "4g"), (520, "2g_elements")])
@pytest.mark.parametrize("with_ids", [False, True])
def test_gather_rows_cast(B, tier, with_ids):
    """src f32 [B, 4100, 1024] (2.15 GB at B = 128, 4.3 GB at 256, 2^31 + 3.6e7 elements at 520) -> out 16-bit [B * 4099, 1024] = src[b][1 + ids[b][i]] rounded; ids = NULL
    is the identity"""
    n, D = 4099, 1024
    src_rows = n + 1
    assert _crosses(B * src_rows * D, 4, tier)
    BR.require(6 * B * src_rows * D + (2 << 30))
    try:
        src = BR.draw((B, src_rows, D), F32, DEV, 261)
        ids = _perm_prefix(B, src_rows - 1, n) if with_ids else None
        buf, out = BR.guarded((B, n, D), LP, DEV)
        call("octmae_gather_rows_cast", src.data_ptr(), None if ids is None else ids.data_ptr(), out.data_ptr(), B, n, src_rows, D, _st())
        torch.cuda.synchronize()
        assert BR.guards_intact(buf, out)

        def exp(b0, b1):
            idx = torch.arange(n, device=DEV).expand(b1 - b0, n) if ids is None else ids[b0:b1]
            return torch.gather(src[b0:b1, 1:], 1, idx.unsqueeze(-1).expand(-1, -1, D)).to(LP), None

        _eq(f"bigoffset_rows/{TAG}/gather_rows_cast/B{B}_ids{int(with_ids)}", BR.compare(out, src_rows * D * 4, exp, step=8))
    finally:
        src = ids = buf = out = exp = None
        BR.release()


@pytest.mark.parametrize("B,tier", [(137, "2g"), (274, "4g"), (547, "2g_elements")])
def test_patch_gather(B, tier):
    """imgs f32 [B, 1, 60, 256, 256] (2.15 GB at B = 137, 4.3 GB at 274, 2^31 + 3.4e6 elements at 547) -> out 16-bit [B * 1280, 768]: the im2col of the kept tokens in
    conv-weight order, rounded once (tests/test_gpu_tokens.py::test_patch_gather_int64_and_int32_ids builds it the same way)"""
    C, T, S, tp, p, nkeep = 1, 60, 256, 3, 16, 1280
    gt, gh = T // tp, S // p
    L, kdim = gt * gh * gh, C * tp * p * p
    img_bytes = C * T * S * S * 4
    assert _crosses(B * img_bytes // 4, 4, tier)
    BR.require(B * img_bytes + 2 * B * nkeep * kdim + (2 << 30))
    try:
        imgs = BR.draw((B, C, T, S, S), F32, DEV, 281)
        ids = _perm_prefix(B, L, nkeep)
        buf, out = BR.guarded((B, nkeep, kdim), LP, DEV)
        call("octmae_patch_gather", imgs.data_ptr(), ids.data_ptr(), 1, out.data_ptr(), B, C, T, S, S, tp, p, nkeep, _st())
        torch.cuda.synchronize()
        assert BR.guards_intact(buf, out)

        def exp(b0, b1):
            full = imgs[b0:b1].view(b1 - b0, C, gt, tp, gh, p, gh, p).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(b1 - b0, L, kdim)
            return torch.gather(full, 1, ids[b0:b1].unsqueeze(-1).expand(-1, -1, kdim)).to(LP), None

        _eq(f"bigoffset_rows/{TAG}/patch_gather/B{B}", BR.compare(out, img_bytes, exp, step=8))
    finally:
        imgs = ids = buf = out = exp = None
        BR.release()


# ------------------------------------------------------------------------------------------------------------------ patchify + MSE
def _ulp(ref):
    mant, emin = (7, -126) if LP == torch.bfloat16 else (10, -14)
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -200))).clamp_min(emin)
    return torch.exp2(e - mant)


@pytest.mark.parametrize("norm_pix", [0, 1])
@pytest.mark.parametrize("B,tier", [(137, "2g"), (274, "4g"), (547, "2g_elements")])
def test_mse_fwd_bwd(B, tier, norm_pix):
    """the ViT-L geometry (60 x 256 x 256, p = 16, u = 3): imgs f32 [B, 1, 60, 256, 256] and pred f32 [B, 1 + 5120, 768] are 2.15 GB each at
    B = 137, 4.3 GB at 274, and 2^31 + 3.4e6 elements each at 547 (the 16-bit dpred too).  Per-token loss within 1e-5 of float64; dpred within one unit in the last place of float64, exact zeros
    on cls and unmasked rows, and equal to the fp32 torch formula without norm_pix_loss."""
    from oracle import mae3d_ref as O
    T, S, p, tp = 60, 256, 16, 3
    cfg = O.MAEConfig(input_size=S, in_chans=1, num_frames=T, t_patch_size=tp, pred_t_dim=T, high_res_input_size=2 * S, norm_pix_loss=bool(norm_pix))
    u, L, PD = cfg.t_pred_patch_size, cfg.num_patches, cfg.patch_dim
    img_bytes, pred_bytes = T * S * S * 4, (L + 1) * PD * 4
    assert _crosses(B * img_bytes // 4, 4, tier) and _crosses(B * pred_bytes // 4, 4, tier)
    BR.require(B * img_bytes + B * pred_bytes + B * pred_bytes // 2 + (3 << 30))
    label = f"bigoffset_rows/{TAG}/mse/B{B}_normpix{norm_pix}"
    try:
        imgs = BR.draw((B, 1, T, S, S), F32, DEV, 271).abs_()
        pred = BR.draw((B, L + 1, PD), F32, DEV, 272)
        mask = (torch.rand((B, L), device=DEV) > 0.3).float()
        coef = torch.full((1,), 2.0 / PD, dtype=F32, device=DEV)
        bufl, loss_tok = BR.guarded((B, L), F32, DEV)
        bufd, dpred = BR.guarded((B, L + 1, PD), LP, DEV)
        call("octmae_mse_fwd", pred.data_ptr(), imgs.data_ptr(), None, loss_tok.data_ptr(), B, 1, T, S, S, u, p, L, norm_pix, _st())
        call("octmae_mse_bwd", pred.data_ptr(), imgs.data_ptr(), None, mask.data_ptr(), coef.data_ptr(), dpred.data_ptr(), B, 1, T, S, S, u, p, L,
             norm_pix, _st())
        torch.cuda.synchronize()
        assert BR.guards_intact(bufl, loss_tok) and BR.guards_intact(bufd, dpred)

        def target64(b0, b1):
            t = O.patchify(imgs[b0:b1].double(), cfg)
            if norm_pix:
                t = (t - t.mean(-1, keepdim=True)) / (t.var(-1, keepdim=True) + 1.0e-6) ** 0.5
            return t

        def tok(b0, b1):
            ref = ((pred[b0:b1, 1:].double() - target64(b0, b1)) ** 2).mean(-1)
            return ref, 1e-5 * ref

        def grad(b0, b1):
            ref = (2.0 / PD) * mask[b0:b1].double().unsqueeze(-1) * (pred[b0:b1, 1:].double() - target64(b0, b1))
            ref = torch.cat([torch.zeros_like(ref[:, :1]), ref], 1)
            # zero rows (cls, mask = 0) must be exact zeros: a bound no error fits under
            return ref, torch.where(ref == 0, torch.full_like(ref, 1e-300), _ulp(ref))

        pbs = {"loss_tok": BR.compare(loss_tok, img_bytes, tok, step=4), "dpred": BR.compare(dpred, pred_bytes, grad, step=4)}
        fails = []
        for k, pb in pbs.items():
            print(f"{label}/{k}: {pb}")
            try:
                BR.record(f"{label}/{k}", pb)
            except AssertionError as e:
                fails.append(str(e))
        assert not fails, "\n".join(fails)
        if not norm_pix:
            def exact(b0, b1):
                t32 = O.patchify(imgs[b0:b1], cfg)
                body = ((coef * mask[b0:b1]).unsqueeze(-1) * (pred[b0:b1, 1:] - t32)).to(LP)
                return torch.cat([torch.zeros_like(body[:, :1]), body], 1), None

            _eq(f"{label}/dpred_vs_fp32_formula", BR.compare(dpred, pred_bytes, exact, step=4))
    finally:
        imgs = pred = mask = coef = bufl = loss_tok = bufd = dpred = target64 = tok = grad = exact = None
        BR.release()


# ------------------------------------------------------------------------------------------------------------------ guards
def test_row_entry_points_decline_counts_they_keep_in_int():
    """-1 before any launch, outputs untouched (as check_argument_checks of tests/test_gpu_slivit_kernels.py): the B * (L + 1) token rows
    of the MSE kernels beyond 2^31 - 1 (PD = 16 puts 2^31 rows of 64 bytes within a card's memory), and in the slice pool B * S beyond the
    grid's y and B * S * T beyond an int while B S T D stays below the 2^40 the entry points already held"""
    lib, st = load(), _st()
    full = lambda n: torch.full((n,), BR.SENTINEL, dtype=F32, device=DEV)      # noqa: E731
    p = lambda t: t.data_ptr()                                                # noqa: E731
    C, T, S, u, pp, L = 1, 3, 16, 3, 16, 1                                    # one token of PD = 768 per sample
    pred, imgs = torch.randn((2, L + 1, 768), device=DEV), torch.randn((2, C, T, S, S), device=DEV)
    mask, coef = torch.ones((2, L), device=DEV), torch.ones(1, device=DEV)
    loss_tok, dpred = full(64), torch.full((2 * (L + 1) * 768,), BR.SENTINEL, dtype=LP, device=DEV)
    calls = []
    for B, l in [(1 << 30, 1), (1 << 20, 2047), (65536, 32767)]:              # B * (L + 1) = 2^31
        calls += [lib.octmae_mse_fwd(p(pred), p(imgs), None, p(loss_tok), B, C, T, S, S, u, pp, l, 0, st),
                  lib.octmae_mse_bwd(p(pred), p(imgs), None, p(mask), p(coef), p(dpred), B, C, T, S, S, u, pp, l, 0, st)]
    D = 64
    x, gamma, beta = torch.randn((2, 2, D), device=DEV), torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    out, pooled, mean, rstd, ws, dx = full(D), full(2 * D), full(2), full(2), full(1024), full(2 * 2 * D)
    dout = torch.randn((1, D), device=DEV)
    for B, s, t in [(1, 65536, 2), (256, 256, 2), (1, 65535, 40000), (255, 257, 40000)]:      # B S = 65 536; B S T = 2.6e9 at B S = 65 535
        assert B * s * t * D < 1 << 40
        calls += [lib.octmae_slice_pool_fwd(p(x), p(gamma), p(beta), p(out), p(pooled), p(mean), p(rstd), p(ws), B, s, t, D, 0, EPS, st),
                  lib.octmae_slice_pool_bwd(p(dout), p(pooled), p(mean), p(rstd), p(gamma), p(dx), None, None, None, None, p(ws), B, s, t, D, 0, st)]
    torch.cuda.synchronize()
    assert calls == [-1] * len(calls), calls
    for t in (loss_tok, dpred, out, pooled, mean, rstd, ws, dx):
        assert bool((t == BR.SENTINEL).all()), "a declined call wrote to an output"
    # the same buffers at their real shapes are accepted
    assert lib.octmae_mse_fwd(p(pred), p(imgs), None, p(loss_tok), 2, C, T, S, S, u, pp, L, 0, st) == 0
    assert lib.octmae_slice_pool_fwd(p(x), p(gamma), p(beta), p(out), p(pooled), p(mean), p(rstd), p(ws), 1, 2, 2, D, 0, EPS, st) == 0
    torch.cuda.synchronize()
    assert not bool((loss_tok[:2] == BR.SENTINEL).any()) and not bool((out == BR.SENTINEL).any())
