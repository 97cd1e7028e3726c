"""Helpers of the tests that hand the kernels buffers past 2^31 and 2^32 bytes (a helper, not a conftest; tests/test_cpu_bigoffsets.py
proves on the CPU that the case tables cross what they claim and that the chunked comparison sees what it is for).

The hot path reaches memory through 32-bit unsigned buffer-descriptor offsets (the LDS-DMA GEMM kernels, the attention tile
loaders), through a host-side admission limit (csrc/gemm_plan.hpp: dma_operands_ok, operand bytes < 0xFFF00000) and through 64-bit
pointer arithmetic on int row indices (docs/OFFSET_RANGES.md).  A slip in any of them is invisible below 2^31 bytes, so:

  inputs      drawn on the device, random, never periodic in the row index: a read that wraps by 2^31 or 2^32 bytes lands on other
              values (test_cpu_bigoffsets.py shows the same wrap passing unnoticed on a periodic fill)
  outputs     guarded(): between two guard bands, the whole buffer prefilled with SENTINEL -- a value no result of these tests takes
  reference   the same operation in float64 on the device, in chunks of at most CHUNK rows (attention: of samples): no float64 copy of
              a whole operand ever exists
  comparison  every element / row of every chunk, under the bounds the other GEMM / LayerNorm / attention tests already use
              (tests/gemm_elem.py restated for device tensors below; tests/test_cpu_bigoffsets.py holds the two to equality), the worst
              kept per BAND of byte offsets of the tensor the case is about: below 2^31, [2^31, 2^32), from 2^32 on

Everything here runs on the device of the tensors it is handed, the CPU included."""
import gc
import math

import pytest
import torch

GiB = 1 << 30
B31, B32 = 1 << 31, 1 << 32
DMA_LIMIT = 0xFFF00000             # csrc/gemm_plan.hpp: dma_operands_ok
SENTINEL = -57344.0                # -1.75 * 2^15: exact in bfloat16, half and fp32; the operands of these tests give results below 1e3
GUARD_BYTES = 1 << 20
CHUNK = 65536
BUDGET = 24 * GiB
BANDS = ("below_2^31", "2^31_to_2^32", "from_2^32")
F64 = torch.float64
EPS32 = 2.0 ** -23


# ---------------------------------------------------------------------------------------------------------------- case tables
# GEMM: activation rows of 1024 16-bit elements (2048 bytes)
GEMM_ROW_BYTES = 2048
GEMM_M = {
    "past_2g": 1048576 + 256 + 37,     # crosses 2^31 bytes with a ragged last tile
    "last_admitted": 2096639,          # 4 293 916 672 bytes < 0xFFF00000: the last the LDS-DMA kernels take
    "first_declined": 2096640,         # exactly 0xFFF00000 bytes: the planner must name a kernel with 64-bit pointers
    "past_4g": 2097152 + 300,          # past 2^32 bytes: 64-bit path only
}
# what each GEMM tier claims of M * 2048: (lower bound, upper bound) in bytes, both inclusive
GEMM_CLAIMS = {"past_2g": (B31 + 1, B32 - 1), "last_admitted": (DMA_LIMIT - 2048, DMA_LIMIT - 1),
               "first_declined": (DMA_LIMIT, DMA_LIMIT), "past_4g": (B32 + 1, 2 * B32)}


def f32_rows(M):
    """rows of the fp32 form of a large-output case: rows twice as long, half as many (rounded up)"""
    return (M + 1) // 2


# attention: (H, HD, N, B, what passes 2^31 / 2^32 bytes).  N = one key past the first full key block of the fused backward (256 keys
# at head_dim 64, 512 at 32): the main kernel and the tail both run.
ATTN_CASES = {
    "hd64_qkv_2g": (16, 64, 257, 1365, ("qkv", B31)),
    "hd64_qkv_4g": (16, 64, 257, 2730, ("qkv", B32)),
    "hd32_qkv_2g": (8, 32, 513, 2730, ("qkv", B31)),
    "hd32_qkv_4g": (8, 32, 513, 5460, ("qkv", B32)),
    "hd64_o_2g": (16, 64, 257, 4081, ("o", B31)),
}


def attn_bytes(H, HD, N, B):
    """bytes of every device tensor of one attention case that is alive at once (chunk temporaries of the reference apart)"""
    tok = B * N * H * HD
    npad = (N + 63) // 64 * 64 + 64
    return {"qkv": 6 * tok, "dqkv": 6 * tok, "o": 2 * tok, "dout": 2 * tok, "lse": 4 * B * H * N, "rowc": 8 * B * H * N,
            "delta": 4 * B * N * H, "ws": 4 * (tok + 2 * B * H * npad)}


def attn_need(H, HD, N, B, chunk_samples):
    """stated device memory of an attention case: its tensors, the guard bands, and the float64 scores of one chunk of samples (the
    reference, its autograd and the rounding model keep about a dozen [chunk, H, N, N] float64 tensors)"""
    return sum(attn_bytes(H, HD, N, B).values()) + 8 * GUARD_BYTES + 14 * 8 * chunk_samples * H * N * N


# row and token kernels: name -> (rows M, row length D, bytes per element of the largest tensor, tier)
ROW_CASES = {
    "ln_d1024_2g": (524288 + 131, 1024, 4, B31), "ln_d1024_4g": (1048576 + 67, 1024, 4, B32),
    "ln_d512_2g": (1048576 + 131, 512, 4, B31), "ln_d512_4g": (2097152 + 67, 512, 4, B32),
    "ln_d1024_2g_elements": (2097152 + 2049, 1024, 4, None),
}
CAST_CASES = {"2g": (B31 // 4 + 8 * 131, 4), "4g": (B32 // 4 + 8 * 67, 4), "2g_elements": (B31 + 8 * 1031, 4)}     # n fp32 source elements


# ---------------------------------------------------------------------------------------------------------------- memory
def require(need_bytes):
    """skip (only) when the device has less free memory than the case's stated need + 2 GiB; the reason carries both numbers"""
    assert need_bytes <= BUDGET, f"a case may keep at most 24 GiB alive, this one states {need_bytes / GiB:.1f} GiB"
    free, _ = torch.cuda.mem_get_info()
    if free < need_bytes + 2 * GiB:
        pytest.skip(f"needs {need_bytes / GiB:.2f} GiB + 2 GiB of device memory, {free / GiB:.2f} GiB are free")


def release():
    """after the case's own `del`s: hand the memory back to the (shared) device"""
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- inputs, outputs
def chunks(M, step=CHUNK):
    return [(r0, min(r0 + step, M)) for r0 in range(0, M, step)]


def draw(shape, dtype, device, seed, scale=1.0, rowwise=None):
    """randn * scale in `dtype`, drawn chunk by chunk on the device (no fp32 copy of the whole tensor).  rowwise(r0, r1) -> [rows, 1]
    factor makes the rows non-exchangeable."""
    g = torch.Generator(device=device).manual_seed(seed)
    out = torch.empty(shape, dtype=dtype, device=device)
    flat = out.view(shape[0], -1)
    for r0, r1 in chunks(shape[0], max(1, min(1 << 24, (1 << 27) // flat.shape[1]))):      # at most 2^27 fp32 values at a time
        z = torch.randn((r1 - r0, flat.shape[1]), generator=g, device=device, dtype=torch.float32) * scale
        if rowwise is not None:
            z = z * rowwise(r0, r1)
        flat[r0:r1] = z.to(dtype)
    return out


def draw_int(shape, dtype, device, seed, lo=-2, hi=2):
    """uniform integers in {lo .. hi} in `dtype` (exact in every float type here): the operands of the weight-gradient cases"""
    g = torch.Generator(device=device).manual_seed(seed)
    out = torch.empty(shape, dtype=dtype, device=device)
    for r0, r1 in chunks(shape[0], max(1, min(1 << 24, (1 << 27) // max(1, math.prod(shape[1:]))))):
        out[r0:r1] = torch.randint(lo, hi + 1, (r1 - r0,) + tuple(shape[1:]), generator=g, device=device).to(dtype)
    return out


def exact_sum_limit_ok(M, amax=2):
    """every partial sum of M products of integers of magnitude <= amax is an integer of magnitude <= amax^2 M: exact in fp32 while
    that stays below 2^24"""
    return amax * amax * M < (1 << 24)


def guarded(shape, dtype, device, fill=SENTINEL):
    """(whole buffer, the tensor of `shape` in its middle): GUARD_BYTES of SENTINEL on either side, the output itself prefilled too"""
    n = math.prod(shape)
    g = GUARD_BYTES // torch.empty((), dtype=dtype).element_size()
    buf = torch.full((g + n + g,), fill, dtype=dtype, device=device)
    return buf, buf[g:g + n].view(shape)


def guards_intact(buf, out, fill=SENTINEL):
    g = (buf.numel() - out.numel()) // 2
    return bool((buf[:g] == fill).all()) and bool((buf[g + out.numel():] == fill).all())


# ---------------------------------------------------------------------------------------------------------------- comparison
class Worst:
    """the running worst per-row error per band of byte offsets; row r of the tensor the case is about starts at r * row_bytes"""

    def __init__(self, row_bytes, device, b31=B31, b32=B32):
        self.row_bytes, self.b31, self.b32 = row_bytes, b31, b32
        self.w = torch.zeros(3, dtype=F64, device=device)
        self.n = torch.zeros(3, dtype=torch.int64, device=device)

    def add(self, r0, err_rows):
        err = err_rows.to(F64).flatten()
        err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))      # a NaN row is the worst row
        off = (r0 + torch.arange(err.numel(), device=err.device, dtype=torch.int64)) * self.row_bytes
        band = (off >= self.b31).long() + (off >= self.b32).long()
        self.w.scatter_reduce_(0, band, err, "amax")
        self.n.scatter_add_(0, band, torch.ones_like(band))

    def result(self):
        """[worst of band 0, 1, 2]; None for a band without rows"""
        w, n = self.w.tolist(), self.n.tolist()
        return [w[i] if n[i] else None for i in range(3)]


def elem_ratio_rows(got, ref, bound):
    """[rows] the largest |got - ref| / bound of every row of a [rows, cols] chunk (tests/gemm_elem.py::worst: a NaN or a misplaced inf
    is an infinite error, got == ref is none).  bound None: equality -- 0 where every element is the reference's, inf elsewhere."""
    got, ref = got.to(F64), ref.to(F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if bound is None:
        e = torch.where(got == ref, 0.0, math.inf).to(F64)
    else:
        assert bool((bound > 0).all()), "every element needs a positive bound"
        e = (got - ref).abs() / bound
        e = torch.where(torch.isfinite(e), e, torch.full_like(e, math.inf))
        e = torch.where(got == ref, torch.zeros_like(e), e)
    return e.reshape(e.shape[0], -1).amax(dim=1)


def compare(got, row_bytes, chunk_fn, step=CHUNK, b31=B31, b32=B32, r_base=0):
    """The chunked comparison: chunk_fn(r0, r1) -> (ref, bound or None) for rows r0 .. r1 of `got` ([M, ...]); returns the worst
    ratio per band.  r_base: the row of the case's tensor that row 0 of `got` belongs to."""
    w = Worst(row_bytes, got.device, b31, b32)
    for r0, r1 in chunks(got.shape[0], step):
        ref, bound = chunk_fn(r0, r1)
        w.add(r_base + r0, elem_ratio_rows(got[r0:r1].reshape(r1 - r0, -1), ref.reshape(r1 - r0, -1),
                                           None if bound is None else bound.reshape(r1 - r0, -1)))
    return w.result()


def record(label, per_band, bound=1.0):
    """every band's worst error and its bound into the parity ledger (tests/conftest.py::parity asserts value <= bound); all bands are
    recorded before the first failure is raised"""
    from tests.conftest import parity
    fails = []
    for name, v in zip(BANDS, per_band):
        if v is None:
            continue
        try:
            parity(f"{label}/{name}", v, bound)
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, "; ".join(fails)


# ---------------------------------------------------------------------------------------------------------------- bounds (tests/gemm_elem.py on the device)
def lp_round_bound(ref, U, tiny):
    return 2.0 * U * ref.abs() + tiny


def acc_bound(absA, absB, terms, extra=None):
    """(terms + 4) 2^-23 (absA @ absB^T + extra): tests/gemm_elem.py::acc_bound for float64 tensors where they are"""
    s = absA @ absB.t()
    if extra is not None:
        s = s + extra
    return (terms + 4) * EPS32 * s


def gelu64(x):
    x = x.to(F64)
    return x * 0.5 * torch.special.erfc(-x / math.sqrt(2.0))


def dgelu64(x):
    x = x.to(F64)
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_bounds(x, U, tiny):
    x = x.to(F64)
    g = gelu64(x)
    low = x < -4.2
    return torch.where(low, torch.zeros_like(g), g), torch.where(low, torch.full_like(g, 6e-5), lp_round_bound(g, U, tiny) + 2e-5 * x.abs())


# ---------------------------------------------------------------------------------------------------------------- row metric (tests/rowwise.py on the device)
def attn_row_err_rows(got, ref):
    """tests/rowwise.py::row_err before its max: [B, H, N] of ||got_row - ref_row|| / max(||ref_row||, rms_n ||ref_row||), float64, on
    the device.  The floor is taken inside each (b, h), so chunks of samples give what the whole tensor gives."""
    got, ref = got.to(F64), ref.to(F64)
    rn = ref.norm(dim=-1)
    floor = rn.pow(2).mean(-1, keepdim=True).sqrt()
    e = (got - ref).norm(dim=-1) / torch.maximum(rn, floor).clamp_min(1e-300)
    return torch.where(torch.isfinite(e), e, torch.full_like(e, math.inf))


# ---------------------------------------------------------------------------------------------------------------- CPU model of a truncated offset
def truncated_gather(src, row_bytes, bits):
    """What a kernel reads that copies [M, D] rows with its byte offset kept in `bits` bits: row r comes from byte offset
    (r * row_bytes) mod 2^bits (the signed case, a store before the buffer, is truncated_scatter)."""
    M = src.shape[0]
    off = (torch.arange(M, dtype=torch.int64) * row_bytes) % (1 << bits)
    return src[off // row_bytes]


def truncated_scatter(buf, out, vals, row_bytes, bits):
    """What a kernel writes whose STORE offset is a signed `bits`-bit number: rows at and past 2^(bits-1) bytes land 2^bits bytes lower
    -- before the output, in the guard band of `buf` (the whole guarded buffer of `out`).  The band must be at least that wide."""
    g = (buf.numel() - out.numel()) // 2
    D = out.shape[1]
    for r in range(out.shape[0]):
        off = r * row_bytes
        if off >= 1 << (bits - 1):
            off -= 1 << bits
        e = g + off // out.element_size()
        assert e >= 0, "guard band narrower than the wrap"
        buf[e:e + D] = vals[r]
