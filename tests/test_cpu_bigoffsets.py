"""What the tests past 2^31 / 2^32 bytes rest on, shown without a GPU: the case tables cross what they claim (shape arithmetic only), the
GEMM planner changes kernels exactly at the admission limit of the LDS-DMA kernels, the weight-gradient operands keep every fp32
partial sum exact, the device-side bounds of tests/bigoffset_ref.py are those of tests/gemm_elem.py, and the chunked comparison flags
each kind of offset slip on a small model of "offset truncated to k bits" -- and does NOT see a wrapped read on a periodic input,
which is why the inputs of those tests are random."""
import ctypes
import os

import pytest
import torch

from tests import bigoffset_ref as BR
from tests import gemm_elem as GE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B31, B32 = BR.B31, BR.B32


# ------------------------------------------------------------------------------------------------ the case tables
def test_gemm_tiers_cross_what_they_claim():
    for name, M in BR.GEMM_M.items():
        lo, hi = BR.GEMM_CLAIMS[name]
        assert lo <= M * BR.GEMM_ROW_BYTES <= hi, (name, M * BR.GEMM_ROW_BYTES)
    assert BR.GEMM_M["last_admitted"] * 2048 == BR.DMA_LIMIT - 2048 == 4293916672          # one row below the limit
    assert BR.GEMM_M["first_declined"] * 2048 == BR.DMA_LIMIT                              # exactly on it
    assert BR.GEMM_M["past_2g"] % 256 != 0 and BR.GEMM_M["past_2g"] % 128 != 0             # a ragged last tile of either size
    # large outputs: [M, 1024] in 16 bits and [ceil(M / 2), 1024] in fp32 are the same bytes (+ at most one row)
    for name, M in BR.GEMM_M.items():
        assert 0 <= BR.f32_rows(M) * 4096 - M * 2048 <= 2048
    assert BR.f32_rows(BR.GEMM_M["past_2g"]) * 4096 > B31 and BR.f32_rows(BR.GEMM_M["past_4g"]) * 4096 > B32


def test_attention_cases_cross_what_they_claim_within_the_budget():
    for name, (H, HD, N, B, (tensor, limit)) in BR.ATTN_CASES.items():
        nb = BR.attn_bytes(H, HD, N, B)
        assert nb[tensor] > limit, (name, nb[tensor])
        assert nb["qkv"] == B * N * 3 * H * HD * 2 and nb["o"] * 3 == nb["qkv"]
        if limit == B31 and tensor == "qkv":
            assert nb["qkv"] < B32 and nb["o"] < B31
        assert N * 3 * H * HD * 2 < 1 << 24                          # one sample is small: the N^2 work stays trivial
        assert N % {64: 256, 32: 512}[HD] == 1                       # one key past the first full key block of the fused backward
        assert B <= 65535                                            # the batch index is the grid's z
        assert BR.attn_need(H, HD, N, B, 16) <= BR.BUDGET, (name, BR.attn_need(H, HD, N, B, 16) / BR.GiB)
    assert BR.attn_bytes(16, 64, 257, 4081)["ws"] > B32              # the fp32 dQ workspace of the largest case is itself past 2^32


def test_row_cases_cross_what_they_claim():
    for name, (M, D, es, limit) in BR.ROW_CASES.items():
        if limit is None:
            assert M * D > B31, name                                 # elements, not bytes
        else:
            assert limit < M * D * es < 2 * limit, name
        assert D % 4 == 0 and M % 4 != 0                             # an odd row count: the last workgroup is ragged
    for name, (n, es) in BR.CAST_CASES.items():
        assert n % 8 == 0
        assert (n > B31) if name.endswith("elements") else (n * es > (B31 if name == "2g" else B32))


# ------------------------------------------------------------------------------------------------ the planner at the admission edge
def _plan(lib, kind, NA, NB, K, lda, ldb, variant=0, splitk=0):
    out = (ctypes.c_int * 13)()
    rc = lib.octmae_gemm_plan(kind, NA, NB, K, lda, ldb, variant, splitk, 1, 256, out)
    return rc, list(out)


def _libraries():
    from octcubem_amd import _lib
    libs = [_lib.load()]
    f16 = os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so")
    if os.path.exists(f16):
        libs.append(ctypes.CDLL(f16))
    return libs


@pytest.mark.parametrize("what", ["forward", "dgrad", "wgrad", "wgrad_bias"])
def test_plan_changes_kernel_exactly_at_the_dma_limit(what):
    """forward x [M, 1024] @ w [256, 1024]^T, dgrad dy [M, 1024] @ w [1024, 256], wgrad dy [M, 1024]^T x [M, 1024]: a 256-tile LDS-DMA
    kernel (plan kernel 1 or 2) at M = 2 096 639, the register-staged kernel with 64-bit pointers (0) from M = 2 096 640 on"""
    for lib in _libraries():
        for M, dma in ((BR.GEMM_M["past_2g"], True), (BR.GEMM_M["last_admitted"], True), (BR.GEMM_M["first_declined"], False),
                       (BR.GEMM_M["past_4g"], False)):
            args = {"forward": (0, 256, M, 1024, 1024, 1024), "dgrad": (1, 256, M, 1024, 256, 1024),
                    "wgrad": (5, 1024, 1024, M, 1024, 1024), "wgrad_bias": (6, 1024, 1024, M, 1024, 1024)}[what]
            rc, out = _plan(lib, *args)
            assert rc == 0, (what, M, rc)
            assert (out[0] in (1, 2)) == dma and (dma or out[0] == 0), (what, M, out)
            for variant in (0x200, 0x400, 0x1000):                   # a forced DMA kernel does not override the limit
                rc, out = _plan(lib, *args, variant=variant)
                assert rc == 0 and (dma or out[0] == 0), (what, M, variant, out)
        # the fused dgrad + delta has no register-staged form: past the limit it answers -2 and the caller falls back
        assert _plan(lib, 4, 1024, BR.GEMM_M["last_admitted"], 1024, 1024, 1024)[0] == 0
        assert _plan(lib, 4, 1024, BR.GEMM_M["first_declined"], 1024, 1024, 1024)[0] == -2


def test_wgrad_cases_stay_exact():
    """integer operands in {-2 .. 2}: |partial sum| <= 4 M < 2^24 at every tier, so fp32 accumulation in any order, split or not, is
    exact and the kernel must EQUAL float64"""
    for name, M in BR.GEMM_M.items():
        assert 4 * M < 1 << 24 and BR.exact_sum_limit_ok(M), name
    assert not BR.exact_sum_limit_ok(1 << 22)
    x = BR.draw_int((1000, 8), torch.bfloat16, "cpu", 3)
    assert set(x.float().unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}


# ------------------------------------------------------------------------------------------------ the bounds are the project's own
def test_device_side_bounds_equal_gemm_elem():
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(37, 24, generator=g).double(), torch.randn(19, 24, generator=g).double()
    extra = torch.randn(37, 19, generator=g).double().abs()
    assert torch.equal(BR.acc_bound(a.abs(), b.abs(), 24, extra), GE.acc_bound(a.abs(), b.abs(), 24, extra))
    x = (4 * torch.randn(4096, generator=g)).bfloat16()
    for dt in (torch.bfloat16, torch.float16):
        U, tiny = GE.LP_U[dt], torch.finfo(dt).tiny
        assert torch.equal(BR.lp_round_bound(a, U, tiny), GE.lp_round_bound(a, U, tiny))
        for mine, theirs in zip(BR.gelu_bounds(x, U, tiny), GE.gelu_bounds(x, U, tiny)):
            assert torch.equal(mine, theirs)
    assert torch.equal(BR.dgelu64(x), GE.dgelu64(x)) and BR.EPS32 == GE.EPS32
    got, ref, bound = a + 1e-3 * extra.sum(1, keepdim=True)[:, :24], a, a.abs() * 1e-2 + 1e-6
    assert float(BR.elem_ratio_rows(got, ref, bound).max()) == pytest.approx(GE.worst(got, ref, bound, with_index=False), rel=1e-12)


def test_row_metric_equals_rowwise_on_chunks():
    from tests import rowwise as RW
    g = torch.Generator().manual_seed(6)
    ref = torch.randn(5, 3, 17, 8, generator=g).double()
    got = ref + 1e-3 * torch.randn(5, 3, 17, 8, generator=g).double()
    whole = RW.row_err(got, ref)
    by_chunk = max(float(BR.attn_row_err_rows(got[i:i + 2], ref[i:i + 2]).max()) for i in range(0, 5, 2))
    assert by_chunk == pytest.approx(whole, rel=1e-12)


# ------------------------------------------------------------------------------------------------ the checker sees what it is for
BITS, ROWB, M_SMALL, D_SMALL = 16, 256, 700, 128        # 2-byte elements: rows of 256 bytes; 2^15 bytes = row 128, 2^16 bytes = row 256


def _copy_case(periodic=False):
    g = torch.Generator().manual_seed(11)
    src = torch.randn(M_SMALL, D_SMALL, generator=g).bfloat16()
    if periodic:
        src = src[:64].repeat(11, 1)[:M_SMALL].contiguous()          # period 64 rows = 2^14 bytes: divides both wrap distances
    return src


def _check(got, src, step=100):
    return BR.compare(got, ROWB, lambda r0, r1: (src[r0:r1].double(), None), step=step, b31=1 << (BITS - 1), b32=1 << BITS)


def test_checker_passes_the_correct_copy_and_names_the_bands():
    src = _copy_case()
    assert _check(src.clone(), src) == [0.0, 0.0, 0.0]
    w = BR.Worst(ROWB, "cpu", 1 << 15, 1 << 16)
    w.add(0, torch.zeros(100))
    assert w.result() == [0.0, None, None]                           # rows 0 .. 99 end below 2^15 bytes


def test_checker_flags_a_read_wrapped_by_2_to_the_k():
    src = _copy_case()
    got = BR.truncated_gather(src, ROWB, BITS)
    assert torch.equal(got[:256], src[:256]) and not torch.equal(got[256], src[256])
    lo, mid, hi = _check(got, src)
    assert lo == 0.0 and mid == 0.0 and hi == float("inf")
    lo, mid, hi = _check(BR.truncated_gather(src, ROWB, BITS - 1), src)       # a 31-bit slip
    assert lo == 0.0 and mid == float("inf") and hi == float("inf")


def test_checker_misses_the_same_wrap_on_a_periodic_input():
    src = _copy_case(periodic=True)
    for bits in (BITS, BITS - 1):
        got = BR.truncated_gather(src, ROWB, bits)
        assert _check(got, src) == [0.0, 0.0, 0.0], "a period that divides the wrap distance hides the wrap"


def test_checker_flags_a_signed_wrap_through_the_guard_band():
    src = _copy_case()[:200]                                         # rows from 128 on are at or past 2^15 bytes
    buf, out = BR.guarded((200, D_SMALL), torch.bfloat16, "cpu")
    assert BR.guards_intact(buf, out)
    BR.truncated_scatter(buf, out, src, ROWB, BITS)
    assert not BR.guards_intact(buf, out)                            # the stores landed before the buffer
    lo, mid, hi = BR.compare(out, ROWB, lambda r0, r1: (src[r0:r1].double(), None), step=64, b31=1 << 15, b32=1 << 16)
    assert lo == 0.0 and mid == float("inf") and hi is None          # and the rows they were meant for kept the sentinel
    assert bool((out[128:] == BR.SENTINEL).all())


def test_checker_flags_rows_left_at_the_sentinel_and_one_wrong_row():
    src = _copy_case()
    buf, out = BR.guarded((M_SMALL, D_SMALL), torch.bfloat16, "cpu")
    out.copy_(src)
    out[300:364] = BR.SENTINEL                                       # a band of rows that never arrived
    assert _check(out, src) == [0.0, 0.0, float("inf")]
    out.copy_(src)
    out[256] = src[255]                                              # one wrong row, the first at 2^16 bytes
    assert _check(out, src) == [0.0, 0.0, float("inf")]
    out.copy_(src)
    out[128, 5] = out[128, 5] * 1.01                                 # one element of the first row at 2^15 bytes, under a bound
    bound = lambda r0, r1: (src[r0:r1].double(), 2.0 ** -9 * src[r0:r1].double().abs() + 1e-30)        # noqa: E731
    lo, mid, hi = BR.compare(out, ROWB, bound, step=100, b31=1 << 15, b32=1 << 16)
    assert lo == 0.0 and mid > 1.0 and hi == 0.0
    assert BR.guards_intact(buf, out)


def test_record_writes_every_band_to_the_ledger_before_failing():
    from tests import conftest
    n0 = len(conftest._LEDGER)
    BR.record("bigoffset/selftest", [0.5, None, 0.25])
    assert [l for l, _, _ in conftest._LEDGER[n0:]] == ["bigoffset/selftest/below_2^31", "bigoffset/selftest/from_2^32"]
    with pytest.raises(AssertionError):
        BR.record("bigoffset/selftest_fail", [2.0, 0.5, 0.5])
    assert len(conftest._LEDGER) == n0 + 5
    del conftest._LEDGER[n0:]
