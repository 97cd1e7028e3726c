"""CPU side of the slab LayerNorm (csrc/slabnorm.hip): the element order and the "a slab is contiguous" claim against einops, bit for
bit; the bounds of tests/slabnorm_ref.py on a plain fp32 evaluation in another summation order (must pass) and on seven planted faults
(each must fail); the ABI number, the exported symbols of both libraries and the argument errors, reported before any launch."""
import ctypes
import os

import pytest
import torch

from tests import slabnorm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-5
F32 = torch.float32


def test_row_r_is_the_contiguous_slab_read_transposed():
    """Row n T + t of the reference's patch matrix, built by einops on the strided view the reference makes, is the contiguous slab
    x[n][n_prefix + t L .. n_prefix + (t + 1) L)[0..C) with element k = c L + l equal to S[l][c]: the same bits."""
    for N, T, L, C, n_prefix in ((2, 3, 9, 8, 1), (1, 2, 5, 16, 0), (2, 1, 1, 8, 2)):
        x = torch.randn(N, n_prefix + T * L, C, generator=torch.Generator().manual_seed(N + L))
        view = x[:, n_prefix:, :].reshape(N, T, L, C).transpose(2, 3)
        assert view.data_ptr() == x[:, n_prefix:].data_ptr() and not view.is_contiguous()       # the reference hands over a strided view
        rows = R.patch_rows(x, T, L, n_prefix)
        assert rows.shape == (N, T, C * L)
        flat = x.reshape(-1)
        for n in range(N):
            for t in range(T):
                start = (n * (n_prefix + T * L) + n_prefix + t * L) * C
                slab = flat[start:start + L * C].view(L, C)                                         # contiguous memory
                assert torch.equal(rows[n, t].view(torch.int32), slab.t().reshape(-1).view(torch.int32))
                k = torch.arange(C * L)
                assert torch.equal(rows[n, t], slab[k % L, k // L])                                 # k = c L + l  <->  S[l][c]


def _sum_other_order(t, dim):
    """an fp32 sum along `dim` in an order no kernel uses: strided thirds, each added back to front"""
    t = t.movedim(dim, -1).flip(-1)
    parts = [t[..., i::3].sum(-1, dtype=F32) for i in range(3)]
    return (parts[2] + parts[0]) + parts[1]


def emulate(x, gamma, beta, dA, T, L, n_prefix, lp_dtype, fault=None, start_gamma=None, start_beta=None):
    """The kernels' arithmetic in plain fp32 torch (every sum through _sum_other_order), with one planted fault."""
    N, tokens, C = x.shape
    K, Rn = C * L, N * T
    first = 0 if fault == "stats_from_token_0" else n_prefix
    slabs = x[:, n_prefix:n_prefix + T * L].reshape(N, T, L, C)
    stat_slabs = x[:, first:first + T * L].reshape(N, T, L, C).reshape(Rn, K)
    if fault == "naive_variance":
        mean = _sum_other_order(stat_slabs, 1) / K
        var = _sum_other_order(stat_slabs * stat_slabs, 1) / K - mean * mean
    else:
        mean = _sum_other_order(stat_slabs, 1) / K
        var = _sum_other_order((stat_slabs - mean[:, None]) ** 2, 1) / (K - 1 if fault == "k_minus_1" else K)
    rstd = 1.0 / torch.sqrt(var + EPS)
    if fault == "order_lc":
        rows = slabs.reshape(Rn, K)                                   # k = l C + c
    else:
        rows = slabs.transpose(2, 3).reshape(Rn, K)                   # k = c L + l
    xh = (rows - mean[:, None]) * rstd[:, None]
    A = (xh * gamma + beta).to(lp_dtype).float()
    if fault == "dropped_l":
        A[Rn - 1, (C - 1) * L + (L - 1)] = 0.0                        # the last l of the last tile column was never written
    g = dA * gamma
    m1, m2 = _sum_other_order(g, 1) / K, _sum_other_order(g * xh, 1) / K
    dS = rstd[:, None] * (g - m1[:, None] - xh * m2[:, None])
    dx = torch.zeros_like(x)
    dx[:, n_prefix:] = dS.reshape(N, T, C, L).transpose(2, 3).reshape(N, T * L, C)
    if fault == "prefix_not_zero" and n_prefix:
        dx[N - 1, 0, C - 1] = 1e-30
    used = slice(0, Rn - 1) if fault == "row_missing" else slice(0, Rn)
    sg = torch.zeros(K) if start_gamma is None else start_gamma
    sb = torch.zeros(K) if start_beta is None else start_beta
    dgamma = sg + _sum_other_order((dA * xh)[used], 0)
    dbeta = sb + _sum_other_order(dA[used], 0)
    return {"mean": mean, "rstd": rstd, "A": A, "dx": dx, "dgamma": dgamma, "dbeta": dbeta}


SHAPES = ((2, 3, 9, 8, 1), (1, 1, 16, 64, 0), (2, 3, 65, 72, 1))


@pytest.mark.parametrize("lp", (torch.bfloat16, torch.float16))
@pytest.mark.parametrize("kind", ("plain", "offset"))
def test_fp32_in_another_summation_order_stays_inside_the_bounds(kind, lp):
    for N, T, L, C, n_prefix in SHAPES:
        x, gamma, beta, dA = R.draw(N, T, L, C, n_prefix, kind, seed=3, lp_dtype=lp)
        sg, sb = torch.randn(C * L), torch.randn(C * L)
        e = R.measure(x, gamma, beta, dA, T, L, n_prefix, lp, emulate(x, gamma, beta, dA, T, L, n_prefix, lp, None, sg, sb), sg, sb)
        assert max(e.values()) <= 1.0, (kind, lp, (N, T, L, C, n_prefix), e)


def test_constant_slab_gives_the_rounded_bias():
    x, gamma, beta, dA = R.draw(2, 3, 9, 8, 1, "const", seed=4)
    got = emulate(x, gamma, beta, dA, 3, 9, 1, torch.bfloat16)
    assert torch.equal(got["A"], beta.to(torch.bfloat16).float().expand(6, -1))
    assert torch.equal(got["mean"], x[:, 1:].reshape(6, -1)[:, 0])


@pytest.mark.parametrize("fault,kind,where", (
    ("order_lc", "plain", ("A", "dx", "dgamma")),
    ("stats_from_token_0", "plain", ("mean", "rstd", "A")),
    ("k_minus_1", "plain", ("rstd",)),
    ("dropped_l", "plain", ("A",)),
    ("row_missing", "plain", ("dgamma", "dbeta")),
    ("prefix_not_zero", "plain", ("dx",)),
    ("naive_variance", "offset", ("rstd",)),
))
def test_every_planted_fault_leaves_the_bounds(fault, kind, where):
    N, T, L, C, n_prefix = SHAPES[0]
    lp = torch.float16
    x, gamma, beta, dA = R.draw(N, T, L, C, n_prefix, kind, seed=5, lp_dtype=lp)
    e = R.measure(x, gamma, beta, dA, T, L, n_prefix, lp, emulate(x, gamma, beta, dA, T, L, n_prefix, lp, fault))
    for q in where:
        assert e[q] > 1.0, (fault, q, e)
    clean = R.measure(x, gamma, beta, dA, T, L, n_prefix, lp, emulate(x, gamma, beta, dA, T, L, n_prefix, lp))
    assert max(clean.values()) <= 1.0, clean


# ------------------------------------------------------------------------------------------------ the C ABI
def test_both_libraries_export_the_symbols_at_abi_28():
    from octcubem_amd import _lib
    names = ("octmae_slab_norm_fwd", "octmae_slab_norm_bwd", "octmae_slabnorm_ws_floats")
    assert _lib.expected_abi_version() >= 28 and all(n in _lib.SIGNATURES for n in names)
    header = open(_lib.HEADER_PATH).read()
    f16 = ctypes.CDLL(os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so"))
    for n in names:
        assert hasattr(_lib.load(), n) and hasattr(f16, n) and f"int {n}(" in header
    assert f16.octmae_abi_version() == _lib.load().octmae_abi_version() == _lib.expected_abi_version()


def test_argument_errors_are_reported_without_a_gpu():
    from octcubem_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    q = (ctypes.addressof(buf) + 15) & ~15          # 16-byte aligned; never dereferenced: every call below is refused before a launch

    def fwd(x=q, gamma=q, beta=q, a=q, mean=q, rstd=q, ws=q, N=2, T=3, L=9, C=8, n_prefix=1, eps=1e-5):
        return lib.octmae_slab_norm_fwd(x, gamma, beta, a, mean, rstd, ws, N, T, L, C, n_prefix, eps, None)

    def bwd(da=q, x=q, mean=q, rstd=q, gamma=q, dx=q, dgamma=None, dbeta=None, ws=q, N=2, T=3, L=9, C=8, n_prefix=1):
        return lib.octmae_slab_norm_bwd(da, x, mean, rstd, gamma, dx, dgamma, dbeta, ws, N, T, L, C, n_prefix, None)

    for null in ("x", "gamma", "beta", "a", "mean", "rstd", "ws"):
        assert fwd(**{null: None}) == -1, null
    for null in ("da", "x", "mean", "rstd", "gamma", "dx", "ws"):
        assert bwd(**{null: None}) == -1, null
    shapes = (dict(C=12), dict(C=4), dict(C=0), dict(C=-8), dict(L=0), dict(T=0), dict(N=0), dict(n_prefix=-1), dict(N=-1), dict(L=-3),
              dict(C=1 << 20, L=1 << 11),           # C L above 2^30
              dict(N=1 << 13, T=1 << 12))           # N T above 2^24
    for bad in shapes:
        assert fwd(**bad) == -1 and bwd(**bad) == -1, bad
        if "n_prefix" not in bad:
            args = {**dict(N=2, T=3, L=9, C=8), **bad}
            assert lib.octmae_slabnorm_ws_floats(*[args[k] for k in "NTLC"]) == -1, bad
    assert fwd(eps=-1.0) == -1
    for odd in ("x", "gamma", "beta", "a", "ws"):
        assert fwd(**{odd: q + 4}) == -1, odd
    for odd in ("da", "x", "gamma", "dx", "ws"):
        assert bwd(**{odd: q + 4}) == -1, odd
    # the workspace covers both calls: the forward's chunk pairs and the backward's tile sums and row-group partials
    assert lib.octmae_slabnorm_ws_floats(2, 3, 9, 8) >= max(2 * 6 * 1, 2 * 6 + 2 * 6 + 2 * 6 * 72)
    assert lib.octmae_slabnorm_ws_floats(8, 20, 256, 1024) > 0
