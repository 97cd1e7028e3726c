"""GPU: the slab LayerNorm kernels (csrc/slabnorm.hip) directly through the C ABI, every output element against the float64 reference
in the reference's own order and the per-element bounds of tests/slabnorm_ref.py (proven on the CPU by tests/test_cpu_slabnorm.py).

Shapes: the smallest at which this can go wrong.  C in {8, 64, 192} and one c-tile edge (56 / 64 / 72: C comes in eights); L in
{1, 9, 16} and one below, at and past the 64-row l-tile (63, 64, 65); T in {1, 3} and N in {1, 2} (1, 3 and 6 rows); n_prefix in {0, 1};
both store paths (L % 8 == 0: 16-byte pieces; otherwise element by element); a row of two statistics chunks with a partial last one
(K = 18432 > 16384); and one shape with more tiles than the dx kernel has workgroups to give every row its own (105 tiles, 6 rows in
5 row groups: one workgroup walks two rows and the dgamma / dbeta partials are folded).  Inputs: slabs that are not exchangeable,
1000 + noise, and constant slabs, for which A must equal lp(beta) bit for bit.

Every output and the workspace sit between guard elements that must keep their value; the workspace is handed over filled with the
guard value (it needs no initialisation); prefix rows of dx are exact zeros; dgamma / dbeta accumulate onto a non-zero start; NULL
pointers change nothing else; two runs are bit-equal.  The same checks run on the half-operand build in a child process
(tests/f16_worker.py)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import _lib, ops
from tests import children
from tests import slabnorm_ref as R

DEV = "cuda"
EPS = 1e-5
GUARD = 256            # elements in front of and behind every output (a multiple of 8: the 16-byte alignment survives in both widths)
SENTINEL = -7680.0     # exact in fp32, bfloat16 and half

# (N, T, L, C, n_prefix, kind)
CASES = [(1, 1, 1, 8, 0, "plain"), (2, 3, 1, 8, 1, "plain"), (1, 3, 9, 8, 1, "plain"), (2, 3, 9, 64, 0, "plain"), (2, 1, 16, 8, 1, "plain"),
         (1, 3, 16, 192, 1, "plain"), (2, 3, 9, 192, 1, "plain"), (1, 1, 16, 64, 0, "plain"),
         (1, 3, 63, 56, 1, "plain"), (2, 3, 64, 64, 1, "plain"), (1, 3, 65, 72, 0, "plain"), (2, 1, 64, 72, 1, "plain"), (1, 1, 65, 56, 1, "plain"),
         (2, 3, 9, 8, 1, "offset"), (1, 3, 16, 64, 1, "offset"), (2, 3, 65, 72, 1, "offset"),
         (2, 3, 9, 8, 1, "const"), (1, 3, 64, 64, 0, "const"), (2, 1, 65, 72, 1, "const"),
         (1, 3, 96, 192, 1, "plain"),              # two statistics chunks per row, the second partial
         (2, 3, 2240, 192, 1, "plain")]            # 105 tiles x 6 rows: 5 row groups, one of them walks two rows
IDS = [f"N{c[0]}T{c[1]}L{c[2]}C{c[3]}p{c[4]}{c[5]}" for c in CASES]


def _guarded(n, dtype=torch.float32, fill=SENTINEL):
    """(whole buffer, the n elements in its middle)"""
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    mid = buf[GUARD:GUARD + n]
    if fill != SENTINEL:
        mid.fill_(fill)
    return buf, mid


def _guards_intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def check_case(N, T, L, C, n_prefix, kind, report=None):
    lp = ops.BF16
    K, rows = C * L, N * T
    x, gamma, beta, dA = R.draw(N, T, L, C, n_prefix, kind, seed=7 + L + C, lp_dtype=lp)
    xd, gd, bd, dAd = x.to(DEV), gamma.to(DEV), beta.to(DEV), dA.to(DEV).to(lp)
    nws = _lib.load().octmae_slabnorm_ws_floats(N, T, L, C)
    assert nws > 0
    st = ops._stream()

    def forward():
        o = {"A": _guarded(rows * K, lp), "mean": _guarded(rows), "rstd": _guarded(rows), "ws": _guarded(nws)}
        _lib.call("octmae_slab_norm_fwd", xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), o["A"][1].data_ptr(), o["mean"][1].data_ptr(),
                  o["rstd"][1].data_ptr(), o["ws"][1].data_ptr(), N, T, L, C, n_prefix, EPS, st)
        torch.cuda.synchronize()
        for k, n in (("A", rows * K), ("mean", rows), ("rstd", rows), ("ws", nws)):
            assert _guards_intact(o[k][0], n), f"forward wrote outside {k}"
        return o["A"][1].view(rows, K), o["mean"][1], o["rstd"][1]

    A, mean, rstd = forward()
    A2, mean2, rstd2 = forward()
    assert torch.equal(_bits(A), _bits(A2)) and torch.equal(_bits(mean), _bits(mean2)) and torch.equal(_bits(rstd), _bits(rstd2))
    if kind == "const":
        assert torch.equal(_bits(A), _bits(bd.to(lp).expand(rows, K))), "a constant slab must give lp(beta)"
        assert torch.equal(mean.cpu(), x[:, n_prefix:].reshape(rows, -1)[:, 0])

    sg = torch.randn(K, generator=torch.Generator().manual_seed(1))
    sb = torch.randn(K, generator=torch.Generator().manual_seed(2))

    def backward(want_g=True, want_b=True):
        o = {"dx": _guarded(x.numel()), "dgamma": _guarded(K), "dbeta": _guarded(K), "ws": _guarded(nws)}
        o["dgamma"][1].copy_(sg)
        o["dbeta"][1].copy_(sb)
        _lib.call("octmae_slab_norm_bwd", dAd.data_ptr(), xd.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gd.data_ptr(),
                  o["dx"][1].data_ptr(), o["dgamma"][1].data_ptr() if want_g else None, o["dbeta"][1].data_ptr() if want_b else None,
                  o["ws"][1].data_ptr(), N, T, L, C, n_prefix, st)
        torch.cuda.synchronize()
        for k, n in (("dx", x.numel()), ("dgamma", K), ("dbeta", K), ("ws", nws)):
            assert _guards_intact(o[k][0], n), f"backward wrote outside {k}"
        return o["dx"][1].view(x.shape), o["dgamma"][1], o["dbeta"][1]

    dx, dgamma, dbeta = backward()
    dx2, dgamma2, dbeta2 = backward()
    assert torch.equal(_bits(dx), _bits(dx2)) and torch.equal(_bits(dgamma), _bits(dgamma2)) and torch.equal(_bits(dbeta), _bits(dbeta2))
    if n_prefix:
        assert int((_bits(dx[:, :n_prefix]) != 0).sum()) == 0, "prefix rows of dx must be +0"
    # NULL pointers: nothing is computed for them, their buffers keep the start value, everything else is bit-identical
    dx3, g3, b3 = backward(want_g=False, want_b=False)
    assert torch.equal(_bits(dx3), _bits(dx)) and torch.equal(g3.cpu(), sg) and torch.equal(b3.cpu(), sb)
    dx4, g4, b4 = backward(want_g=True, want_b=False)
    assert torch.equal(_bits(dx4), _bits(dx)) and torch.equal(_bits(g4), _bits(dgamma)) and torch.equal(b4.cpu(), sb)
    dx5, g5, b5 = backward(want_g=False, want_b=True)
    assert torch.equal(_bits(dx5), _bits(dx)) and torch.equal(g5.cpu(), sg) and torch.equal(_bits(b5), _bits(dbeta))

    got = {"mean": mean, "rstd": rstd, "A": A.float(), "dx": dx, "dgamma": dgamma, "dbeta": dbeta}
    e = R.measure(x, gamma, beta, dA, T, L, n_prefix, lp, got, sg, sb, eps=EPS)
    if report is not None:
        report[(N, T, L, C, n_prefix, kind)] = e
    print(f"[slabnorm {lp}] N{N} T{T} L{L} C{C} p{n_prefix} {kind}: " + ", ".join(f"{k} {v:.3f}" for k, v in e.items()) + " of the bound")
    bad = {k: v for k, v in e.items() if not v <= 1.0}
    assert not bad, (N, T, L, C, n_prefix, kind, bad)


def check_wrappers():
    """ops.slab_norm_fwd / _bwd: the refusals raise before a launch, and the wrapper gives the C ABI's bits"""
    x, gamma, beta, dA = R.draw(2, 3, 9, 8, 1, "plain", seed=3, lp_dtype=ops.BF16)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    A, mean, rstd = ops.slab_norm_fwd(xd, gd, bd, EPS, 3, 9, 1)
    assert A.shape == (6, 72) and A.dtype == ops.BF16 and mean.shape == (6,)
    dx = ops.slab_norm_bwd(dA.to(DEV).to(ops.BF16), xd, mean, rstd, gd, 3, 9, 1)
    assert dx.shape == x.shape and int((_bits(dx[:, 0]) != 0).sum()) == 0
    with pytest.raises(ValueError):
        ops.slab_norm_fwd(xd, gd, bd, EPS, 3, 8, 1)                   # 28 tokens are not 1 + 3 * 8
    with pytest.raises(ValueError):
        ops.slab_norm_fwd(xd, gd[:-8].clone(), bd, EPS, 3, 9, 1)      # gamma too short
    with pytest.raises(ValueError):
        ops.slab_norm_fwd(xd[:, :, :4].contiguous(), gd, bd, EPS, 3, 9, 1)          # C = 4
    with pytest.raises(RuntimeError):
        ops.slab_norm_fwd(xd.transpose(0, 1), gd, bd, EPS, 3, 9, 1)   # not contiguous
    with pytest.raises(RuntimeError):
        ops.slab_norm_fwd(x, gamma, beta, EPS, 3, 9, 1)               # CPU tensors: there is no fallback
    with pytest.raises(ValueError):
        ops.slab_norm_bwd(dA.to(DEV).to(ops.BF16)[:5], xd, mean, rstd, gd, 3, 9, 1)


def run_all_checks():
    rep = {}
    for c in CASES:
        check_case(*c, report=rep)
    check_wrappers()
    return rep


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_slab_norm_forward_and_backward_per_element(case):
    check_case(*case)


def test_wrappers_refuse_before_launching():
    check_wrappers()


def half_build_cases():
    """What tests/f16_worker.py runs on the half-operand build; a failed check ends it with a traceback and a non-zero status."""
    return {"cases": len(run_all_checks())}


def test_same_checks_on_the_half_operand_build():
    children.spawn_f16_worker("slabnorm_f16", "tests.test_gpu_slabnorm_kernels:half_build_cases")
    meta = children.f16_worker_result("slabnorm_f16")
    assert meta["lib"] == "liboctmae_f16.so" and meta["lp_is_f16"] is True and meta["cases"] == len(CASES)
