"""tests/gemm_elem.py on the CPU, both sides: plain fp32 arithmetic on 16-bit-rounded operands stays inside the per-element bounds of
tests/test_gpu_gemm_elements.py whatever the order of its additions, the two activation formulas of csrc/common.hpp -- restated in
numpy fp32 -- stay inside theirs over EVERY finite 16-bit input, and each fault a tile kernel tends to have (one element, one k-tile,
one row slab, one wrong activation value) exceeds them."""
import numpy as np
import pytest
import torch

from tests import gemm_elem as GE

BF, HALF = torch.bfloat16, torch.float16
TYPES = [(BF, "bf16"), (HALF, "f16")]


def _tiny(dtype):
    return torch.finfo(dtype).tiny


def _operands(M, N, K, seed, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(dtype)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(dtype)
    return x, w


def _orders(x, w):
    """fp32 products of the rounded operands, summed in fp32 in different orders"""
    xf, wf = x.float(), w.float()
    K = xf.shape[1]
    out = {"plain": xf @ wf.t(), "reversed": xf.flip(1) @ wf.flip(1).t()}
    for parts in (2, 3, 7):
        acc = torch.zeros(xf.shape[0], wf.shape[0])
        for ks in torch.arange(K).chunk(parts):
            acc = acc + xf[:, ks] @ wf[:, ks].t()
        out[f"chunks{parts}"] = acc
    out["one_by_one"] = torch.zeros(xf.shape[0], wf.shape[0])
    for k in range(K):                                              # the longest chain of fp32 additions there is
        out["one_by_one"] = out["one_by_one"] + xf[:, k:k + 1] * wf[:, k:k + 1].t()
    return out


@pytest.mark.parametrize("K", [64, 72, 192, 1024, 1281])
def test_fp32_accumulation_in_any_order_stays_inside_acc_bound(K):
    """Largest ratio seen: 0.0102 (K = 64, torch's fp32 matmul and the strictly sequential sum alike), 0.008 at K = 72, 0.004 at 192,
    0.001 at 1024 and 1281 -- rounding errors of random signs add like sqrt(K), the bound like K, and most partial sums are far
    smaller than the sum of the magnitudes.  With a bias and a residual added in fp32 the ratio stays below 0.5 as well."""
    M, N = 48, 40
    x, w = _operands(M, N, K, K)
    ref = x.double() @ w.double().t()
    bound = GE.acc_bound(x.double().abs(), w.double().abs(), K)
    seen = {}
    for name, y in _orders(x, w).items():
        seen[name] = GE.worst(y, ref, bound, with_index=False)
        assert seen[name] <= 1.0, (name, seen[name])
    assert max(seen.values()) < 0.5, seen                            # the 2 x allowance is not what a correct sum lives on
    g = torch.Generator().manual_seed(K + 1)
    b, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    y = res + ((x.float() @ w.float().t()) + b)
    r = GE.worst(y, res.double() + ref + b.double(), GE.acc_bound(x.double().abs(), w.double().abs(), K, b.abs() + res.abs()), with_index=False)
    assert r < 0.5, r


def _lp_of(f32_array, dtype):
    return torch.from_numpy(np.ascontiguousarray(f32_array)).to(dtype)


@pytest.mark.parametrize("dtype,tag", TYPES)
def test_restated_activation_formulas_stay_inside_their_bounds_on_every_finite_input(dtype, tag):
    """gelu_f and dgelu_exact_f of csrc/common.hpp in fp32 (fma through float64) over all 65 280 / 63 488 finite values: the stored
    16-bit results are inside the bounds the GPU sweep applies, and the fp32 values themselves pin what the comments there say --
    |gelu_f(x) - gelu(x)| <= 1.73e-5 |x|, reached beyond the clamp where Phi_poly(4.2) = 1 - 1.72e-5 stands for 1 (more than the
    1.4e-5 once documented), |gelu' error| <= 2.8e-7 (2.56e-7 over the bfloat16 values, 2.79e-7 over the half ones)."""
    U, tiny = GE.LP_U[dtype], _tiny(dtype)
    x = GE.all_finite_lp(dtype)
    xf = x.float().numpy()
    act32, dg32 = GE.gelu_f32(xf), GE.dgelu_f32(xf)
    assert np.isfinite(act32).all() and np.isfinite(dg32).all()
    ref, bound = GE.gelu_bounds(x, U, tiny)
    r, idx = GE.worst(_lp_of(act32, dtype), ref, bound)
    assert r <= 1.0, (tag, r, idx, float(x[idx]))
    assert torch.isfinite(_lp_of(act32, dtype).float()).all()
    ref_d, bound_d = GE.dgelu_bounds(x, U, tiny)
    r, idx = GE.worst(_lp_of(dg32, dtype), ref_d, bound_d)
    assert r <= 1.0, (tag, r, idx, float(x[idx]))
    # the fp32 values before the 16-bit rounding
    xd = x.double()
    keep = (xd >= -4.2) & (xd != 0)
    rel = ((torch.from_numpy(act32).double() - GE.gelu64(xd)).abs() / xd.abs().clamp_min(1e-300))[keep]
    assert 1.4e-5 < float(rel.max()) <= 1.73e-5, float(rel.max())
    assert float(torch.from_numpy(act32).double()[xd < -4.2].abs().max()) == 0.0
    err_d = (torch.from_numpy(dg32).double() - ref_d).abs()
    assert float(err_d.max()) <= 2.8e-7, float(err_d.max())


# ------------------------------------------------------------------------------------------------ planted defects
def test_one_element_off_by_one_ulp_fails_bit_equality():
    for dtype, _ in TYPES:
        x, w = _operands(70, 50, 64, 3, dtype)
        y16 = (x.float() @ w.float().t()).to(dtype)
        assert GE.bit_exact(y16, y16.clone()) == (0.0, (0, 0))
        for idx in ((0, 0), (69, 49), (33, 7)):
            bad = y16.clone()
            bad.view(torch.int16)[idx] += 1                          # the next number of the type, away from zero
            r, where = GE.bit_exact(bad, y16)
            assert r > 1.0 and where == idx, (r, where, idx)
        z = torch.zeros(4, 4, dtype=dtype)
        neg = z.clone(); neg[2, 1] = -0.0
        r, where = GE.bit_exact(neg, z)                              # the sign of a zero is a bit, too
        assert r > 1.0 and where == (2, 1)


def test_one_element_holding_its_neighbours_value_is_caught():
    M, N, K = 300, 264, 192
    x, w = _operands(M, N, K, 5)
    ref = x.double() @ w.double().t()
    bound = GE.acc_bound(x.double().abs(), w.double().abs(), K)
    y = x.float() @ w.float().t()
    assert GE.worst(y, ref, bound, with_index=False) <= 1.0
    for idx in ((0, 0), (299, 262), (128, 127)):
        bad = y.clone()
        bad[idx] = y[idx[0], idx[1] + 1]
        r, where = GE.worst(bad, ref, bound)
        assert r > 1.0 and where == idx, (r, where)
        # ... and through the 16-bit rounding allowance of a dgrad-type output as well
        r16, where16 = GE.worst(bad.to(BF), ref, GE.lp_round_bound(ref, GE.LP_U[BF], _tiny(BF)) + bound)
        assert r16 > 1.0 and where16 == idx, (r16, where16)
    nan = y.clone(); nan[7, 9] = float("nan")
    assert GE.worst(nan, ref, bound) == (float("inf"), (7, 9))
    with pytest.raises(AssertionError):
        GE.worst(y, ref, torch.zeros_like(ref))


@pytest.mark.parametrize("twice", [False, True], ids=["left_out", "counted_twice"])
def test_one_k_tile_of_one_tile_is_caught(twice):
    """64 of 1024 terms missing from (or doubled in) one 128 x 128 tile of a 257 x 256 output: every element of that tile is outside
    its bound (bar the few whose 64 terms happen to cancel), no element of another tile is."""
    M, N, K = 257, 256, 1024
    x, w = _operands(M, N, K, 7)
    ref = x.double() @ w.double().t()
    bound = GE.acc_bound(x.double().abs(), w.double().abs(), K)
    y = x.float() @ w.float().t()
    part = x.float()[128:256, 64:128] @ w.float()[128:256, 64:128].t()
    bad = y.clone()
    bad[128:256, 128:256] += part if twice else -part
    assert GE.worst(y, ref, bound, with_index=False) <= 1.0
    r, (i, j) = GE.worst(bad, ref, bound)
    assert r > 1.0 and 128 <= i < 256 and 128 <= j < 256, (r, i, j)
    hit = ((bad.double() - ref).abs() / bound > 1.0)
    assert int(hit.sum()) > 0.99 * 128 * 128 and not bool(hit[:128].any()) and not bool(hit[:, :128].any())


def test_last_ragged_slab_missing_from_one_column_sum_is_caught():
    """The rows after the last whole 64-row slab (44 of 300; the ONE row of 65) left out of one of 264 column sums."""
    g = torch.Generator().manual_seed(11)
    for M in (65, 300):
        dx = torch.randn(M, 264, generator=g).to(BF)
        cs0 = torch.randn(264, generator=g)
        ref = cs0.double() + dx.double().sum(0)
        bound = GE.sum_bound(dx.double().abs().sum(0), M + 4, cs0.abs())          # (M + 8) 2^-23 (|cs0| + sum |dx|)
        cs = cs0 + dx.float().sum(0)
        assert GE.worst(cs, ref, bound, with_index=False) <= 1.0
        for col in (0, 131, 263):
            bad = cs.clone()
            bad[col] -= dx.float()[(M - 1) // 64 * 64:, col].sum()
            r, where = GE.worst(bad, ref, bound)
            assert r > 1.0 and where == (col,), (M, col, r, where)


def test_the_polynomial_gelu_prime_is_caught_through_the_half_rounding_allowance():
    """dgelu_poly_f's documented error level (4.4e-4) at ONE input, x = -3 where gelu' = -0.0119: the half build's allowance there is
    2 * 2^-12 * 0.0119 + 6.1e-5 + 1e-6 = 6.8e-5.  (At inputs where |gelu'| is near 1 one half rounding is 4.9e-4 by itself: there
    such an error hides in the type, not in the test.)"""
    U, tiny = GE.LP_U[HALF], _tiny(HALF)
    x = GE.all_finite_lp(HALF)
    ref, bound = GE.dgelu_bounds(x, U, tiny)
    good = _lp_of(GE.dgelu_f32(x.float().numpy()), HALF)
    assert GE.worst(good, ref, bound, with_index=False) <= 1.0
    idx = tuple(int(i) for i in (x == -3.0).nonzero()[0])
    bad = good.clone()
    bad[idx] = (good[idx].float() + 4.4e-4).to(HALF)
    r, where = GE.worst(bad, ref, bound)
    assert r > 1.0 and where == idx, (r, where)


def test_gelu_without_its_low_branch_is_caught():
    """x * Phi_poly(-4.2) at x = -65 504 is -1.12 (Phi_poly(-4.2) = 1.72e-5), where |act| <= 6e-5 is asked"""
    for dtype, _ in TYPES:
        U, tiny = GE.LP_U[dtype], _tiny(dtype)
        x = GE.all_finite_lp(dtype)
        ref, bound = GE.gelu_bounds(x, U, tiny)
        bad = _lp_of(GE.gelu_f32(x.float().numpy(), low_branch=False), dtype)
        idx = tuple(int(i) for i in (x.float() == -65504.0).nonzero()[0]) if dtype == HALF else None
        err = (bad.double() - ref).abs() / bound
        assert GE.worst(bad, ref, bound, with_index=False) > 1.0
        if idx is not None:
            assert float(err[idx]) > 1.0 and abs(float(bad[idx]) + 1.12) < 0.05, (float(err[idx]), float(bad[idx]))


def test_all_finite_lp_and_half_spacing():
    for dtype, _ in TYPES:
        x = GE.all_finite_lp(dtype)
        flat = x.flatten()
        n = GE.N_FINITE[dtype]
        assert x.shape == (256, 256) and bool(torch.isfinite(flat.float()).all()) and bool((flat[n:] == 0).all())
        assert len(set(flat[:n].view(torch.int16).tolist())) == n                       # every pattern once
        assert float(flat.float().max()) == torch.finfo(dtype).max and float(flat.float().min()) == -torch.finfo(dtype).max
        pos = flat[:n].view(torch.int16).to(torch.int32)
        pos = flat[:n][(pos >= 0)].double().sort().values                               # +0 ... the largest number
        gap = pos[1:] - pos[:-1]
        assert torch.equal(2 * GE.half_spacing(pos[:-1], dtype), gap)                   # the spacing above each value
