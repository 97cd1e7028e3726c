"""CPU side of the saliency kernels (csrc/saliency.hip): the exported symbols, the argument checks that refuse a call before any launch,
the restatements of tests/saliency_ref.py against themselves and against F.interpolate, the planted faults the Grad-CAM bound must
catch, and the ops.weight_grads switch."""
import ctypes
import os

import pytest
import torch

from tests import saliency_ref as R
from tests.gemm_elem import worst

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("octmae_patch_scatter", "octmae_cam_weights", "octmae_cam_tokens", "octmae_heatmap")


def _libs():
    from octcubem_amd import _lib
    f16 = ctypes.CDLL(os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so"))
    for name in SYMBOLS + ("octmae_cam_ws_floats",):
        getattr(f16, name).argtypes = _lib.SIGNATURES[name]
        getattr(f16, name).restype = ctypes.c_int
    return [_lib.load(), f16]


def test_both_libraries_export_the_symbols_at_abi_23():
    from octcubem_amd import _lib
    assert _lib.expected_abi_version() >= 23
    for lib in _libs():
        assert lib.octmae_abi_version() == _lib.expected_abi_version()
        for name in SYMBOLS:
            assert name in _lib.SIGNATURES and hasattr(lib, name), name


def test_argument_errors_are_reported_before_any_launch():
    buf = ctypes.create_string_buffer(256)
    q = (ctypes.addressof(buf) + 15) & ~15          # 16-byte aligned; never dereferenced: every call below is refused before a launch
    for lib in _libs():
        def scatter(dp=q, ids=q, is64=1, out=q, B=2, C=1, T=6, H=32, W=32, tp=3, p=16, nkeep=4):
            return lib.octmae_patch_scatter(dp, ids, is64, out, B, C, T, H, W, tp, p, nkeep, None)
        assert scatter(dp=None) == -1 and scatter(out=None) == -1
        assert scatter(p=12, H=36, W=36) == -1 and scatter(p=4) == -1                 # p % 8
        assert scatter(H=40) == -1 and scatter(W=40) == -1                            # H % p, W % p
        assert scatter(T=7) == -1                                                     # T % tp
        assert scatter(nkeep=9) == -1 and scatter(nkeep=0) == -1                      # L = 2 * 2 * 2 = 8
        assert scatter(p=0) == -1 and scatter(tp=0) == -1 and scatter(B=0) == -1 and scatter(C=0) == -1
        assert scatter(dp=q + 2) == -1 and scatter(out=q + 4) == -1                   # 16-byte accesses

        def weights(G=q, w=q, ws=q, B=3, L=5, npre=1, C=64):
            return lib.octmae_cam_weights(G, w, ws, B, L, npre, C, None)

        def tokens(A=q, w=q, cam=q, B=3, L=5, npre=1, C=64):
            return lib.octmae_cam_tokens(A, w, cam, B, L, npre, C, None)
        for null in ("G", "w", "ws"):
            assert weights(**{null: None}) == -1, null
        for null in ("A", "w", "cam"):
            assert tokens(**{null: None}) == -1, null
        for f in (weights, tokens):
            assert f(C=6) == -1 and f(C=0) == -1 and f(L=0) == -1 and f(B=0) == -1 and f(npre=-1) == -1
        assert lib.octmae_cam_ws_floats(3, 5, 64) == 3 * 64 and lib.octmae_cam_ws_floats(1, 257, 8) == 5 * 8
        assert lib.octmae_cam_ws_floats(0, 5, 64) == -1

        def heat(m=q, mnmx=q, out=q, B=1, t=2, h=2, w=3, F=6, H=32, W=48):
            return lib.octmae_heatmap(m, mnmx, out, B, t, h, w, F, H, W, None)
        for null in ("m", "mnmx", "out"):
            assert heat(**{null: None}) == -1, null
        assert heat(W=46) == -1 and heat(W=2) == -1                                   # W % 4
        for zero in ("B", "t", "h", "w", "F", "H", "W"):
            assert heat(**{zero: 0}) == -1, zero
        assert heat(out=q + 2) == -1


@pytest.mark.parametrize("C,tp,p,T,H,W,nkeep", [(1, 3, 16, 6, 32, 48, 3), (3, 1, 16, 3, 16, 16, 3), (1, 1, 8, 2, 16, 24, 12)])
def test_scatter_restatement_is_the_exact_adjoint_of_the_gather_restatement(C, tp, p, T, H, W, nkeep):
    g = torch.Generator().manual_seed(C + tp + p)
    B = 2
    L = (T // tp) * (H // p) * (W // p)
    ids = torch.stack([torch.randperm(L, generator=g)[:nkeep] for _ in range(B)])
    # small integers: every product and every partial sum is exact in float64, so the two sides are EQUAL, not close
    x = torch.randint(-8, 9, (B, C, T, H, W), generator=g).to(R.F64)
    y = torch.randint(-8, 9, (B * nkeep, C * tp * p * p), generator=g).to(R.F64)
    lhs = (R.gather_ref(x, ids, tp, p, nkeep) * y).sum()
    sc = R.scatter_ref(y, ids, (B, C, T, H, W), tp, p)
    assert float(lhs) == float((x * sc).sum()) and float(lhs) != 0.0
    # scatter after gather keeps the kept voxels and zeroes the rest; gather after scatter is the identity
    assert torch.equal(R.gather_ref(sc, ids, tp, p, nkeep), y)
    kept = R.scatter_ref(torch.ones_like(y), ids, (B, C, T, H, W), tp, p)
    assert torch.equal(R.scatter_ref(R.gather_ref(x, ids, tp, p, nkeep), ids, (B, C, T, H, W), tp, p), x * kept)
    assert int(kept.sum()) == B * nkeep * C * tp * p * p
    # ids None = the first nkeep tokens
    assert torch.equal(R.gather_ref(x, None, tp, p, nkeep), R.gather_ref(x, torch.arange(nkeep).expand(B, nkeep), tp, p, nkeep))


@pytest.mark.parametrize("name", list(R.HEAT_CASES))
def test_heat_restatement_equals_interpolate_on_the_normalised_map(name):
    m, size = R.heat_input(name)
    mine = R.heat_value64(m, size)
    ref = R.heat_interpolate(m, size, torch.float64)
    assert mine.shape == ref.shape == (m.shape[0], *size)
    assert float((mine - ref).abs().max()) <= 1e-9              # 255 v: float64 rounding of two formulations of the same weights
    b64 = R.heat_ref64(m, size)
    b32 = R.heat_ref32(m, size)
    d = (b64.int() - b32.int()).abs()
    # what tests/test_gpu_saliency.py allows the kernel: fp32 arithmetic moves a byte only across a floor, and rarely
    assert int(d.max()) <= 1 and float((d != 0).double().mean()) <= 0.01
    if name == "identity":          # equal sizes: the smallest voxel is 0, the largest 254 or 255
        assert int(b64.min()) == 0 and int(b64.max()) in (254, 255) and int(b32.min()) == 0 and int(b32.max()) in (254, 255)


def test_heat_restatement_identity_and_constant_map():
    m, size = R.heat_input("identity")
    v = R.heat_value64(m, size)
    mn, mx = float(m.min()), float(m.max())
    exp = 255.0 * ((m.double() - mn) / (float(torch.tensor(1e-7)) + (mx - mn)))
    assert torch.equal(v, exp)                                  # equal sizes: the resampling matrices are identities
    assert int(R.heat_ref64(torch.full((2, 2, 3, 4), 3.25), (4, 8, 8)).max()) == 0
    assert torch.equal(R._lin_matrix(5, 5), torch.eye(5, dtype=R.F64))


@pytest.mark.parametrize("C,L,npre", [(4, 1, 0), (64, 5, 1), (1024, 257, 1)])
def test_cam_bound_holds_for_fp32_torch_and_catches_planted_faults(C, L, npre):
    g = torch.Generator().manual_seed(C + L)
    A = torch.randn(3, npre + L, C, generator=g)
    G = torch.randn(3, npre + L, C, generator=g)
    G[0] = G[0].abs() * A[0].sign()          # sample 0: every product of the mean with A is positive -> cam well above 0 in every row
    w64, wb, cam64, cb = R.cam_ref64(A, G, npre)
    w32 = G[:, npre:].sum(1) / L
    cam32 = torch.einsum("bc,blc->bl", w32, A[:, npre:]).clamp_min(0)
    assert worst(w32, w64, wb, with_index=False) <= 1.0 and worst(cam32, cam64, cb, with_index=False) <= 1.0
    if L > 1:                                # one dropped token row in the mean
        w_bad = G[:, npre:-1].sum(1) / L
        assert worst(w_bad, w64, wb, with_index=False) > 1.0
        assert worst(torch.einsum("bc,blc->bl", w_bad, A[:, npre:]).clamp_min(0), cam64, cb, with_index=False) > 1.0
    # one dropped group of 4 columns in the dot product
    cam_bad = torch.einsum("bc,blc->bl", w32[:, :-4], A[:, npre:, :-4]).clamp_min(0) if C > 4 else torch.zeros_like(cam32)
    assert worst(cam_bad, cam64, cb, with_index=False) > 1.0


def test_weight_grads_switch_nests_and_restores_on_exception():
    from octcubem_amd import ops
    assert ops.weight_grads_enabled() is True
    with ops.weight_grads(False):
        assert ops.weight_grads_enabled() is False
        with ops.weight_grads(True):
            assert ops.weight_grads_enabled() is True
            with ops.weight_grads(False):
                assert ops.weight_grads_enabled() is False
            assert ops.weight_grads_enabled() is True
        assert ops.weight_grads_enabled() is False
    assert ops.weight_grads_enabled() is True
    with pytest.raises(KeyError):
        with ops.weight_grads(False):
            with ops.weight_grads(False):
                raise KeyError("boom")
    assert ops.weight_grads_enabled() is True
    ctx = ops.weight_grads(False)               # one object, entered twice
    with ctx:
        with ctx:
            assert ops.weight_grads_enabled() is False
        assert ops.weight_grads_enabled() is False
    assert ops.weight_grads_enabled() is True
