"""CPU side of the eigen-smoothed CAM and the augmentation fold (csrc/saliency.hip: octmae_cam_eigen, octmae_cam_accumulate): the
references of tests/camsmooth_ref.py against each other, the thresholds tests/test_gpu_camsmooth.py relies on, the exported symbols and
the argument checks that refuse a call before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import camsmooth_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("octmae_cam_eigen_ws_floats", "octmae_cam_eigen", "octmae_cam_accumulate")
SHAPES = [(5, 4), (257, 64), (64, 1024), (1280, 256)]


@pytest.mark.parametrize("L,C", SHAPES)
def test_generator_plants_the_gap_that_was_asked(L, C):
    for ratio in (0.5, 0.8):
        A, w = R.planted(L, C, ratio, seed=L + C)
        assert A.dtype == np.float32 and A.shape == (L, C) and w.shape == (C,)
        assert 0.5 <= float(np.abs(w).min()) and float(np.abs(w).max()) <= 2.0
        assert C < 16 or ((w < 0).any() and (w > 0).any())
        _, _, s1, rho, margin = R.eigen_ref64(A, w)
        print(f"planted ({L}, {C}) ratio {ratio}: sigma1 {s1:.6f}, sigma2 / sigma1 {rho:.6f}, sign margin {margin:.3f}")
        assert abs(s1 - 1.0) <= 1e-3 and abs(rho - ratio) <= 0.1 * ratio
        # the offset is there (the columns are far from centred) and centring removes it
        assert float(np.abs(A.astype(np.float64).mean(0)).max()) > 0.5


@pytest.mark.parametrize("L,C", SHAPES)
def test_fp32_model_meets_the_svd_on_the_planted_cases(L, C):
    A, w = R.planted(L, C, 0.5, seed=L + C)
    p64, v64, s1, rho, margin = R.eigen_ref64(A, w)
    assert rho <= 0.55 and margin > 1e-3
    p, res, v = R.eigen_model32(A, w, 0, 32)
    err, bound = R.map_error(p, p64), R.model_bound(A, w, 0, s1, rho, 32)
    print(f"({L}, {C}) gap 0.5, 32 iterations: model error / max|p| {err:.3e} (bound {bound:.3e}), residual {res:.3e}, "
          f"float64 residual of the model's direction {R.residual64(A, w, 0, v):.3e}")
    assert err <= bound
    assert res < 1e-4 / 4                               # the GPU test asks < 1e-4 of the kernels
    assert np.array_equal(R.eigen_model32(A, w, 0, 32, relu=True)[0], np.maximum(p, np.float32(0)))
    # the oracle's own direction has no residual to speak of
    assert R.residual64(A, w, 0, v64) <= 1e-12


@pytest.mark.parametrize("L,C,seed", R.ITER_CASES)
def test_iteration_count_shows_in_the_residual(L, C, seed):
    """the thresholds of the GPU test (gap 0.8: residual > 5e-2 after 2 iterations, < 1e-4 after 32) on its inputs, with room on
    either side"""
    A, w = R.planted_batch(3, L, C, 0.8, seed, n_prefix=1)
    for b in range(3):
        _, _, _, rho, margin = R.eigen_ref64(A[b], w[b], 1)
        _, res2, v2 = R.eigen_model32(A[b], w[b], 1, 2)
        _, res32, _ = R.eigen_model32(A[b], w[b], 1, 32)
        print(f"({L}, {C}) sample {b}, gap {rho:.3f}: residual {res2:.3e} after 2 iterations, {res32:.3e} after 32; sign margin {margin:.2f}")
        assert res2 > 1.5 * R.RES_FEW and res32 < R.RES_MANY / 4 and margin >= R.MIN_MARGIN
        assert abs(res2 - R.residual64(A[b], w[b], 1, v2)) <= 1e-4      # the model's own residual is the float64 one of its direction


def test_degenerate_inputs_give_a_zero_map_and_a_zero_residual():
    g = np.random.default_rng(3)
    w = g.standard_normal(8).astype(np.float32)
    one_row = g.standard_normal((1, 8)).astype(np.float32)
    constant = np.repeat((g.integers(-8, 9, 8) / 4.0)[None, :], 6, axis=0).astype(np.float32)     # means that are exact in float32
    generic = g.standard_normal((6, 8)).astype(np.float32)
    for name, A, ww in (("L = 1", one_row, w), ("constant columns", constant, w), ("w = 0", generic, np.zeros(8, np.float32))):
        p, res, _ = R.eigen_model32(A, ww, 0, 4)
        p64, *_ = R.eigen_ref64(A, ww)
        assert not p.any() and res == 0.0 and not p64.any(), name
    p, res, _ = R.eigen_model32(np.vstack([np.full_like(one_row, 3e38), one_row]), w, 1, 4)      # the prefix row is not read
    assert not p.any() and res == 0.0
    bad = generic.copy()
    bad[2, 3] = np.nan
    assert np.isnan(R.eigen_model32(bad, w, 0, 4)[1])
    bad[2, 3] = np.inf
    assert np.isnan(R.eigen_model32(bad, w, 0, 4)[1])


def test_sign_rule_follows_the_centred_plain_cam():
    A, w = R.planted(33, 16, 0.5, seed=9)
    p64, v64, *_ = R.eigen_ref64(A, w)
    Mc = R._centred64(A, w, 0)
    assert float(p64 @ Mc.sum(1)) > 0 and np.allclose(Mc @ v64, p64)
    pm, _, _ = R.eigen_model32(A, -w, 0, 32)             # w -> -w mirrors Mc: the map flips with the plain CAM
    p, _, _ = R.eigen_model32(A, w, 0, 32)
    assert R.map_error(-pm, p.astype(np.float64)) <= 1e-4


def test_accumulate_reference_flips_rows_and_normalises_per_sample():
    g = np.random.default_rng(5)
    cam = g.standard_normal((2, 3 * 5)).astype(np.float32)
    cam[1] = cam[1] * 100 + 7
    a = R.accumulate_ref64(None, cam, 5, False, 0.5, True)
    assert a.min() == 0.0 and abs(a.max() - 0.5) <= 1e-6 and np.allclose(a[:, 0], 0.5 * (cam[:, 0] - cam.min(1)) / (cam.max(1) - cam.min(1)), atol=1e-6)
    f = R.accumulate_ref64(None, cam, 5, True, 0.5, True)
    assert np.array_equal(f.reshape(2, 3, 5)[:, :, ::-1], a.reshape(2, 3, 5))
    flipped = np.ascontiguousarray(cam.reshape(2, 3, 5)[:, :, ::-1]).reshape(2, 15)
    both = R.accumulate_ref64(a, flipped, 5, True, 0.5, False)
    assert np.allclose(both, 2 * a, atol=1e-12)
    assert not R.accumulate_ref64(None, np.full((1, 4), 3.25, np.float32), 4, True, 1.0, True).any()


# ---- the library ----------------------------------------------------------------------------------------------------------------------
def _libs():
    from octcubem_amd import _lib
    f16 = ctypes.CDLL(os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so"))
    for name in SYMBOLS:
        getattr(f16, name).argtypes = _lib.SIGNATURES[name]
        getattr(f16, name).restype = ctypes.c_int
    return [_lib.load(), f16]


def test_both_libraries_export_the_symbols_and_the_table_matches_the_header():
    from octcubem_amd import _lib
    assert _lib.expected_abi_version() >= 31
    hdr = open(os.path.join(ROOT, "include", "octmae.h")).read()
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float}
    for name in SYMBOLS:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", hdr, re.M)
        assert m, f"{name} is not declared in include/octmae.h"
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        want = [ctypes.c_void_p if "*" in a else ctype[a.split()[0]] for a in args]
        assert _lib.SIGNATURES[name] == want, (name, args)
    for lib in _libs():
        assert lib.octmae_abi_version() == _lib.expected_abi_version()
        for name in SYMBOLS:
            assert hasattr(lib, name), name


def test_argument_errors_are_reported_before_any_launch():
    buf = ctypes.create_string_buffer(256)
    q = (ctypes.addressof(buf) + 15) & ~15          # 16-byte aligned; never dereferenced: every call below is refused before a launch
    for lib in _libs():
        def eigen(A=q, w=q, cam=q, res=q, ws=q, B=3, L=5, npre=1, C=64, iters=8, relu=1):
            return lib.octmae_cam_eigen(A, w, cam, res, ws, B, L, npre, C, iters, relu, None)
        for null in ("A", "w", "cam", "res", "ws"):
            assert eigen(**{null: None}) == -1, null
        assert eigen(C=6) == -1 and eigen(C=0) == -1 and eigen(L=0) == -1 and eigen(B=0) == -1 and eigen(npre=-1) == -1
        assert eigen(iters=0) == -1 and eigen(iters=-3) == -1
        assert eigen(A=q + 4) == -1 and eigen(w=q + 8) == -1 and eigen(ws=q + 4) == -1
        assert eigen(B=65536) == -2
        # part [B][S][C] + partu [B][S] + abar, v, t [B][C] + u, c1 [B][L] + flag [B], each rounded up to 4 floats
        assert lib.octmae_cam_eigen_ws_floats(3, 5, 64) == 3 * 64 + 4 + 3 * 192 + 2 * 16 + 4
        assert lib.octmae_cam_eigen_ws_floats(1, 257, 8) == 5 * 8 + 8 + 3 * 8 + 2 * 260 + 4
        assert lib.octmae_cam_eigen_ws_floats(0, 5, 64) == -1 and lib.octmae_cam_eigen_ws_floats(65535, 5121, 1024) == -2

        def fold(acc=q, cam=q, mnmx=q, B=2, n=30, width=5, flip=1, weight=0.5, first=1):
            return lib.octmae_cam_accumulate(acc, cam, mnmx, B, n, width, flip, weight, first, None)
        for null in ("acc", "cam", "mnmx"):
            assert fold(**{null: None}) == -1, null
        assert fold(B=0) == -1 and fold(n=0) == -1 and fold(width=0) == -1 and fold(width=4) == -1 and fold(width=31) == -1
