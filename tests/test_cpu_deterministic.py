"""Deterministic mode without a GPU: the switch, the ABI, and the planner (csrc/gemm_plan.hpp) -- host arithmetic only -- plus the numpy
model of the fold order that the GPU oracle of tests/test_gpu_deterministic.py is built on.

The plans of the DEFAULT mode are queried by a module fixture before the first test of this module runs -- in a session's order
(test_cpu_* first) before any test has touched the option -- and test_option_off_restores_every_plan compares against them.  Nothing
is loaded or computed at import: with OCTMAE_DETERMINISTIC set in the environment the tests of this module fail, the collection of
the session does not."""
import ctypes

import numpy as np
import pytest

from octcubem_amd import _lib
from tests import deterministic_ref as D

LIB = None                   # the library and the size of its split-K workspace: set by the module fixture
WS = 0
CUS = 256
BASELINE = {}
SLOTS = 64 << 20             # the bytes of the split-K workspace in front of its arrival counters: what the slabs may take


def _all_plans():
    """every plan of the sweep under the current option, old and new queries, as one comparable structure"""
    got = {}
    for N, K, M in D.sweep_singles():
        for kind in (5, 6):
            got[("s", kind, N, K, M)] = (D.gemm_plan(LIB, kind, N, K, M, WS, CUS), D.gemm_plan(LIB, kind, N, K, M, 0, CUS),
                                          D.gemm_plan_old(LIB, kind, N, K, M, 1, CUS), D.gemm_plan_old(LIB, kind, N, K, M, 0, CUS))
        p = D.gemm_plan(LIB, 5, N, K, M, WS, CUS)[1]
        got[("b", N, K, M)] = D.split_bounds(LIB, M, p["slices"], p["tiles_a"] * p["tiles_b"])
    for a, b, M in D.sweep_pairs():
        got[("p", a, b, M)] = (D.pair_plan(LIB, a, b, M, WS, CUS), D.pair_plan(LIB, a, b, M, 0, CUS), D.pair_plan_old(LIB, a, b, M, CUS))
    # kinds 2 / 3: dgrad x GELU' with the column sums, without / with the per-slab workspace (fc1's bias gradient)
    for M in (4096, 1281, 300):
        for K in (256, 1024, 136):
            for kind in (2, 3):
                out = (ctypes.c_int * 13)()
                rc = LIB.octmae_gemm_plan(kind, K, M, 512, K, 512, 0, 1, 1, CUS, out)
                got[("d", kind, M, K)] = (rc, list(out))
    return got


@pytest.fixture(scope="module", autouse=True)
def _default_plans():
    global LIB, WS
    LIB = _lib.load()
    WS = D.split_ws_bytes(LIB)
    assert LIB.octmae_deterministic() == 0, "these tests need the default mode at start (OCTMAE_DETERMINISTIC must not be set)"
    if not BASELINE:
        BASELINE.update(_all_plans())


@pytest.fixture
def deterministic():
    prev = LIB.octmae_set_option(b"deterministic", 1)
    try:
        yield
    finally:
        LIB.octmae_set_option(b"deterministic", prev)


def test_switch_abi_and_symbols():
    assert LIB.octmae_abi_version() == 35 == _lib.expected_abi_version()
    for name in ("octmae_deterministic", "octmae_wgrad_accum_pair_ws", "octmae_wgrad_det_ws_bytes", "octmae_wgrad_fold",
                 "octmae_gemm_plan_ws", "octmae_wgrad_pair_plan_ws", "octmae_mt_sumsq_ws", "octmae_mt_adamw_fused_ws"):
        assert name in _lib.SIGNATURES and hasattr(LIB, name), name
    prev = LIB.octmae_set_option(b"deterministic", 1)
    try:
        assert prev == 0
        assert LIB.octmae_set_option(b"deterministic", 1) == 1
        assert LIB.octmae_deterministic() == 1
        assert LIB.octmae_set_option(b"deterministic", 7) == 1 and LIB.octmae_deterministic() == 1      # any non-zero value is "on"
    finally:
        LIB.octmae_set_option(b"deterministic", 0)
    assert LIB.octmae_deterministic() == 0


def test_python_switch_round_trip():
    import octcubem_amd
    from octcubem_amd import ops
    assert octcubem_amd.set_deterministic is ops.set_deterministic
    assert ops.is_deterministic() is False
    prev = ops.set_deterministic(True)
    try:
        assert prev is False and ops.is_deterministic() is True
        assert ops.set_deterministic(True) is True
    finally:
        ops.set_deterministic(False)
    assert ops.is_deterministic() is False


def test_workspace_query():
    """column-sum rows at the head (a single launch with a bias gradient; a pair always, for its wider dY) + the slabs"""
    M = 8192
    assert LIB.octmae_colsum_ws_rows(M) > 0 and LIB.octmae_colsum_ws_rows(200) == 0
    assert D.ws_bytes_for(LIB, 256, 512, 0, 0, M, False, 1) == 0            # one slice, no bias gradient: nothing
    assert D.ws_bytes_for(LIB, 256, 512, 0, 0, M, False, 3) == 3 * 256 * 512 * 4
    assert D.ws_bytes_for(LIB, 256, 512, 0, 0, M, True, 3) == D.colsum_head(LIB, M, 256) + 3 * 256 * 512 * 4
    assert D.ws_bytes_for(LIB, 256, 512, 0, 0, 200, True, 3) == 3 * 256 * 512 * 4          # few rows: one split, no rows to park
    assert D.ws_bytes_for(LIB, 4096, 1024, 1024, 4096, M, False, 2) == D.colsum_head(LIB, M, 4096) + 2 * 2 * 4096 * 1024 * 4
    b = ctypes.c_longlong(0)
    assert LIB.octmae_wgrad_det_ws_bytes(0, 512, 0, 0, M, 0, 2, ctypes.byref(b)) == -1
    assert LIB.octmae_wgrad_det_ws_bytes(8, 8, 0, 0, M, 0, 0, ctypes.byref(b)) == -1
    assert LIB.octmae_wgrad_det_ws_bytes(8, 8, 8, 0, M, 0, 2, ctypes.byref(b)) == -1 and LIB.octmae_wgrad_det_ws_bytes(8, 8, 0, 0, M, 0, 2, None) == -1


def _check_cover(M, slices, tiles):
    d, b = D.split_bounds(LIB, M, slices, tiles)
    ktiles = (M + D.TK - 1) // D.TK
    assert d == 0, "deterministic mode runs equal slices"
    assert b[0] == 0 and b[-1] == ktiles and all(b[z] < b[z + 1] for z in range(slices)), (M, slices, b)
    rows = D.slice_rows(b, M)
    assert rows[0][0] == 0 and rows[-1][1] == M and all(rows[z][1] == rows[z + 1][0] for z in range(slices - 1))
    assert all(r1 > r0 for r0, r1 in rows), "no slice is empty"


def test_planner_sweep_single_launches(deterministic):
    split, staggered_before = 0, 0
    for N, K, M in D.sweep_singles():
        for kind in (5, 6):
            (rc0, base), _, _, _ = BASELINE[("s", kind, N, K, M)]
            rc, p = D.gemm_plan(LIB, kind, N, K, M, WS, CUS)
            assert rc == 0 == rc0
            what = (kind, N, K, M, p)
            assert p["kstagger"] == 0, what
            assert p["colsum"] != D.COLSUM_FUSED and (kind == 5 or p["colsum"] == 3), what          # 3: the fixed-order pass before the GEMM
            assert 1 <= p["slices"] <= base["slices"], what                                          # the default's split, capped
            assert (p["atomic1"] == D.ROUTE_SLABS) == (p["slices"] > 1), what
            need = D.ws_bytes_for(LIB, N, K, 0, 0, M, kind == 6, p["slices"])
            assert p["slices"] == 1 or p["slices"] * N * K * 4 <= need <= SLOTS, what
            # the query is what a caller sizes the workspace from: lending exactly that runs exactly these slices, one byte less does not
            if p["slices"] > 1:
                assert D.gemm_plan(LIB, kind, N, K, M, need, CUS)[1]["slices"] == p["slices"], what
                assert D.gemm_plan(LIB, kind, N, K, M, need - 1, CUS)[1]["slices"] < p["slices"], what
            assert (p["kernel"], p["tiles_a"], p["tiles_b"], p["cgroup"]) == (base["kernel"], base["tiles_a"], base["tiles_b"], base["cgroup"]), what
            assert p["grid"] == p["tiles_a"] * p["tiles_b"] * p["slices"], what
            _check_cover(M, p["slices"], p["tiles_a"] * p["tiles_b"])
            ktiles = -(-M // D.TK)
            assert p["per"] == -(-ktiles // p["slices"]), what
            split += p["slices"] > 1
            staggered_before += base["kstagger"] > 0
            # without a workspace, or with one too small for two slabs: unsplit, never atomics
            for ws in (0, 2 * N * K * 4 - 4):
                rc, q = D.gemm_plan(LIB, kind, N, K, M, ws, CUS)
                assert rc == 0 and q["slices"] == 1 and q["atomic1"] != D.ROUTE_SLABS and q["kstagger"] == 0, (ws, what, q)
            rc, q = D.gemm_plan_old(LIB, kind, N, K, M, 0, CUS)
            assert rc == 0 and q["slices"] == 1, (what, q)
    assert split > 100, "the sweep must contain split launches, or it proves nothing"
    assert staggered_before > 0, "the sweep must contain launches the default mode staggers"


def test_a_small_workspace_caps_the_split(deterministic):
    """M = 8192, N = K = 256: 16 slices by default; a workspace of 2 (3, 5) slabs gives exactly that many or fewer, equal, non-empty"""
    N = K = 256
    M = 8192
    assert BASELINE[("s", 5, N, K, M)][0][1]["slices"] >= 8
    for fit in (2, 3, 5):
        rc, p = D.gemm_plan(LIB, 5, N, K, M, fit * N * K * 4 + 100, CUS)
        assert rc == 0 and 2 <= p["slices"] <= fit and p["atomic1"] == D.ROUTE_SLABS, (fit, p)
        _check_cover(M, p["slices"], 1)
    # with the bias gradient the head of the workspace holds the column-sum rows: the slabs get what is left
    need = D.ws_bytes_for(LIB, N, K, 0, 0, M, True, 2)
    assert need == D.colsum_head(LIB, M, N) + 2 * N * K * 4 > 2 * N * K * 4
    rc, p = D.gemm_plan(LIB, 6, N, K, M, need, CUS)
    assert rc == 0 and p["slices"] == 2, p
    rc, p = D.gemm_plan(LIB, 6, N, K, M, need - 8, CUS)
    assert rc == 0 and p["slices"] == 1, p


def test_planner_sweep_pairs(deterministic):
    split = 0
    for a, b, M in D.sweep_pairs():
        (rc0, base), _, _ = BASELINE[("p", a, b, M)]
        rc, p = D.pair_plan(LIB, a, b, M, WS, CUS)
        assert rc == rc0
        if rc != 0:
            continue
        what = (a, b, M, p)
        assert p["kstagger"] == 0 and p["colsum"] == 3, what
        assert (p["atomic1"] == D.ROUTE_SLABS) == (p["slices"] > 1), what
        assert 1 <= p["slices"] <= base["slices"] or p["kernel"] != base["kernel"], what
        need = D.ws_bytes_for(LIB, a[0], a[1], b[0], b[1], M, True, p["slices"])
        slabs = p["slices"] * (a[0] * a[1] + b[0] * b[1]) * 4 if p["slices"] > 1 else 0
        assert need == D.colsum_head(LIB, M, max(a[0], b[0])) + slabs and need <= SLOTS, what
        if p["slices"] > 1:
            assert D.pair_plan(LIB, a, b, M, need, CUS)[1]["slices"] == p["slices"], what
            q = D.pair_plan(LIB, a, b, M, need - 1, CUS)[1]
            assert q["slices"] < p["slices"] or q["kernel"] != p["kernel"], what
        if p["kernel"] == 3 and p["slices"] > 1:
            assert p["nst"] == 4, what               # a split 128-tile pair runs on the 4-stage ring only in this mode
        _check_cover(M, p["slices"], p["ta0"] * p["tb0"] + p["ta1"] * p["tb1"])
        split += p["slices"] > 1
        for q in (D.pair_plan(LIB, a, b, M, 0, CUS), D.pair_plan_old(LIB, a, b, M, CUS)):
            assert q[0] == 0 and q[1]["slices"] == 1 and q[1]["atomic1"] != D.ROUTE_SLABS, (what, q)
    assert split >= 8


def test_dgelu_column_sums_never_ride_on_atomics(deterministic):
    seen = set()
    for (tag, *key), val in BASELINE.items():
        if tag != "d":
            continue
        kind, M, K = key
        out = (ctypes.c_int * 13)()
        rc = LIB.octmae_gemm_plan(kind, K, M, 512, K, 512, 0, 1, 1, CUS, out)
        assert rc == val[0] == 0
        assert out[12] in ((2, 4) if kind == 3 else (4,)), (kind, M, K, list(out))     # FoldWs with a workspace lent, else the pass after
        assert list(out)[:12] == val[1][:12], "nothing but the column-sum route moves"
        seen.add((kind, val[1][12], out[12]))
    assert (2, 1, 4) in seen, "the sweep must contain a launch whose default route is the atomic one"


def test_option_off_restores_every_plan():
    prev = LIB.octmae_set_option(b"deterministic", 1)
    try:
        assert _all_plans() != BASELINE
    finally:
        LIB.octmae_set_option(b"deterministic", prev)
    assert _all_plans() == BASELINE


def test_default_mode_ignores_the_workspace_size():
    """with the option off the new queries report what the old ones do, whatever workspace is lent"""
    for N, K, M in D.sweep_singles()[::7]:
        for kind in (5, 6):
            with_ws, without, old_ws, old_none = BASELINE[("s", kind, N, K, M)]
            assert with_ws == old_ws and without == old_none and with_ws[1]["slices"] == without[1]["slices"]
    for a, b, M in D.sweep_pairs():
        with_ws, without, old = BASELINE[("p", a, b, M)]
        assert with_ws == without == old


@pytest.mark.parametrize("S", [1, 2, 3, 8, 16])
def test_fold_model_against_float64(S):
    g = np.random.default_rng(S)
    gw0 = g.standard_normal((37, 52)).astype(np.float32) * 30
    parts = [(g.standard_normal((37, 52)) * 10.0 ** g.integers(-3, 3)).astype(np.float32) for _ in range(S)]
    got = D.fold(gw0, parts)
    assert got.dtype == np.float32
    exact = gw0.astype(np.float64) + sum(p.astype(np.float64) for p in parts)
    assert np.all(np.abs(got.astype(np.float64) - exact) <= D.fold_bound(gw0, parts))
    # the order is part of the definition: ascending, onto the old value -- another order gives other bits somewhere
    if S >= 3:
        assert np.any(D.fold(gw0, parts[::-1]) != got)
    # and it is what the launches' own arithmetic does: one fp32 addition per slice
    acc = gw0.copy()
    for p in parts:
        acc += p
    assert np.array_equal(acc, got)


def test_chunk_sum_model():
    parts = np.float32([1e8, 1.0, -1e8, 3.0])
    assert D.chunk_sum(parts) == np.float32(3.0) and D.chunk_sum(parts[::-1]) == np.float32(0.0)
    assert D.chunk_sum([np.float32(0.1)]) == np.float32(0.1), "one chunk: 0 + p is p, the bits of today's one-chunk tensor"
