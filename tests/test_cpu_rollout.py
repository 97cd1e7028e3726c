"""CPU tests of the attention-rollout step: the f32 restatement of csrc/rollout.hip inside the bounds tests/rollout_ref.py derives and
five planted faults outside them, the vector chain against the published matrix product, mass conservation, the restated launch plan
against the kernel's constants, the ABI of the two entry points and every refusal of theirs (they return before any launch)."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import rollout_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("octmae_rollout_ws", "octmae_rollout_step")


@functools.lru_cache(maxsize=None)
def problem(shape):
    B, N, H, HD = shape
    q, k, scale = R.make_problem(B, N, H, HD, seed=5)
    return R.chain_scores(q, k, B, N, H, HD), scale


def _round_f32(exact):
    """the f32 nearest to a Fraction, ties to even"""
    from fractions import Fraction
    lo = np.float32(float(exact))
    cands = {lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))}
    return min(cands, key=lambda c: (abs(Fraction(float(c)) - exact), int(c.view(np.uint32)) & 1))


def test_chain_scores_are_the_fused_chain():
    """the restated score is ONE rounding per k -- the exact a b + acc in rational arithmetic, rounded once -- also where float64
    would round twice"""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    q = rng.standard_normal((5, 7)).astype(np.float32)
    k = rng.standard_normal((5, 7)).astype(np.float32)
    s = R.chain_scores(q, k, 1, 5, 1, 7)[0, 0]
    for i in range(5):
        for j in range(5):
            acc = np.float32(0)
            for kk in range(7):
                acc = _round_f32(Fraction(float(q[i, kk])) * Fraction(float(k[j, kk])) + Fraction(float(acc)))
            assert acc == s[i, j], (i, j)
    # acc + a b = 2^30 + 192 - 2^-34: float64 rounds it onto the midpoint of two f32 numbers, and the tie would then go UP to the even one
    a, b, acc = np.float32(8 * (1 + 2.0 ** -20)), np.float32(8 * (1 - 2.0 ** -20)), np.float32(2.0 ** 30 + 128)
    assert np.float32(np.float64(acc) + np.float64(a) * np.float64(b)) == np.float32(2.0 ** 30 + 256)
    got = R._fma32(np.array([np.float64(a)]), np.array([np.float64(b)]), np.array([acc]))[0]
    assert got == acc == _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(acc)))


@pytest.mark.parametrize("fusion", R.FUSIONS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_f32_restatement_is_inside_the_bounds(shape, fusion):
    B, N, H, HD = shape
    s, scale = problem(shape)
    assert float(np.abs(float(scale) * s.astype(np.float64)).max()) > 79.0 or N == 1      # hot rows: |z| reaches 80
    assert N < 3 or float(np.abs(float(scale) * s.astype(np.float64)).max(axis=3).min()) < 1.0   # cold rows: |z| stays below 1
    refs = [R.StepRef(s[b], scale, fusion) for b in range(B)]
    for start in R.STARTS:
        r = R.make_start(start, B, N)
        got = R.emulate(s, scale, r, fusion)
        for b in range(B):
            ref = refs[b].apply(r[b])
            w = R.worst(got[b], ref)
            print(shape, fusion, start, "worst |err| / bound =", w)
            assert w < 1.0, (start, b, w)
            # mass is kept: the rows of Ahat sum to 1
            mass_bound = float(ref[1].sum())
            assert abs(float(ref[0].sum()) - float(r[b].astype(np.float64).sum())) <= 1e-12 * max(1.0, float(r[b].sum()))
            assert abs(float(got[b].astype(np.float64).sum()) - float(r[b].astype(np.float64).sum())) <= mass_bound


@pytest.mark.parametrize("fusion", R.FUSIONS)
@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_faults_leave_the_bounds(fault, fusion):
    shape = (1, 130, 3, 32)
    s, scale = problem(shape)
    r = R.make_start("random", 1, 130)
    ref = R.step_reference(s, scale, r, fusion)
    assert R.worst(R.emulate(s, scale, r, fusion), ref) < 1.0
    w = R.worst(R.emulate(s, scale, r, fusion, fault), ref)
    print(fault, fusion, "worst |err| / bound =", w)
    if fault == "rho2" and fusion == "mean":
        assert w < 1.0          # rho IS 2 under mean fusion: not a fault there
    else:
        assert w > 1.0, w


@pytest.mark.parametrize("first_layer", [0, 1])
@pytest.mark.parametrize("fusion", R.FUSIONS)
def test_vector_chain_equals_the_start_row_of_the_published_product(fusion, first_layer):
    B, N, H, HD, L = 2, 37, 3, 16, 4
    scores, scales, attn = [], [], []
    for layer in range(L):
        q, k, scale = R.make_problem(B, N, H, HD, seed=20 + layer)
        s = R.chain_scores(q, k, B, N, H, HD)
        scores.append(s)
        scales.append(scale)
        attn.append(torch.softmax(float(scale) * torch.from_numpy(s).double(), dim=-1))
    # the published algorithm, literally: per layer fuse the heads, add eye, normalise the rows, multiply in layer order
    eye = torch.eye(N, dtype=torch.float64)
    Rm = eye.expand(B, N, N).clone()
    for A in attn[first_layer:]:
        Fu = A.mean(dim=1) if fusion == "mean" else (A.max(dim=1).values if fusion == "max" else A.min(dim=1).values)
        a = Fu + eye
        a = a / a.sum(dim=-1, keepdim=True)
        Rm = a @ Rm
    assert torch.equal(Rm, R.published_rollout(attn, fusion, first_layer))
    for w in (R.make_start("cls", B, N), R.make_start("patches", B, N), R.make_start("zeros", B, N, seed=4)):
        w64 = torch.from_numpy(w).double()
        want = torch.einsum("bi,bij->bj", w64, Rm)
        got, bound = R.chain_reference(scores, scales, w, fusion, first_layer)
        assert float((got - want).abs().max()) <= 1e-12
        assert float((got.sum(dim=1) - w64.sum(dim=1)).abs().max()) <= 1e-12
        assert bool((bound > 0).all()) and float(bound.max()) < 1e-3
        # the f32 restatement run as a chain stays inside the propagated bound
        r = w
        for layer in range(L - 1, first_layer - 1, -1):
            r = R.emulate(scores[layer], scales[layer], r, fusion)
        assert R.worst(r, (got, bound)) < 1.0


def hip_constant(text, name):
    return int(re.search(rf"^constexpr int {name} = (\d+);", text, re.M).group(1))


def test_restated_plan_follows_the_kernel_constants():
    """Whoever changes a constant of the tile or of csrc/rollout.hip is told here to move R.SHAPES (tests/test_gpu_rollout.py)."""
    src = open(os.path.join(ROOT, "octcubem_amd", "csrc", "rollout.hip")).read()
    tile = open(os.path.join(ROOT, "octcubem_amd", "csrc", "simtile.hpp")).read()
    assert '#include "simtile.hpp"' in src
    assert hip_constant(tile, "SIM_TARGET_WGS") == R.TARGET_WGS and hip_constant(src, "RO_MAX_SPLIT") == R.MAX_SPLIT
    assert hip_constant(tile, "SIM_ROWS") == hip_constant(tile, "SIM_COLS") == R.TILE and hip_constant(src, "RO_MAX_HD") == R.MAX_HD
    assert re.search(r"p->split = \(int\)sim_split\(p->blocks, p->blocks, RO_MAX_SPLIT\);", src)
    assert not re.search(r"atomic", src.split("#include", 1)[1])          # no atomics in the code, float or integer
    assert tuple(R.split(shape[1]) for shape in R.SHAPES) == R.SPLITS
    N = R.TRIP_SHAPE[1]
    tiles = -(-N // R.TILE)
    assert R.split(N) < tiles and R.split(N - R.TILE) == tiles - 1            # the smallest N with a second trip
    assert [len(R.walked_tiles(tiles, R.split(N), y)) for y in range(R.split(N))] == [2] + [1] * 31
    assert R.split(5121) == 13 and R.split(64 * 1024) == 1 and R.split(64 * 16) == 16


def test_abi_declares_the_rollout_entry_points():
    from octcubem_amd import _lib
    header = open(os.path.join(ROOT, "include", "octmae.h")).read()
    assert re.search(r"^int octmae_rollout_ws\(int B, long long N, int H, int fusion\);", header, re.M)
    assert re.search(r"^int octmae_rollout_step\(", header, re.M)
    assert re.search(r"^ \*     Added under 35 .*octmae_rollout_step \(\+ octmae_rollout_ws\)", header, re.M)     # the version list
    for sym in SYMBOLS:
        assert sym in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["octmae_rollout_ws"]) == 4 and len(_lib.SIGNATURES["octmae_rollout_step"]) == 15
    assert not set(SYMBOLS) & set(_lib.RESTYPES)                     # both return int: a byte count below 2^31, a status
    lib = _lib.load()
    assert lib.octmae_abi_version() == _lib.expected_abi_version() == _lib.CONSTANTS["OCTMAE_ABI_VERSION"]
    mk = open(os.path.join(ROOT, "octcubem_amd", "csrc", "Makefile")).read()
    assert "rollout.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    for name in ("liboctmae.so", "liboctmae_f16.so"):
        path = os.path.join(ROOT, "octcubem_amd", name)
        assert os.path.exists(path), f"{path}: __graft_entry__.build() makes both libraries"
        names = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for sym in SYMBOLS:
            assert re.search(rf"\bT {sym}$", names, re.M), (name, sym)


def test_workspace_query():
    from octcubem_amd import _lib
    ws = _lib.load().octmae_rollout_ws
    for bad in ((0, 5, 1, 0), (1, 0, 1, 0), (1, 5, 0, 0), (-1, 5, 1, 0), (1, -5, 1, 0), (1, 5, -1, 0), (1, 5, 1, -1), (1, 5, 1, 3),
                (1, 2 ** 31, 1, 0), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 0), (1, 2 ** 31 - 1, 64, 0)):
        assert ws(*bad) == -2, bad
    assert ws(1, 2 ** 25, 15, 0) == 4 * 15 * 2 ** 25 and ws(1, 2 ** 25, 16, 0) == -2     # the byte count is an int: 2^31 bytes are refused
    for B, N, H in ((1, 1, 1), (1, 64, 3), (2, 65, 2), (3, 197, 12), (1, 2049, 1), (4, 5121, 16), (1, 70000, 2)):
        for fusion in range(3):
            assert ws(B, N, H, fusion) == R.ws_bytes(B, N, H, fusion), (B, N, H, fusion)
    # lse [B][H][N]: linear in each; rho [B][N] for max / min only; the slabs only past one block
    assert ws(1, 64, 1, 0) == 4 * 64 and ws(1, 64, 1, 1) == ws(1, 64, 1, 2) == 8 * 64
    assert ws(2, 64, 5, 0) == 2 * 5 * ws(1, 64, 1, 0) and ws(1, 65, 1, 0) == 4 * 65 * (1 + 2)
    assert ws(1, 5121, 16, 0) == 4 * 5121 * (16 + 13) and ws(1, 5121, 16, 1) == 4 * 5121 * (16 + 1 + 13)
    assert ws(3, 5121, 16, 0) == 3 * ws(1, 5121, 16, 0) < ws(3, 5122, 16, 0) < ws(3, 5122, 17, 0)


# every refusal of octmae_rollout_step happens before any launch: the pointers below are never followed
Q, K, RI, RO_, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
GOOD = dict(q=Q, q_stride=128, k=K, k_stride=128, B=2, N=65, H=2, HD=64, scale=0.125, fusion=1, r_in=RI, r_out=RO_, ws=WS,
            ws_bytes=R.ws_bytes(2, 65, 2, 1), stream=None)
REFUSALS = {
    "null q": dict(q=None), "null k": dict(k=None), "null r_in": dict(r_in=None), "null r_out": dict(r_out=None), "null ws": dict(ws=None),
    "B 0": dict(B=0), "B negative": dict(B=-2), "N 0": dict(N=0), "N negative": dict(N=-65), "H 0": dict(H=0), "H negative": dict(H=-2),
    "HD 0": dict(HD=0), "HD 129": dict(HD=129, q_stride=4096, k_stride=4096), "HD negative": dict(HD=-64),
    "q stride short": dict(q_stride=127), "k stride short": dict(k_stride=127), "fusion -1": dict(fusion=-1), "fusion 3": dict(fusion=3),
    "N 2^31": dict(N=2 ** 31, ws_bytes=2 ** 62), "in place": dict(r_out=RI), "ws short": dict(ws_bytes=R.ws_bytes(2, 65, 2, 1) - 1),
    "ws sized for mean": dict(ws_bytes=R.ws_bytes(2, 65, 2, 0)),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_entry_point_refuses_before_any_launch(case):
    from octcubem_amd import _lib
    args = dict(GOOD, **REFUSALS[case])
    assert R.ws_bytes(2, 65, 2, 1) > R.ws_bytes(2, 65, 2, 0) and GOOD["q_stride"] == GOOD["H"] * GOOD["HD"]
    rc = _lib.load().octmae_rollout_step(*(args[name] for name in GOOD))
    assert rc == -2, (case, rc)


def test_capture_attention_is_off_by_default_and_nests():
    from octcubem_amd import ops
    assert ops._ATTN_CAPTURE is None
    with ops.capture_attention() as outer:
        assert ops._ATTN_CAPTURE is outer == []
        with ops.capture_attention() as inner:
            assert ops._ATTN_CAPTURE is inner and inner is not outer
        assert ops._ATTN_CAPTURE is outer
    assert ops._ATTN_CAPTURE is None
    with pytest.raises(ZeroDivisionError):
        with ops.capture_attention():
            1 / 0
    assert ops._ATTN_CAPTURE is None
