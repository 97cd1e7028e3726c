"""GPU tests of octmae_retrieval_pair_ranks (ops.retrieval_pair_ranks, csrc/retrieval_pair.hip): both directions of up to three square
retrieval problems from one walk over the tiles of each product.

Sizes: (N, d) pairs over N in {1, 2, R-1, R, R+1, 2C+3} = {1, 2, 63, 64, 65, 131} and d in {1, 2, 3, K-1, K, K+1, 512, 515} (R = C = 64 rows
and columns per tile, K = 32 k per LDS step), each for P = 1, 2, 3; and (3001, 3) for P = 1 and 3, where a workgroup walks several column
tiles (47 tiles on a split of 22 at P = 1, of 8 at P = 3), a column's count arrives from 47 row blocks and a row's from several
workgroups.

Families.  ``dyadic``: entries in {-2 .. 2} / 4, every product a multiple of 1/16 and every partial sum below 2^10, so the f32 chain is
exact and the expected counts are integer numpy arithmetic (tests/pair_ranks_ref.py) -- every entry of ``out`` EQUAL; ties everywhere.
``against the per-direction kernel``: normalised normal features, a tenth of the rows of every operand bit copies of other rows: ``out``
must equal the stacked ``retrieval_ranks(a, b)[:, :2]`` and ``retrieval_ranks(b, a)[:, :2]``, whose own float64 bounds
tests/test_gpu_retrieval.py holds."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from tests import children
from tests import pair_ranks_ref as PR

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_F16 = os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so")

SIZES = ((1, 1), (2, 2), (63, 3), (64, 31), (65, 32), (131, 33), (64, 512), (131, 515))
BIG = (3001, 3)
DYADIC_CASES = [(n, d, p) for (n, d) in SIZES for p in (1, 2, 3)] + [BIG + (1,), BIG + (3,)]
TRIAD = ((0, 1), (0, 2), (1, 2))          # P = 3: the three products among three shared operands; P < 3: its first P pairs


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=None)
def dyadic_operands(n, d):
    rng = np.random.default_rng([n, d, 11])
    ints = [rng.integers(-2, 3, size=(n, d)) for _ in range(3)]
    return tuple(ints)


@functools.lru_cache(maxsize=None)
def dyadic_want(n, d, p):
    x = dyadic_operands(n, d)
    want = PR.pair_counts([x[i] @ x[j].T for i, j in TRIAD[:p]])             # integer scores, 16 x the f32 ones: exact
    want.setflags(write=False)
    return want


def launch(operands, p):
    from octcubem_amd import ops
    n = operands[0].shape[0]
    got = ops.retrieval_pair_ranks([(operands[i], operands[j]) for i, j in TRIAD[:p]])
    assert got.dtype == torch.int32 and tuple(got.shape) == (p, 2, n, 2) and got.is_contiguous()
    return got.cpu().numpy().astype(np.int64)


def check_dyadic(n, d, p):
    x = [dev((v / 4).astype(np.float32)) for v in dyadic_operands(n, d)]
    got, want = launch(x, p), dyadic_want(n, d, p)
    assert np.array_equal(got, want), f"N={n} d={d} P={p}: {int((got != want).sum())} of {want.size} counts differ"


@pytest.mark.parametrize("n,d,p", DYADIC_CASES)
def test_dyadic_counts_are_equal(n, d, p):
    check_dyadic(n, d, p)


def test_dyadic_cases_have_ties_and_wins_in_both_directions():
    for n, d in ((131, 515), (65, 32), BIG):
        want = dyadic_want(n, d, 3)
        for p in range(3):
            for direction in (0, 1):
                assert (want[p, direction, :, 0] > 0).any() and (want[p, direction, :, 1] > 0).any(), (n, d, p, direction)
        assert not np.array_equal(want[:, 0], want[:, 1])                 # the two directions are different questions
    big = dyadic_want(*BIG, 3)
    assert big[:, 0].max() > 64 and big[:, 1].max() > 64                  # more than one tile's share in a row count and in a column count


def normalize(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def copied_operands(n, d, c):
    """x1, x2 = normalize(c x0 + unit noise); then a tenth of the rows of EACH operand become bit copies of other rows of it"""
    rng = np.random.default_rng([n, d, 12])
    x0 = normalize(rng.standard_normal((n, d)))
    xs = [x0] + [normalize(c * x0 + normalize(rng.standard_normal((n, d)))) for _ in range(2)]
    out = []
    for x in xs:
        x = x.copy()
        copies = rng.choice(n, size=max(n // 10, 2), replace=False)
        src = rng.choice(np.setdiff1d(np.arange(n), copies), size=len(copies))
        x[copies] = x[src]
        out.append(x)
    return tuple(out)


@pytest.mark.parametrize("n,d,c", ((131, 515, 0.15), (3001, 3, 20.0)))
def test_equals_the_per_direction_kernel(n, d, c):
    from octcubem_amd import ops
    x = [dev(v) for v in copied_operands(n, d, c)]
    got = launch(x, 3)
    for p, (i, j) in enumerate(TRIAD):
        rows = ops.retrieval_ranks(x[i], x[j])[:, :2].cpu().numpy()
        cols = ops.retrieval_ranks(x[j], x[i])[:, :2].cpu().numpy()
        assert np.array_equal(got[p, 0], rows) and np.array_equal(got[p, 1], cols), (p, int((got[p, 0] != rows).sum()), int((got[p, 1] != cols).sum()))
        assert (rows[:, 1] > 0).any() and (cols[:, 1] > 0).any()          # the bit copies tie
        for counts in (rows, cols):
            r1 = float((counts.sum(1) < 1).mean())
            print(f"N={n} d={d} pair {p}: R@1 {r1:.3f}")
            assert 0.0 < r1 < 1.0


def test_two_launches_give_the_same_bits():
    x = [dev(v) for v in copied_operands(131, 515, 0.15)]
    assert np.array_equal(launch(x, 3), launch(x, 3))


@pytest.mark.parametrize("n,d", ((65, 33), (131, 515)))
def test_strided_views_of_wider_buffers(n, d):
    ints = dyadic_operands(n, d) if (n, d) in SIZES else None
    rng = np.random.default_rng([n, d, 13])
    if ints is None:
        ints = tuple(rng.integers(-2, 3, size=(n, d)) for _ in range(3))
    want = PR.pair_counts([ints[i] @ ints[j].T for i, j in TRIAD])
    views = []
    for k, v in enumerate(ints):
        wide = (rng.integers(-2, 3, size=(2 * n, d + 5 + k)) / 4).astype(np.float32)
        wide[k % 2::2, 2 + k:2 + k + d] = v / 4
        view = dev(wide)[k % 2::2, 2 + k:2 + k + d]
        assert not view.is_contiguous() and view.stride(0) == 2 * (d + 5 + k)
        views.append(view)
    assert np.array_equal(launch(views, 3), want)


@pytest.mark.parametrize("n,d", ((65, 3), (131, 33)))
def test_equal_rows_tie_by_index(n, d):
    rng = np.random.default_rng([n, d, 14])
    v = dev(np.tile(rng.standard_normal(d).astype(np.float32), (n, 1)))
    got = launch([v, v.clone(), v.clone()], 3)
    assert np.array_equal(got[..., 0], np.zeros((3, 2, n), dtype=np.int64))
    assert np.array_equal(got[..., 1], np.broadcast_to(np.arange(n), (3, 2, n)))


def test_bad_arguments_raise_before_any_launch():
    from octcubem_amd import ops
    a, b, c = (dev((v / 4).astype(np.float32)) for v in dyadic_operands(65, 32))
    seen = []
    prev = ops.KTIMER
    ops.KTIMER = types.SimpleNamespace(launch=lambda kind, flops, nbytes, fn, exec_flops=None: (seen.append(kind), fn()))
    try:
        for bad_value in (float("nan"), float("inf"), float("-inf")):
            bad = a.clone()
            bad[7, 1] = bad_value
            with pytest.raises(ValueError, match="a of pair 0 contains non-finite"):
                ops.retrieval_pair_ranks([(bad, b)])
            with pytest.raises(ValueError, match="b of pair 1 contains non-finite"):
                ops.retrieval_pair_ranks([(a, b), (c, bad)])
        with pytest.raises(TypeError, match="a must be float32"):
            ops.retrieval_pair_ranks([(a.double(), b)])
        with pytest.raises(TypeError, match="b must be float32"):
            ops.retrieval_pair_ranks([(a, b), (a, c.half())])
        with pytest.raises(RuntimeError, match="must be a GPU tensor"):
            ops.retrieval_pair_ranks([(a.cpu(), b)])
        with pytest.raises(RuntimeError, match="must be a GPU tensor"):
            ops.retrieval_pair_ranks([(a, b), (a, c.cpu())])
        with pytest.raises(ValueError, match="every operand must be"):
            ops.retrieval_pair_ranks([(a, b[:64])])                         # unequal N inside a pair
        with pytest.raises(ValueError, match="every operand must be"):
            ops.retrieval_pair_ranks([(a, b), (a[:64], c[:64])])            # ... and between pairs
        with pytest.raises(ValueError, match="expected a"):
            ops.retrieval_pair_ranks([(a, b[:, :31])])                      # unequal D inside a pair
        with pytest.raises(ValueError, match="every operand must be"):
            ops.retrieval_pair_ranks([(a, b), (a[:, :31], c[:, :31])])      # ... and between pairs
        with pytest.raises(ValueError, match="1 .. 3"):
            ops.retrieval_pair_ranks([])
        with pytest.raises(ValueError, match="1 .. 3"):
            ops.retrieval_pair_ranks([(a, b)] * 4)
        with pytest.raises(ValueError, match="unit column stride"):
            ops.retrieval_pair_ranks([(a.t().contiguous().t(), b)])
        with pytest.raises(ValueError, match="empty"):
            ops.retrieval_pair_ranks([(a[:0], b[:0])])
    finally:
        ops.KTIMER = prev
    assert seen == []


def test_the_entry_point_refuses():
    from octcubem_amd import _lib
    lib = _lib.load()
    q = lib.octmae_retrieval_pair_ws
    assert q(4, 1) == 16 and q(3001, 3) == 3 * 3001 * 4
    for n, p in ((0, 1), (-1, 1), (4, 0), (4, 4), (2 ** 31, 1)):
        assert q(n, p) == -1, (n, p)
    a = torch.zeros(4, 8, device=DEV)
    b = torch.zeros(4, 8, device=DEV)
    out = torch.full((2, 2, 4, 2), 7, dtype=torch.int32, device=DEV)
    ws = torch.zeros(64, dtype=torch.uint8, device=DEV)
    A, B, O, W = a.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr()
    fn = lib.octmae_retrieval_pair_ranks
    rest = (None, 0, None, 0)
    for args in ((A, 8, B, 8) + rest + rest + (0, O, W, 64, 4, 8), (A, 8, B, 8) + rest + rest + (4, O, W, 64, 4, 8),
                 (None, 8, B, 8) + rest + rest + (1, O, W, 64, 4, 8), (A, 8, None, 8) + rest + rest + (1, O, W, 64, 4, 8),
                 (A, 8, B, 8) + rest + rest + (1, None, W, 64, 4, 8), (A, 8, B, 8) + rest + rest + (1, O, None, 64, 4, 8),
                 (A, 8, B, 8) + rest + rest + (1, O, W, 15, 4, 8), (A, 8, B, 8) + rest + rest + (1, O, W + 1, 63, 4, 8),
                 (A, 7, B, 8) + rest + rest + (1, O, W, 64, 4, 8), (A, 8, B, 7) + rest + rest + (1, O, W, 64, 4, 8),
                 (A, 8, B, 8) + rest + rest + (1, O, W, 64, 0, 8), (A, 8, B, 8) + rest + rest + (1, O, W, 64, 4, 0),
                 (A, 8, B, 8) + rest + rest + (1, O, W, 64, 2 ** 31, 8),
                 (A, 8, B, 8) + rest + rest + (2, O, W, 64, 4, 8),             # the second pair is missing
                 (A, 8, B, 8, A, 8, B, 7) + rest + (2, O, W, 64, 4, 8), (A, 8, B, 8, A, 8, B, 8) + rest + (2, O, W, 31, 4, 8)):
        assert fn(*args, None) == -1, args
    torch.cuda.synchronize()
    assert int((out != 7).sum()) == 0                                         # nothing written
    assert fn(*((A, 8, B, 8, A, 8, B, 8) + rest + (2, O, W, 32, 4, 8)), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy()[..., 0], np.zeros((2, 2, 4))) and np.array_equal(out.cpu().numpy()[0, 0, :, 1], np.arange(4))


def test_retrieval_pair_ranks_ignore_autocast_and_autograd():
    a, b, c = (dev((v / 4).astype(np.float32)).requires_grad_() for v in dyadic_operands(65, 32))
    with torch.autocast("cuda", dtype=torch.float16):
        got = launch([a, b, c], 3)
    assert np.array_equal(got, dyadic_want(65, 32, 3))


def test_launch_is_accounted_with_its_flops():
    from octcubem_amd import ops
    x = [dev((v / 4).astype(np.float32)) for v in dyadic_operands(65, 32)]
    seen = []
    prev = ops.KTIMER
    ops.KTIMER = types.SimpleNamespace(launch=lambda kind, flops, nbytes, fn, exec_flops=None: (seen.append((kind, flops)), fn()))
    try:
        launch(x, 3)
        launch(x, 1)
        for i, j in TRIAD:
            ops.retrieval_ranks(x[i], x[j])
            ops.retrieval_ranks(x[j], x[i])
    finally:
        ops.KTIMER = prev
    assert seen[:2] == [("retrieval_pair_ranks", 2.0 * 3 * 65 * 65 * 32), ("retrieval_pair_ranks", 2.0 * 65 * 65 * 32)]
    assert sum(f for _, f in seen[2:]) == 2 * seen[0][1]                      # half of what the six per-direction launches account


# ---------------------------------------------------------------------------------------------- the half build
def half_build_cases():
    """What tests/f16_worker.py runs on the half-operand build."""
    for case in DYADIC_CASES:
        check_dyadic(*case)
    return {"passed": [list(c) for c in DYADIC_CASES]}


def start_children():
    """tests/conftest.py calls this once the collection holds a test of this module, before this process has touched the GPU;
    tests/children.py releases the worker when the GPU has room for it."""
    if os.path.exists(LIB_F16):
        children.spawn_f16_worker("pair_ranks_f16", "tests.test_gpu_pair_ranks:half_build_cases")


def test_half_build_runs_the_same_pair_kernel():
    """The entry point has no 16-bit operand: liboctmae_f16.so must give the same counts on every dyadic case."""
    assert os.path.exists(LIB_F16), "make -C octcubem_amd/csrc both"
    start_children()
    res = children.f16_worker_result("pair_ranks_f16")
    assert res["lib"] == "liboctmae_f16.so" and res["lp_is_f16"] is True
    assert res["passed"] == [list(c) for c in DYADIC_CASES], res
