"""GPU tests of the top-k retrieval: octmae_retrieval_topk (ops.retrieval_topk, csrc/retrieval_topk.hip) and coem.retrieve_topk /
retrieval_report / evaluate on top of it.

The kernel walks the tiles of the ranks kernel (64 rows of a per workgroup, 64 columns per tile, 32 k per LDS step) and keeps k <= 32
(score, index) pairs per row; the column tiles of a row block are split over up to 1024 workgroups, whose partial lists a second kernel
merges.  Families.  ``dyadic``: entries in {-2 .. 2} / 4 (a tenth of b's rows doubled, so that later tiles reach the lists), the f32
chain is exact, retrieval_ref.chain_scores IS the kernel's score and indices and score bits must EQUAL the stable descending sort of
tests/retrieval_topk_ref.py -- ties in every row pin the tie rule, keep, the groups and the padding.  ``continuous``: unit-norm rows,
four conditions per element against the float64 score S and the standard bound of an f32 chain of d terms,
e(i, j) = gamma_d sum_k |a_ik b_jk|, gamma_d = d u / (1 - d u), u = 2^-24."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from tests import children
from tests import retrieval_ref as R
from tests import retrieval_topk_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_F16 = os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so")

SHAPES = ((1, 1, 1), (65, 65, 3), (64, 131, 33), (131, 63, 512), (64, 64, 32))
KS = (1, 3, 10, 32)
# keep / groups given or not; "own": only columns of group 0 are kept, so the rows of group 0 have no candidate at all
MODES = ("none", "keep", "groups", "both", "own")
DYADIC_CASES = [(n, m, d, mode) for (n, m, d) in SHAPES for mode in MODES]
TRIP_CASES = [(n, m, d, mode) for (n, m, d) in T.TRIP_SHAPES for mode in ("none", "both")]


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def side_inputs(rng, n, m, mode):
    keep = (rng.random(m) < 0.5).astype(np.uint8)
    keep[m - 1] = 1                                     # the last column of the last (ragged) tile takes part
    rg, cg = rng.integers(0, 4, size=n).astype(np.int32), rng.integers(0, 4, size=m).astype(np.int32)
    if m == 1:
        cg[0] = rg[0]                                   # the one column is of the one row's group
    if mode == "own":
        keep = (cg == 0).astype(np.uint8)
    return (keep if mode in ("keep", "both", "own") else None), *((rg, cg) if mode in ("groups", "both", "own") else (None, None))


@functools.lru_cache(maxsize=None)
def dyadic_scores(n, m, d):
    rng = np.random.default_rng([n, m, d, 1])
    ia, ib = rng.integers(-2, 3, size=(n, d)), rng.integers(-2, 3, size=(m, d))
    # a tenth of the columns, the last one among them, count double: with ties everywhere the lowest columns would fill every list and
    # the later tiles (other workgroups, later trips) would never contribute
    boost = rng.random(m) < 0.1
    boost[m - 1] = True
    ib[boost] *= 2
    a, b = (ia / 4).astype(np.float32), (ib / 4).astype(np.float32)
    s = R.chain_scores(a, b)
    assert np.array_equal(s, (a.astype(np.float64) @ b.astype(np.float64).T).astype(np.float32))      # exact: the chain's own bits
    for x in (a, b, s):
        x.setflags(write=False)
    return a, b, s


@functools.lru_cache(maxsize=None)
def dyadic_case(n, m, d, mode):
    """inputs, and the expected lists at k = 32: the first k of them are the expected lists at k (a prefix, padding included)"""
    a, b, s = dyadic_scores(n, m, d)
    keep, rg, cg = side_inputs(np.random.default_rng([n, m, d, MODES.index(mode), 2]), n, m, mode)
    idx, score = T.topk_from(s, T.K_MAX, keep, rg, cg)
    for x in (idx, score):
        x.setflags(write=False)
    return a, b, keep, rg, cg, idx, score


def launch(a, b, k, keep=None, rg=None, cg=None):
    from octcubem_amd import ops
    idx, score = ops.retrieval_topk(dev(a), dev(b), k, dev(keep), dev(rg), dev(cg))
    assert idx.dtype == torch.int32 and score.dtype == torch.float32 and tuple(idx.shape) == tuple(score.shape) == (a.shape[0], k)
    assert idx.is_contiguous() and score.is_contiguous()
    return idx.cpu().numpy().astype(np.int64), score.cpu().numpy()


def same_bits(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.int32), np.ascontiguousarray(y).view(np.int32))


def check_dyadic(n, m, d, mode, ks=KS):
    a, b, keep, rg, cg, want_idx, want_score = dyadic_case(n, m, d, mode)
    for k in ks:
        idx, score = launch(a, b, k, keep, rg, cg)
        assert np.array_equal(idx, want_idx[:, :k]), \
            f"n={n} m={m} d={d} {mode} k={k}: {int((idx != want_idx[:, :k]).sum())} of {idx.size} indices differ"
        assert same_bits(score, want_score[:, :k]), f"n={n} m={m} d={d} {mode} k={k}: the score bits differ"


@pytest.mark.parametrize("n,m,d,mode", DYADIC_CASES)
def test_dyadic_lists_are_equal(n, m, d, mode):
    check_dyadic(n, m, d, mode)


@pytest.mark.parametrize("n,m,d,mode", TRIP_CASES)
def test_dyadic_lists_past_the_split_and_the_grid_cap(n, m, d, mode):
    """(3, 65600, 2): one row block, split 1024, workgroup 0 walks a second tile and 1024 partial lists are merged; (3001, 3001, 3):
    split 22 of 47 tiles, a 57-column last tile; (65473, 131, 2): split 1, three tiles per workgroup, the lists written directly"""
    assert T.plan(n, m)[1] > T.plan(n, m)[2]
    check_dyadic(n, m, d, mode, ks=(10, 32))


def test_dyadic_cases_have_ties_padding_and_empty_rows():
    _, _, s = dyadic_scores(131, 63, 512)
    assert (np.diff(np.sort(s, axis=1), axis=1) == 0).any(axis=1).all()                       # ties in every row
    _, _, _, _, _, idx, _ = dyadic_case(131, 63, 512, "none")
    assert (idx[:, 31] >= 0).all()
    _, _, keep, rg, cg, idx, _ = dyadic_case(131, 63, 512, "both")
    assert not keep.all() and (idx[:, 31] == -1).any() and (idx[:, 0] >= 0).all()              # padded rows, none empty
    _, _, _, _, _, idx, score = dyadic_case(1, 1, 1, "none")                                   # m < k
    assert idx[0, 0] == 0 and (idx[0, 1:] == -1).all() and np.isneginf(score[0, 1:]).all()
    assert (dyadic_case(1, 1, 1, "groups")[5] == -1).all()                                     # the only column is of the row's group
    for n, m, d in SHAPES[1:]:
        _, _, keep, rg, cg, idx, _ = dyadic_case(n, m, d, "own")
        empty = (idx == -1).all(axis=1)
        assert np.array_equal(empty, rg == 0) and empty.any() and not empty.all()               # all -1 rows beside filled ones
    for n, m, d in T.TRIP_SHAPES:
        _, _, keep, rg, cg, idx, _ = dyadic_case(n, m, d, "both")
        tiles = np.unique(idx[idx >= 0] // 64)
        print(f"n={n} m={m}: the lists draw on {len(tiles)} of {-(-m // 64)} tiles")
        assert len(tiles) >= min(3, -(-m // 64))                                                # the lists draw on several tiles


def normalize(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("n,m,d", ((3001, 3001, 3), (3, 65600, 2)))
def test_ties_across_tiles_and_workgroups_resolve_by_index(n, m, d):
    """Bit copies of one row of b at columns j (first tile), j + 64 (the next workgroup), j + 64 split (the same workgroup's second
    trip) and in the last tile; every other row of b is half as long, so the copies lead the list of every query that points their
    way, with equal scores: the lowest indices win, in ascending order, also where the k-th and the (k+1)-th score are equal."""
    split = T.plan(n, m)[2]
    last = (m - 1) // 64 * 64 + 3
    copies = np.array(sorted({5, 5 + 64, 5 + 64 * split, last}))
    assert len(copies) == 4 and copies[-1] < m and copies[2] // 64 % split == 0 and copies[2] // 64 >= split
    rng = np.random.default_rng([n, m, d, 6])
    a = normalize(rng.standard_normal((n, d)))
    a[0] = normalize(np.ones((1, d)))
    b = (0.5 * normalize(rng.standard_normal((m, d)))).astype(np.float32)
    b[copies] = normalize(np.ones((1, d)))
    lead = a.astype(np.float64) @ b[copies[0]].astype(np.float64) > 0.51            # every other score is at most 0.5 (1 + 2^-20)
    assert lead[0] and lead.sum() >= min(n, 3) // 3
    for k in (1, 3, 4, 10):
        idx, score = launch(a, b, k)
        assert np.array_equal(idx[lead][:, :4], np.tile(copies[:k], (int(lead.sum()), 1))), (k, idx[lead][:3])
        assert (score[lead][:, :min(k, 4)] == score[lead][:, :1]).all()
        if k > 4:
            assert (score[lead][:, 4] < score[lead][:, 0]).all()


@pytest.mark.parametrize("family", ("dyadic", "continuous"))
@pytest.mark.parametrize("with_keep", (False, True))
def test_lists_agree_with_the_ranks_kernel(family, with_keep):
    """p = out[i, 0] + out[i, 1] of ops.retrieval_ranks is the target's place in the same order over the same score bits: the target
    sits at slot p when p < k and is absent otherwise -- exactly, whatever the rounding."""
    from octcubem_amd import ops
    n, m, d, k = 131, 131, 33, 10
    rng = np.random.default_rng([n, m, d, 7, int(with_keep)])
    if family == "dyadic":
        a, b, _ = dyadic_scores(n, m, d)
    else:
        a, b = normalize(rng.standard_normal((n, d))), normalize(rng.standard_normal((m, d)))
    target = rng.integers(0, m, size=n).astype(np.int32)
    keep = None
    if with_keep:
        keep = (rng.random(m) < 0.6).astype(np.uint8)
        keep[target] = 1
    out = ops.retrieval_ranks(dev(a), dev(b), dev(target), dev(keep)).cpu().numpy().astype(np.int64)
    p = out[:, 0] + out[:, 1]
    idx, _ = launch(a, b, k, keep)
    assert (p < k).any() and (p >= k).any()
    for i in range(n):
        if p[i] < k:
            assert idx[i, p[i]] == target[i], (i, p[i], idx[i], target[i])
        else:
            assert target[i] not in idx[i], (i, p[i], idx[i], target[i])


def check_continuous(a, b, k, keep, rg, cg, idx, score):
    n, m, d = a.shape[0], b.shape[0], a.shape[1]
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    S = a64 @ b64.T
    du = d * 2.0 ** -24
    E = du / (1 - du) * (np.abs(a64) @ np.abs(b64).T)
    cand = T.candidates(S, keep, rg, cg)
    filled = idx >= 0
    rows = np.arange(n)[:, None]
    safe = np.where(filled, idx, 0)
    # 3: the filled slots are a prefix of min(k, candidates) distinct candidates
    assert np.array_equal(filled.sum(axis=1), np.minimum(k, cand.sum(axis=1)))
    assert (filled[:, :-1] | ~filled[:, 1:]).all() and np.isneginf(score[~filled]).all()
    assert cand[rows, safe][filled].all()
    returned = np.zeros((n, m), dtype=np.int64)
    np.add.at(returned, (np.broadcast_to(rows, idx.shape)[filled], idx[filled]), 1)
    assert returned.max() <= 1
    # 1: every returned score within e of S
    assert (np.abs(score.astype(np.float64) - S[rows, safe]) <= E[rows, safe])[filled].all()
    # 2: non-increasing, equal scores by ascending index
    both = filled[:, 1:]
    assert (score[:, :-1] >= score[:, 1:])[both].all()
    assert ((score[:, :-1] > score[:, 1:]) | (idx[:, :-1] < idx[:, 1:]))[both].all()
    # 4: no candidate left out could have beaten the last one returned (a row with an open slot has returned every candidate: 3)
    full = filled[:, -1]
    last = safe[:, -1]
    left = cand & (returned == 0) & full[:, None]
    bound = (S[np.arange(n), last] + E[np.arange(n), last])[:, None] + E
    assert (S <= bound)[left].all(), f"{int((S > bound)[left].sum())} candidates left out above the bound"
    return int(left.sum())


@pytest.mark.parametrize("n,m,d", ((131, 131, 33), (65, 131, 515), (3001, 3001, 3)))
@pytest.mark.parametrize("mode", ("none", "both"))
def test_continuous_lists_lie_within_the_f32_bound(n, m, d, mode):
    rng = np.random.default_rng([n, m, d, 4])
    a, b = normalize(rng.standard_normal((n, d))), normalize(rng.standard_normal((m, d)))
    keep, rg, cg = side_inputs(rng, n, m, mode)
    k = 10
    idx, score = launch(a, b, k, keep, rg, cg)
    left = check_continuous(a, b, k, keep, rg, cg, idx, score)
    assert left > 0
    print(f"n={n} m={m} d={d} {mode}: {left} candidates left out, all within the bound")


def test_two_launches_give_the_same_bits():
    rng = np.random.default_rng(9)
    for n, m, d, k in ((65, 131, 515, 32), (3001, 3001, 3, 10)):               # split 2 x 3 and 47 x 22: partial lists and the merge
        assert T.plan(n, m)[2] > 1
        a, b = normalize(rng.standard_normal((n, d))), normalize(rng.standard_normal((m, d)))
        b[m // 2:] = b[:m - m // 2]                                             # ... with ties between workgroups
        i1, s1 = launch(a, b, k)
        i2, s2 = launch(a, b, k)
        assert np.array_equal(i1, i2) and same_bits(s1, s2)


@pytest.mark.parametrize("n,m,d", ((65, 131, 33), (131, 65, 515)))
def test_strided_views_of_wider_buffers(n, m, d):
    from octcubem_amd import ops
    rng = np.random.default_rng([n, m, d, 5])
    a, b = (rng.integers(-2, 3, size=(n, d)) / 4).astype(np.float32), (rng.integers(-2, 3, size=(m, d)) / 4).astype(np.float32)
    keep, rg, cg = side_inputs(rng, n, m, "both")
    want_idx, want_score = T.topk_from(R.chain_scores(a, b), 10, keep, rg, cg)
    wa = (rng.integers(-2, 3, size=(2 * n, d + 5)) / 4).astype(np.float32)
    wb = (rng.integers(-2, 3, size=(m, d + 3)) / 4).astype(np.float32)
    wa[::2, 3:3 + d] = a
    wb[:, 1:1 + d] = b
    va, vb = dev(wa)[::2, 3:3 + d], dev(wb)[:, 1:1 + d]
    assert not va.is_contiguous() and va.stride(0) == 2 * (d + 5) and vb.stride(0) == d + 3
    idx, score = ops.retrieval_topk(va, vb, 10, dev(keep).bool(), dev(rg), dev(cg))
    assert np.array_equal(idx.cpu().numpy(), want_idx) and same_bits(score.cpu().numpy(), want_score)


def test_retrieval_topk_ignores_autocast():
    from octcubem_amd import ops
    a, b, keep, rg, cg, want_idx, want_score = dyadic_case(65, 65, 3, "both")
    with torch.autocast("cuda", dtype=torch.float16):
        idx, score = ops.retrieval_topk(dev(a), dev(b), 10, dev(keep), dev(rg), dev(cg))
    assert idx.dtype == torch.int32 and score.dtype == torch.float32
    assert np.array_equal(idx.cpu().numpy(), want_idx[:, :10]) and same_bits(score.cpu().numpy(), want_score[:, :10])


def test_launch_is_accounted_with_its_flops():
    from octcubem_amd import ops
    a, b, _ = dyadic_scores(65, 65, 3)
    seen = []
    prev = ops.KTIMER
    ops.KTIMER = types.SimpleNamespace(launch=lambda kind, flops, nbytes, fn, exec_flops=None: (seen.append((kind, flops)), fn()))
    try:
        ops.retrieval_topk(dev(a), dev(b), 3)
    finally:
        ops.KTIMER = prev
    assert seen == [("retrieval_topk", 2.0 * 65 * 65 * 3)]


def test_bad_arguments_raise_before_any_launch():
    from octcubem_amd import ops
    a, b, keep, rg, cg, _, _ = dyadic_case(64, 64, 32, "both")
    da, db, dk, drg, dcg = dev(a), dev(b), dev(keep), dev(rg), dev(cg)
    seen = []
    prev = ops.KTIMER
    ops.KTIMER = types.SimpleNamespace(launch=lambda kind, flops, nbytes, fn, exec_flops=None: (seen.append(kind), fn()))
    try:
        for bad_value in (float("nan"), float("inf"), float("-inf")):
            bad = da.clone()
            bad[7, 1] = bad_value
            with pytest.raises(ValueError, match="a contains non-finite"):
                ops.retrieval_topk(bad, db, 3)
            with pytest.raises(ValueError, match="b contains non-finite"):
                ops.retrieval_topk(da, bad, 3)
        for k in (0, 33, -1, 2.0, True, None):
            with pytest.raises(ValueError, match="k must be"):
                ops.retrieval_topk(da, db, k)
        with pytest.raises(TypeError, match="a must be float32"):
            ops.retrieval_topk(da.double(), db, 3)
        with pytest.raises(TypeError, match="b must be float32"):
            ops.retrieval_topk(da, db.half(), 3)
        with pytest.raises(TypeError, match="row_group must be int32"):
            ops.retrieval_topk(da, db, 3, row_group=drg.long(), col_group=dcg)
        with pytest.raises(TypeError, match="keep must be bool or uint8"):
            ops.retrieval_topk(da, db, 3, dk.int())
        with pytest.raises(RuntimeError, match="a must be a GPU tensor"):
            ops.retrieval_topk(torch.from_numpy(a), db, 3)
        with pytest.raises(RuntimeError, match="keep must be a GPU tensor"):
            ops.retrieval_topk(da, db, 3, torch.from_numpy(keep))
        with pytest.raises(ValueError, match="together"):
            ops.retrieval_topk(da, db, 3, row_group=drg)
        with pytest.raises(ValueError, match="together"):
            ops.retrieval_topk(da, db, 3, col_group=dcg)
        with pytest.raises(ValueError, match="unit column stride"):
            ops.retrieval_topk(da.t().contiguous().t(), db, 3)
        with pytest.raises(ValueError, match="unit column stride"):
            ops.retrieval_topk(da, db.repeat(2, 2)[::2, ::2], 3)
        with pytest.raises(ValueError, match="expected a"):
            ops.retrieval_topk(da, db[:, :31], 3)
        with pytest.raises(ValueError, match="expected a"):
            ops.retrieval_topk(da[0], db, 3)
        with pytest.raises(ValueError, match="empty"):
            ops.retrieval_topk(da[:0], db, 3)
        with pytest.raises(ValueError, match=r"col_group must be \[64\]"):
            ops.retrieval_topk(da, db, 3, row_group=drg, col_group=dcg[:63])
        with pytest.raises(ValueError, match=r"keep must be \[64\]"):
            ops.retrieval_topk(da, db, 3, dk[:10])
    finally:
        ops.KTIMER = prev
    assert seen == []


def test_the_entry_point_refuses():
    from octcubem_amd import _lib
    lib = _lib.load()
    fn = lib.octmae_retrieval_topk
    n, m, d, k = 4, 130, 8, 3                                                  # one row block, three column tiles: split 3
    need = lib.octmae_retrieval_topk_ws(n, m, k)
    assert need == T.ws_bytes(n, m, k) == 3 * 4 * 3 * 8
    a, b = torch.zeros(n, d, device=DEV), torch.zeros(m, d, device=DEV)
    oi = torch.full((n, k), 77, dtype=torch.int32, device=DEV)
    osc = torch.full((n, k), 77.0, device=DEV)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    g4, g130 = torch.zeros(n, dtype=torch.int32, device=DEV), torch.ones(m, dtype=torch.int32, device=DEV)
    A, B, OI, OS, WS = a.data_ptr(), b.data_ptr(), oi.data_ptr(), osc.data_ptr(), ws.data_ptr()
    good = dict(a=A, sa=d, b=B, sb=d, keep=None, rg=None, cg=None, k=k, oi=OI, os=OS, ws=WS, wsb=need, n=n, m=m, d=d)
    for change in (dict(a=None), dict(b=None), dict(oi=None), dict(os=None), dict(n=0), dict(m=0), dict(d=0), dict(sa=d - 1), dict(sb=d - 1),
                   dict(k=0), dict(k=33), dict(m=2 ** 31), dict(n=64 * 2 ** 31 + 1), dict(rg=g4.data_ptr()), dict(cg=g130.data_ptr()),
                   dict(wsb=need - 1), dict(ws=None), dict(wsb=0)):
        assert fn(*{**good, **change}.values(), None) == -2, change
    torch.cuda.synchronize()
    assert int((oi != 77).sum()) == 0 and int((osc != 77.0).sum()) == 0          # nothing was written
    assert lib.octmae_retrieval_topk_ws(64, 64, 32) == 0                         # no split: no workspace, ws may be NULL
    o2i, o2s = torch.full((64, 32), 77, dtype=torch.int32, device=DEV), torch.full((64, 32), 77.0, device=DEV)
    a2 = torch.zeros(64, d, device=DEV)
    assert fn(a2.data_ptr(), d, a2.data_ptr(), d, None, None, None, 32, o2i.data_ptr(), o2s.data_ptr(), None, 0, 64, 64, d, None) == 0
    assert fn(*good.values(), None) == 0
    assert fn(*{**good, "rg": g4.data_ptr(), "cg": g130.data_ptr()}.values(), None) == 0
    torch.cuda.synchronize()
    assert oi.tolist() == [[0, 1, 2]] * n and osc.tolist() == [[0.0] * k] * n    # all scores tie at 0: the lowest columns
    assert o2i.tolist() == [list(range(32))] * 64


# ---------------------------------------------------------------------------------------------- end to end
BATCHES = (5, 5, 3)
K_EVAL = 3


class DyadicTowers(torch.nn.Module):
    """a CLIP pair whose features are the first eight voxels / pixels of its inputs: dyadic inputs give dyadic features"""

    def __init__(self):
        super().__init__()
        self.logit_scale = torch.nn.Parameter(torch.tensor(np.log(4.0), dtype=torch.float32))

    def forward(self, vol, img):
        return vol.flatten(1)[:, :8].float(), img.flatten(1)[:, :8].float(), self.logit_scale.exp()


def val_loader():
    rng = np.random.default_rng(8)
    n = sum(BATCHES)
    vol = torch.from_numpy((rng.integers(-2, 3, size=(n, 1, 2, 4, 4)) / 4).astype(np.float32))
    ir = torch.from_numpy((rng.integers(-2, 3, size=(n, 3, 4, 4)) / 4).astype(np.float32))
    out, i = [], 0
    for bsz in BATCHES:
        out.append((vol[i:i + bsz], ir[i:i + bsz]))
        i += bsz
    return out, vol.flatten(1)[:, :8].numpy(), ir.flatten(1)[:, :8].numpy()


def test_evaluate_saves_the_lists_and_the_report_reads_them(tmp_path):
    from octcubem_amd import coem
    model = DyadicTowers().to(DEV)
    loader, fi, ft = val_loader()
    n = sum(BATCHES)
    data = {"val": types.SimpleNamespace(dataloader=loader)}
    args = types.SimpleNamespace(device=DEV, val_frequency=1, epochs=4, save_logs=True, checkpoint_path=str(tmp_path),
                                 save_retrieval_results=True, multimodal_type="default", return_metainfo=False, correct_label=0,
                                 retrieval_topk=K_EVAL)
    got = coem.evaluate(model, data, 2, args)
    assert got["num_samples"] == n
    path = os.path.join(str(tmp_path), "retrieval_results_2.npz")
    z = np.load(path)
    assert set(z.files) == {"image_features", "text_features", "logit_scale", "topk_image_to_text", "topk_text_to_image",
                            "topk_image_to_text_scores", "topk_text_to_image_scores"}
    assert np.array_equal(z["image_features"], fi) and np.array_equal(z["text_features"], ft)
    s = R.chain_scores(fi, ft)
    for name, mat in (("topk_image_to_text", s), ("topk_text_to_image", s.T)):
        want_idx, want_score = T.topk_from(mat, K_EVAL)
        assert z[name].dtype == np.int32 and z[name].shape == (n, K_EVAL) and np.array_equal(z[name], want_idx)
        assert z[name + "_scores"].dtype == np.float32 and same_bits(z[name + "_scores"], want_score)
    # without the argument, or with 0: the file of before
    for k in (0, None):
        args.retrieval_topk = k
        coem.evaluate(model, data, 3, args)
        assert set(np.load(os.path.join(str(tmp_path), "retrieval_results_3.npz")).files) == {"image_features", "text_features", "logit_scale"}
    # the report off the file, on the kernel and through the numpy restatement
    patients = [f"pat-{i // 3}" for i in range(n)]
    side = [int(i % 2) for i in range(n)]
    for ir_oct in (False, True):
        rep = coem.retrieval_report(path, side, patients, os.path.join(str(tmp_path), "gpu"), "tiny", topk_list=(1, 3, 5), ir_oct=ir_oct)
        ref = coem.retrieval_report(path, side, patients, os.path.join(str(tmp_path), "ref"), "tiny", topk_list=(1, 3, 5), ir_oct=ir_oct,
                                    topk=T.topk_fn(R.f64_scores))
        assert rep["accuracy"] == ref["accuracy"] and np.array_equal(rep["indices"], ref["indices"])
        assert same_bits(rep["scores"], ref["scores"])
        name = "tiny_laterality_ir.csv" if ir_oct else "tiny_laterality.csv"
        assert open(os.path.join(str(tmp_path), "gpu", name)).read() == open(os.path.join(str(tmp_path), "ref", name)).read()
        for i in range(n):
            assert all(patients[j] != patients[i] for j in rep["indices"][i])
    # retrieve_topk on device tensors with string groups
    idx, score = coem.retrieve_topk(dev(fi), dev(ft), 5, query_groups=patients, gallery_groups=patients)
    gid = np.array([i // 3 for i in range(n)])
    want_idx, want_score = T.topk_from(s, 5, None, gid, gid)
    assert idx.dtype == np.int64 and np.array_equal(idx, want_idx) and same_bits(score, want_score)


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
        children.spawn_f16_worker("retrieval_topk_f16", "tests.test_gpu_retrieval_topk:half_build_cases", limit_s=240)


def test_half_build_runs_the_same_topk_kernel():
    """The entry point has no 16-bit operand: liboctmae_f16.so must give the same lists on every dyadic case.  The child was started
    before this process touched the GPU; it is released here and then runs under its own time limit."""
    assert os.path.exists(LIB_F16), "make -C octcubem_amd/csrc both"
    start_children()
    res = children.f16_worker_result("retrieval_topk_f16")
    assert res["lib"] == "liboctmae_f16.so" and res["lp_is_f16"] is True
    assert res["passed"] == [list(c) for c in DYADIC_CASES], res
