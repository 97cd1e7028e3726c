"""CPU tests of the top-k retrieval: the numpy restatement (tests/retrieval_topk_ref.py) against a brute-force loop, the restated
launch plan against the constants of csrc/retrieval_topk.hip, and the host side of octcubem_amd/coem.py (retrieve_topk,
topk_match_accuracy, retrieval_report) fed through ``topk=``.  Accuracy values: float64 quotients of integers, compared within 1e-12."""
import csv
import os
import re

import numpy as np
import pytest
import torch

from tests import retrieval_ref as R
from tests import retrieval_topk_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_force(s, k, keep, rg, cg):
    """pick the best remaining candidate k times, by the contract's order, with python comparisons"""
    n, m = s.shape
    idx = np.full((n, k), -1, dtype=np.int64)
    score = np.full((n, k), -np.inf, dtype=s.dtype)
    for i in range(n):
        left = [j for j in range(m) if (keep is None or keep[j]) and (rg is None or cg[j] != rg[i]) and not np.isnan(s[i, j])]
        for p in range(k):
            if not left:
                break
            best = left[0]
            for j in left[1:]:
                if s[i, j] > s[i, best] or (s[i, j] == s[i, best] and j < best):
                    best = j
            left.remove(best)
            idx[i, p], score[i, p] = best, s[i, best]
    return idx, score


@pytest.mark.parametrize("n,m,k,sides", ((7, 9, 3, 0), (7, 9, 10, 3), (5, 23, 5, 1), (5, 23, 32, 2), (1, 1, 1, 0), (6, 4, 4, 3)))
def test_reference_equals_a_brute_force_loop_with_ties(n, m, k, sides):
    rng = np.random.default_rng([n, m, k, sides])
    s = rng.integers(-2, 3, size=(n, m)).astype(np.float32)          # ties in every row
    s[rng.random((n, m)) < 0.1] = np.nan
    s[rng.random((n, m)) < 0.1] = -np.inf
    s[rng.random((n, m)) < 0.05] = np.inf
    s[s == 0] = np.where(rng.random(int((s == 0).sum())) < 0.5, -0.0, 0.0)     # -0.0 ties with 0.0
    keep = (rng.random(m) < 0.7).astype(np.uint8) if sides & 1 else None
    rg, cg = (rng.integers(0, 3, size=n), rng.integers(0, 3, size=m)) if sides & 2 else (None, None)
    idx, score = T.topk_from(s, k, keep, rg, cg)
    want_idx, want_score = brute_force(s, k, keep, rg, cg)
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(score.view(np.int32), want_score.view(np.int32))          # the bits: -0.0 stays -0.0
    assert (score[idx == -1] == -np.inf).all()                                       # padding is -1 / -inf


def test_all_rows_padded_when_nothing_is_a_candidate():
    s = np.arange(12, dtype=np.float32).reshape(3, 4)
    idx, score = T.topk_from(s, 2, keep=np.zeros(4, dtype=np.uint8))
    assert (idx == -1).all() and np.isneginf(score).all()
    idx, _ = T.topk_from(s, 2, row_group=np.zeros(3, dtype=np.int32), col_group=np.array([0, 0, 1, 0], dtype=np.int32))
    assert np.array_equal(idx, np.array([[2, -1]] * 3))


def test_restated_plan_follows_the_kernel_constants_and_the_workspace_follows_the_plan():
    """Whoever changes a constant of the tile (csrc/simtile.hpp) or of csrc/retrieval_topk.hip is told here to move the shapes of
    tests/test_gpu_retrieval_topk.py."""
    src = open(os.path.join(ROOT, "octcubem_amd", "csrc", "retrieval_topk.hip")).read()
    tile = open(os.path.join(ROOT, "octcubem_amd", "csrc", "simtile.hpp")).read()
    const = lambda name, text=tile: int(re.search(rf"^constexpr int {name} = (\d+);", text, re.M).group(1))
    assert '#include "simtile.hpp"' in src and not re.search(r"^constexpr int RT_(ROWS|COLS|K|TARGET_WGS) ", src, re.M)
    assert const("SIM_ROWS") == const("SIM_COLS") == T.TILE and const("SIM_TARGET_WGS") == T.TARGET_WGS
    assert const("RT_KMAX", src) == T.K_MAX
    # sim_split as written: ceil(target / row_blocks), then the two caps; this file's cap is the grid's y
    assert re.search(r"long long split = \(SIM_TARGET_WGS \+ row_blocks - 1\) / row_blocks;\s*if \(split > col_tiles\) split = col_tiles;\s*"
                     r"if \(split > cap\) split = cap;", tile)
    assert re.search(rf"return sim_split\(\(n \+ SIM_ROWS - 1\) / SIM_ROWS, \(m \+ SIM_COLS - 1\) / SIM_COLS, {T.MAX_GRID_Y}\);", src)
    assert re.search(r"static_assert\(sizeof\(RtPair\) == 8,", src) and T.PAIR_BYTES == 8
    assert re.search(r"return split > 1 \? split \* n \* k \* \(long long\)sizeof\(RtPair\) : 0;", src)
    # the same walk as the ranks kernel: its trip shapes are past this split too
    assert (T.TILE, T.TARGET_WGS, T.MAX_GRID_Y) == (R.TILE, R.TARGET_WGS, R.MAX_GRID_Y) and T.TRIP_PLANS == R.TRIP_PLANS
    for (n, m, d), want in zip(T.TRIP_SHAPES, T.TRIP_PLANS):
        assert T.plan(n, m) == want and want[1] > want[2]
    assert T.plan(1, 1) == (1, 1, 1) and T.plan(131, 131) == (3, 3, 3) and T.plan(64, 70000) == (1, 1094, 1024)
    assert T.ws_bytes(1, 1, 32) == 0 and T.ws_bytes(64, 64, 32) == 0                       # one tile: no split
    assert T.ws_bytes(65, 65, 3) == 2 * 65 * 3 * 8 and T.ws_bytes(131, 63, 10) == 0
    assert T.ws_bytes(3, 65600, 32) == 1024 * 3 * 32 * 8 and T.ws_bytes(3001, 3001, 10) == 22 * 3001 * 10 * 8
    assert T.ws_bytes(65473, 131, 32) == 0                                                  # 1024 row blocks: split 1
    from octcubem_amd import ops
    assert ops.RETRIEVAL_TOPK_MAX == T.K_MAX


def test_library_workspace_query_equals_the_plan():
    from octcubem_amd import _lib
    fn = _lib.load().octmae_retrieval_topk_ws
    for n, m, k in ((1, 1, 1), (65, 65, 3), (64, 131, 32), (131, 63, 10), (3, 65600, 32), (3001, 3001, 10), (65473, 131, 32),
                    (63, 2 ** 31 - 1, 32)):
        assert fn(n, m, k) == T.ws_bytes(n, m, k), (n, m, k)
    for bad in ((0, 5, 1), (5, 0, 1), (5, 5, 0), (5, 5, 33), (5, 2 ** 31, 1)):
        assert fn(*bad) == -2, bad


def test_abi_declares_both_symbols():
    from octcubem_amd import _lib
    header = open(os.path.join(ROOT, "include", "octmae.h")).read()
    for name in ("octmae_retrieval_topk", "octmae_retrieval_topk_ws"):
        decl = re.search(rf"^(?:long long )?int {name}\(([^;]*)\);", header, re.M | re.S)
        assert decl, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == decl.group(1).count(",") + 1, name
    assert len(_lib.SIGNATURES["octmae_retrieval_topk"]) == 16 and len(_lib.SIGNATURES["octmae_retrieval_topk_ws"]) == 3
    assert _lib.expected_abi_version() >= 29 and re.search(r"^ \* 29: octmae_retrieval_topk", header, re.M)
    mk = open(os.path.join(ROOT, "octcubem_amd", "csrc", "Makefile")).read()
    assert "retrieval_topk.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    import ctypes
    for lib in (_lib.load(), ctypes.CDLL(os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so"))):
        assert hasattr(lib, "octmae_retrieval_topk") and hasattr(lib, "octmae_retrieval_topk_ws")
        assert lib.octmae_abi_version() == _lib.expected_abi_version()


# ---------------------------------------------------------------------------------------------- the accuracy
def test_match_accuracy_equals_the_scripts_expressions_on_full_lists():
    from octcubem_amd import coem
    rng = np.random.default_rng(11)
    n = 37
    attr = rng.integers(0, 2, size=n)
    idx = np.stack([rng.permutation(n)[:10] for _ in range(n)])
    got = coem.topk_match_accuracy(idx, attr, attr)
    assert list(got) == [1, 3, 5, 10]
    for k in (1, 3, 5, 10):
        count, micro, macro = T.script_accuracy(idx[:, :k], attr)
        assert count == int((attr[idx[:, :k]] == attr[:, None]).sum()) and 0 < count < n * k
        assert round(got[k]["Micro Accuracy"] * n * k) == count                        # the integer behind the quotient
        assert abs(got[k]["Micro Accuracy"] - micro) <= 1e-12 and abs(got[k]["Macro Accuracy"] - macro) <= 1e-12
        assert isinstance(got[k]["Micro Accuracy"], float) and isinstance(got[k]["Macro Accuracy"], float)
    # a different attribute on the two sides, a tensor as input
    ga = rng.integers(0, 3, size=n)
    got = coem.topk_match_accuracy(torch.from_numpy(idx), torch.from_numpy(attr), list(ga), topk_list=(2,))
    assert abs(got[2]["Micro Accuracy"] - float((ga[idx[:, :2]] == attr[:, None]).mean())) <= 1e-12


def test_match_accuracy_never_counts_an_open_slot():
    from octcubem_amd import coem
    qa = ["R", "L", "R", "L"]
    ga = ["R", "R", "L", "L", "R"]
    idx = np.array([[0, 2, 4],          # R: R L R   -> 2 of 3
                    [3, -1, -1],        # L: L       -> 1 of 1
                    [-1, -1, -1],       # no candidate: no slot, no row of the macro mean
                    [1, 2, -1]])        # L: R L     -> 1 of 2
    got = coem.topk_match_accuracy(idx, qa, ga, topk_list=(1, 2, 3))
    assert got[1] == {"Micro Accuracy": 2 / 3, "Macro Accuracy": (1 + 1 + 0) / 3}
    assert got[2] == {"Micro Accuracy": 3 / 5, "Macro Accuracy": (1 / 2 + 1 + 1 / 2) / 3}
    assert got[3] == {"Micro Accuracy": 4 / 6, "Macro Accuracy": (2 / 3 + 1 + 1 / 2) / 3}
    nothing = coem.topk_match_accuracy(np.full((2, 2), -1), ["a", "b"], ["a"], topk_list=(2,))
    assert np.isnan(nothing[2]["Micro Accuracy"]) and np.isnan(nothing[2]["Macro Accuracy"])
    with pytest.raises(ValueError, match="k = 4"):
        coem.topk_match_accuracy(idx, qa, ga, topk_list=(1, 4))
    with pytest.raises(ValueError, match="outside"):
        coem.topk_match_accuracy(np.array([[5, 0, 0]] * 4), qa, ga, topk_list=(1,))


# ---------------------------------------------------------------------------------------------- retrieve_topk, retrieval_report
def features(n=12, d=4, seed=2):
    """dyadic features: multiples of 1/4, every score a multiple of 1/16 -- exact in f32 and float64, with ties"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-2, 3, size=(n, d)) / 4).astype(np.float32), (rng.integers(-2, 3, size=(n, d)) / 4).astype(np.float32)


def test_retrieve_topk_maps_labels_through_one_dictionary():
    from octcubem_amd import coem
    img, txt = features()
    seen = {}

    def spy(a, b, k, keep=None, row_group=None, col_group=None):
        seen.update(k=k, keep=None if keep is None else keep.tolist(), rg=row_group.tolist(), cg=col_group.tolist(),
                    dtypes=(row_group.dtype, col_group.dtype, a.dtype))
        return T.topk_fn()(a, b, k, keep, row_group, col_group)
    qg = ["p7", "p3", "p7", ("p", 1)]
    gg = ["p3", "new", "p7", ("p", 1), "p3", "new"]
    idx, score = coem.retrieve_topk(img[:4], txt[:6].astype(np.float64), 3, query_groups=qg, gallery_groups=gg,
                                    keep=[1, 1, 1, 0, 2, 1], topk=spy)
    assert seen["rg"] == [0, 1, 0, 2] and seen["cg"] == [1, 3, 0, 2, 1, 3] and seen["keep"] == [1, 1, 1, 0, 1, 1] and seen["k"] == 3
    assert seen["dtypes"] == (torch.int32, torch.int32, torch.float32)
    assert idx.dtype == np.int64 and score.dtype == np.float32 and idx.shape == score.shape == (4, 3)
    want_idx, want_score = T.topk_from(R.f64_scores(img[:4], txt[:6]), 3, np.array([1, 1, 1, 0, 1, 1]), np.array(seen["rg"]),
                                       np.array(seen["cg"]))
    assert np.array_equal(idx, want_idx) and np.array_equal(score, want_score.astype(np.float32))
    for i in range(4):
        assert all(j == -1 or (gg[j] != qg[i] and j != 3) for j in idx[i])
    assert (idx[3] >= 0).all() and (idx[1] == -1).sum() == 0                  # 5 / 3 candidates
    with pytest.raises(ValueError, match="together"):
        coem.retrieve_topk(img, txt, 3, query_groups=list(range(12)), topk=spy)
    with pytest.raises(ValueError, match="query groups"):
        coem.retrieve_topk(img, txt, 3, query_groups=[1, 2], gallery_groups=list(range(12)), topk=spy)
    with pytest.raises(ValueError, match="keep needs"):
        coem.retrieve_topk(img, txt, 3, keep=[1, 0], topk=spy)


def test_cpu_features_without_a_topk_function_raise():
    from octcubem_amd import coem
    img, txt = features()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        coem.retrieve_topk(torch.from_numpy(img), torch.from_numpy(txt), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        coem.retrieve_topk(img, txt, 3)


def test_retrieval_report_writes_the_scripts_table(tmp_path):
    from octcubem_amd import coem
    n = 12
    img, txt = features(n)
    patients = [f"pat-{i // 3}" for i in range(n)]                            # four patients of three samples
    side = [i % 2 for i in range(n)]
    path = os.path.join(str(tmp_path), "retrieval_results_3.npz")
    np.savez(path, image_features=img, text_features=txt, logit_scale=np.full(2, 14.0, dtype=np.float32))
    out = os.path.join(str(tmp_path), "tables")
    rep = coem.retrieval_report(path, side, patients, out, "modelA", topk_list=(1, 3, 5), topk=T.topk_fn())
    assert sorted(rep) == ["accuracy", "indices", "scores"] and rep["indices"].shape == (n, 5) and rep["indices"].dtype == np.int64
    s = R.f64_scores(img, txt)
    gid = np.array([i // 3 for i in range(n)])
    want_idx, want_score = T.topk_from(s, 5, None, gid, gid)
    assert np.array_equal(rep["indices"], want_idx) and np.array_equal(rep["scores"], want_score.astype(np.float32))
    assert (rep["indices"] >= 0).all()
    for i in range(n):                                                        # no returned sample is of the query's patient
        assert all(patients[j] != patients[i] for j in rep["indices"][i])
    # the accuracy is the script's, on its own masked matrix (full lists: 9 candidates per query)
    masked = s.copy()
    masked[gid[:, None] == gid[None, :]] = -1e5
    for k in (1, 3, 5):
        count, micro, macro = T.script_accuracy(T.topk_from(masked, k)[0], np.array(side))
        assert abs(rep["accuracy"][k]["Micro Accuracy"] - micro) <= 1e-12 and abs(rep["accuracy"][k]["Macro Accuracy"] - macro) <= 1e-12
    # the file: the k values, the micro row, the macro row
    assert os.listdir(out) == ["modelA_laterality.csv"]
    text = open(os.path.join(out, "modelA_laterality.csv")).read()
    assert text.endswith("\n") and "\r" not in text
    rows = list(csv.reader(text.splitlines()))
    assert len(rows) == 3 and rows[0] == ["1", "3", "5"]
    assert [float(v) for v in rows[1]] == [rep["accuracy"][k]["Micro Accuracy"] for k in (1, 3, 5)]
    assert [float(v) for v in rows[2]] == [rep["accuracy"][k]["Macro Accuracy"] for k in (1, 3, 5)]
    # the swap: the other tower asks, another name
    swapped = coem.retrieval_report(dict(np.load(path)), side, patients, out, "modelA", topk_list=(1, 3, 5), ir_oct=True,
                                    attribute_name="eye", topk=T.topk_fn())
    assert sorted(os.listdir(out)) == ["modelA_eye_ir.csv", "modelA_laterality.csv"]
    assert np.array_equal(swapped["indices"], T.topk_from(s.T, 5, None, gid, gid)[0])
    assert not np.array_equal(swapped["indices"], rep["indices"])
    with pytest.raises(ValueError, match="returned"):                         # a topk function that delivers shorter lists than asked
        coem.retrieval_report(path, side, patients, out, "m", topk_list=(1, 3), topk=lambda a, b, k, **kw: T.topk_fn()(a, b, 2, **kw))
