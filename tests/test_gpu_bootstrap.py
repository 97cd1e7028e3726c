"""GPU tests of the bootstrap kernel (csrc/bootstrap.hip through ops.bootstrap_rank_metrics) against the numpy restatement of
tests/bootstrap_ref.py on identical multiplicities: P, N and U2 EQUAL, ap_sum / P and auprc within SUM_BOUND(n), max_f1 within F1_BOUND
(both derived in tests/bootstrap_ref.py), at every edge of the walk -- the 256 positions of a wave and of the block, the 1024 of a
chunk, read out of the source -- and at the switch between a staged and a gathered row of multiplicities; the host finish above it,
the refusals in front of it, and engine_finetune.evaluate_report end to end on a stub model."""
import csv
import functools
import os
import types

import numpy as np
import pytest
import torch

from tests import bootstrap_ref as B
from tests import metrics_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BLOCK, CHUNK, STAGED = B.kernel_constants()
# 1 / 2: below a thread's four positions; the block (which is also what one wave covers: 64 threads x 4 positions) and a chunk, each
# with a position less and one more; three chunks and a ragged fourth
NS = (1, 2, BLOCK - 1, BLOCK, BLOCK + 1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5)
LAYOUTS = ("distinct", "all_tied", "straddling_ties", "zero_weight_lead")
KEYS = ("roc_auc", "AP", "auprc", "max_f1")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


@functools.lru_cache(maxsize=None)
def walk_case(n, C, R, layout):
    """(scores float32 [n, C], labels uint8 [n, C], mult int32 [R, n], the reference's six outputs), seeded; computed once."""
    rng = np.random.default_rng([n, C, R, LAYOUTS.index(layout)])
    s = np.empty((n, C), dtype=np.float32)
    for c in range(C):
        p = np.arange(n)
        if layout == "distinct":
            gid = p
        elif layout == "all_tied":
            gid = np.zeros(n, dtype=np.int64)
        elif layout == "straddling_ties":
            # single positions, but one group over the wave boundary at BLOCK (positions BLOCK - 6 + c .. BLOCK + 5) and one over the
            # chunk boundary (CHUNK - 3 .. CHUNK + 3 + c), clipped by n
            gid = p.copy()
            gid[(p >= BLOCK - 6 + c) & (p < BLOCK + 6)] = BLOCK - 6 + c
            gid[(p >= CHUNK - 3) & (p < CHUNK + 4 + c)] = CHUNK - 3
        else:
            gid = p // 3                                         # groups of three
        s[rng.permutation(n), c] = -gid.astype(np.float32)       # position p of the descending order holds group gid[p]
    lab = rng.integers(0, 2, size=(n, C)).astype(np.uint8)
    mult = np.stack([np.bincount(rng.integers(0, n, n), minlength=n) for _ in range(R)]).astype(np.int32)
    if layout == "zero_weight_lead":
        for uid, _, _, end in B.sorted_columns(s, lab):
            mult[:, uid[:np.nonzero(end)[0][min(1, int(end.sum()) - 1)] + 1]] = 0      # the first two groups of every class
    want = B.rank_metrics(s, lab, mult)
    for a in (s, lab, mult):
        a.setflags(write=False)
    return s, lab, mult, want


def run_op(s, lab, mult, unit=None, valid=None):
    from octcubem_amd import ops
    got = ops.bootstrap_rank_metrics(dev(s), dev(lab), dev(mult), None if unit is None else dev(unit), None if valid is None else dev(valid))
    assert tuple(got) == ("P", "N", "U2", "ap_sum", "auprc", "max_f1")
    R, C = mult.shape[0], s.shape[1]
    for k, v in got.items():
        assert v.is_cuda and tuple(v.shape) == (R, C) and v.is_contiguous() and v.dtype == (torch.int64 if k in ("P", "N", "U2") else torch.float64)
    return {k: v.cpu().numpy() for k, v in got.items()}


@pytest.mark.parametrize("n", NS)
def test_the_walk_equals_the_restatement_at_every_edge(n):
    for layout in LAYOUTS:
        for C in (1, 3):
            for R in (1, 7):
                s, lab, mult, want = walk_case(n, C, R, layout)
                bad = B.mismatches(run_op(s, lab, mult), want, n)
                assert not bad, f"n={n} C={C} R={R} {layout}: {len(bad)} outputs differ, first {bad[0]}"


def test_the_layouts_hold_what_they_are_named_for():
    n = 3 * CHUNK + 5
    s, lab, mult, _ = walk_case(n, 3, 7, "straddling_ties")
    for c, (_, _, _, end) in enumerate(B.sorted_columns(s, lab)):
        assert not end[BLOCK - 6 + c:BLOCK + 5].any() and end[BLOCK + 5] and end[BLOCK - 7 + c]      # one group over position BLOCK
        assert not end[CHUNK - 3:CHUNK + 3 + c].any() and end[CHUNK + 3 + c] and end[CHUNK - 4]       # one group over position CHUNK
    s, lab, mult, want = walk_case(n, 3, 7, "zero_weight_lead")
    for uid, _, _, end in B.sorted_columns(s, lab):
        assert (mult[:, uid[:6]] == 0).all() and end[:6].sum() == 2
    assert (want["P"] > 0).all() and (want["N"] > 0).all()
    s, lab, _, _ = walk_case(n, 1, 1, "all_tied")
    assert B.sorted_columns(s, lab)[0][3].sum() == 1               # one group spans every chunk
    assert NS[-1] > 3 * CHUNK and BLOCK == 256 and CHUNK == 4 * BLOCK


def explicit_problem():
    rng = np.random.default_rng(77)
    n, C = CHUNK + 1, 2
    s = (rng.integers(0, 64, (n, C)) / 8).astype(np.float32)
    lab = rng.integers(0, 2, (n, C)).astype(np.uint8)
    lab[:2] = ((1, 1), (0, 0))
    mult = np.ones((4, n), dtype=np.int32)
    mult[1] = lab[:, 0] == 0                                    # no positive of class 0 drawn
    mult[2] = lab[:, 1] == 1                                    # no negative of class 1 drawn
    mult[3] = 0
    mult[3, 5] = n                                              # one unit drawn n times
    return s, lab, mult


def test_explicit_rows_of_multiplicities():
    from octcubem_amd import metrics, ops
    s, lab, mult = explicit_problem()
    n = s.shape[0]
    want = B.rank_metrics(s, lab, mult)
    got = run_op(s, lab, mult)
    assert B.mismatches(got, want, n) == []
    assert got["P"][1, 0] == 0 and got["N"][1, 0] > 0 and got["N"][2, 1] == 0 and got["P"][2, 1] > 0
    assert sorted((got["P"][3] + got["N"][3]).tolist()) == [n, n] and ((got["P"][3] == 0) | (got["N"][3] == 0)).all()
    # all ones: the point estimates of the existing path, the AUROC bit for bit
    point = metrics.binary_rank_metrics(ops.rank_counts(dev(s), dev(lab)), lab)
    fin = B.finish(got)
    assert np.array_equal(fin["roc_auc"][0], point["roc_auc"])
    assert np.abs(fin["AP"][0] - point["AP"]).max() <= B.SUM_BOUND(n) and np.abs(fin["auprc"][0] - point["auprc"]).max() <= B.SUM_BOUND(n)
    assert np.abs(fin["max_f1"][0] - point["max_f1"]).max() <= B.F1_BOUND
    # the host finish on the device op: undefined pairs are NaN and are counted
    res = metrics.bootstrap_rank_metrics(dev(s), dev(lab), mult=dev(mult))
    for k in KEYS:
        x = res[k]["samples"]
        assert np.isnan(x[1, 0]) and np.isnan(x[2, 1]) and np.isnan(x[3]).all() and np.isnan(x).sum() == 4
        assert list(res[k]["n_defined"]) == [2, 2] and res["macro"][k]["n_defined"] == 1
        assert np.array_equal(res[k]["point"], point[k])
        assert np.array_equal(x, fin[k], equal_nan=True)


def test_clusters_of_one_to_nine_with_a_mask_per_class():
    rng = np.random.default_rng(78)
    U, C = 300, 3
    unit = rng.permutation(np.repeat(np.arange(U), 1 + np.arange(U) % 9)).astype(np.int64)
    n = unit.size
    assert n > CHUNK and np.bincount(unit).min() == 1 and np.bincount(unit).max() == 9
    s = (rng.integers(0, 200, (n, C)) / 8).astype(np.float32)
    lab = rng.integers(0, 2, (n, C)).astype(np.uint8)
    valid = (rng.integers(0, 4, (n, C)) > 0).astype(np.uint8)
    assert not np.array_equal(valid[:, 0], valid[:, 1]) and not np.array_equal(valid[:, 1], valid[:, 2])
    mult = np.stack([np.bincount(rng.integers(0, U, U), minlength=U) for _ in range(5)]).astype(np.int32)
    want = B.rank_metrics(s, lab, mult, unit, valid)
    assert B.mismatches(run_op(s, lab, mult, unit, valid), want, n) == []
    assert B.mismatches(run_op(s, lab, mult, unit.astype(np.int32), valid.astype(bool)), want, n) == []
    # a NaN outside the population is legal and weighs nothing
    s2 = s.copy()
    s2[valid == 0] = np.nan
    assert np.isnan(s2).any() and B.mismatches(run_op(s2, lab, mult, unit, valid), want, n) == []


@pytest.mark.parametrize("U", (STAGED, STAGED + 1))
def test_staged_and_gathered_rows_of_multiplicities(U):
    """U <= BS_LDS_UNITS: the row of mult is staged in LDS; one unit more: gathered from global memory.  The highest ids are used."""
    rng = np.random.default_rng(U)
    n, C, R = CHUNK + 300, 2, 3
    unit = rng.integers(0, U, n)
    unit[:4] = (U - 1, 0, U - 1, U - 2)
    s = (rng.integers(0, 100, (n, C)) / 8).astype(np.float32)
    lab = rng.integers(0, 2, (n, C)).astype(np.uint8)
    mult = rng.integers(0, 3, (R, U)).astype(np.int32)
    assert B.mismatches(run_op(s, lab, mult, unit), B.rank_metrics(s, lab, mult, unit), n) == []


def test_multiplicities_sum_to_the_units_and_repeat():
    from octcubem_amd import metrics
    a = metrics.bootstrap_multiplicities(9, 1237, 3, DEV)
    assert a.is_cuda and a.dtype == torch.int32 and tuple(a.shape) == (9, 1237)
    assert bool((a.sum(1) == 1237).all()) and bool((a >= 0).all())
    assert torch.equal(a, metrics.bootstrap_multiplicities(9, 1237, 3, DEV))
    assert not torch.equal(a, metrics.bootstrap_multiplicities(9, 1237, 4, DEV)) and not torch.equal(a[0], a[1])


def test_column_slices_of_wider_buffers():
    from octcubem_amd import ops
    s, lab, mult, want = walk_case(CHUNK + 1, 3, 7, "zero_weight_lead")
    n = s.shape[0]
    rng = np.random.default_rng(5)
    wide_s = dev(rng.standard_normal((n, 7)).astype(np.float32))
    wide_l = dev(rng.integers(0, 2, (n, 6)).astype(np.uint8))
    wide_v = torch.zeros((n, 5), dtype=torch.bool, device=DEV)
    wide_s[:, 2:5], wide_l[:, 1:4], wide_v[:, 2:5] = dev(s), dev(lab), True
    got = ops.bootstrap_rank_metrics(wide_s[:, 2:5], wide_l[:, 1:4], dev(mult), None, wide_v[:, 2:5])
    assert B.mismatches({k: v.cpu().numpy() for k, v in got.items()}, want, n) == []
    with pytest.raises(ValueError, match="stride"):
        ops.bootstrap_rank_metrics(wide_s.t()[2:5].t()[:, ::2], wide_l[:, 1:3], dev(mult))


def test_refusals_raise_before_any_launch(monkeypatch):
    from octcubem_amd import ops
    s, lab, mult, _ = walk_case(BLOCK + 1, 3, 7, "distinct")
    n = s.shape[0]
    ds, dl, dm = dev(s), dev(lab), dev(mult)
    unit = torch.arange(n, device=DEV)
    launched = []
    monkeypatch.setattr(ops, "call", lambda *a: launched.append(a[0]))
    for bad in (-1, n):
        u = unit.clone()
        u[n // 2] = bad
        with pytest.raises(ValueError, match="unit ids"):
            ops.bootstrap_rank_metrics(ds, dl, dm, u)
    m = dm.clone()
    m[3, 7] = -1
    with pytest.raises(ValueError, match="negative"):
        ops.bootstrap_rank_metrics(ds, dl, m)
    nan = ds.clone()
    nan[5, 1] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        ops.bootstrap_rank_metrics(nan, dl, dm)
    valid = torch.ones_like(dl)
    with pytest.raises(ValueError, match="NaN at a valid position"):
        ops.bootstrap_rank_metrics(nan, dl, dm, None, valid)
    big = torch.full_like(dm, 2 ** 23)                           # a row sums to 257 x 2^23 >= 2^31
    with pytest.raises(ValueError, match="32-bit"):
        ops.bootstrap_rank_metrics(ds, dl, big)
    with pytest.raises(ValueError, match="32-bit"):              # a cluster of 249 samples, a row sum of 2^28
        ops.bootstrap_rank_metrics(ds, dl, torch.full((1, 2), 2 ** 27, dtype=torch.int32, device=DEV), (unit >= 8).long())
    for args in ((ds.cpu(), dl, dm), (ds, dl.cpu(), dm), (ds, dl, dm.cpu()), (ds, dl, dm, unit.cpu())):
        with pytest.raises(RuntimeError, match="GPU tensors"):
            ops.bootstrap_rank_metrics(*args)
    with pytest.raises(TypeError):
        ops.bootstrap_rank_metrics(ds.double(), dl, dm)
    with pytest.raises(TypeError):
        ops.bootstrap_rank_metrics(ds, dl, dm.long())
    with pytest.raises(ValueError, match="mult"):
        ops.bootstrap_rank_metrics(ds, dl, dm[:, :-1])
    assert launched == []
    ops.bootstrap_rank_metrics(ds, dl, dm)
    assert launched == ["octmae_bootstrap_rank_metrics"]


@pytest.mark.parametrize("task_mode", ("multi_cls", "multi_label"))
def test_report_end_to_end_on_a_stub_model(task_mode, tmp_path):
    from octcubem_amd import engine_finetune, metrics
    multi_label = task_mode == "multi_label"
    loader, model, _ = B.stub_problem(multi_label)
    model = model.to(DEV)
    crit = torch.nn.BCEWithLogitsLoss() if multi_label else torch.nn.CrossEntropyLoss()
    names = ["amd", "dme", "normal"]
    args = types.SimpleNamespace(bootstrap=16, bootstrap_seed=6)
    plain = engine_finetune.evaluate_report(loader, model, DEV, str(tmp_path / "off"), 1, "val", 3, criterion=crit, task_mode=task_mode,
                                            disease_list=names)
    got = engine_finetune.evaluate_report(loader, model, DEV, str(tmp_path / "on"), 1, "val", 3, criterion=crit, task_mode=task_mode,
                                          disease_list=names, args=args)
    assert got == plain
    assert set(os.listdir(tmp_path / "on")) == set(os.listdir(tmp_path / "off")) | {"metrics_ci_val.csv"}
    with torch.no_grad():
        logits = torch.cat([model(b[0].to(DEV)) for b in loader]).float()
    targets = torch.cat([b[1] for b in loader]).to(DEV)
    scores = torch.sigmoid(logits) if multi_label else torch.softmax(logits, dim=1)
    labels = (targets != 0) if multi_label else torch.nn.functional.one_hot(targets.long(), 3).to(torch.uint8)
    want = metrics.bootstrap_rank_metrics(scores, labels, resamples=16, seed=6)
    # the same multiplicities through the numpy restatement: every class is defined in all 16 resamples
    mult = metrics.bootstrap_multiplicities(16, 48, 6, DEV)
    ref = metrics.bootstrap_rank_metrics(scores.cpu().numpy(), labels.cpu().numpy(), mult=mult.cpu().numpy(), kernel=B.rank_metrics,
                                         rank_counts=metrics_ref.rank_counts)
    rows = list(csv.reader(open(tmp_path / "on" / "metrics_ci_val.csv", newline="", encoding="utf8")))
    assert rows[0] == engine_finetune.CI_HEADER and [(r[1], r[2]) for r in rows[1:]] == [(k, c) for k in KEYS for c in ["macro"] + names]
    for r in rows[1:]:
        assert r[0] == "1" and r[6:] == ["16", "16", "0.05", "6", "sample"]
        i = None if r[2] == "macro" else names.index(r[2])
        part, rpart = (want["macro"][r[1]], ref["macro"][r[1]]) if i is None else (want[r[1]], ref[r[1]])
        pick = (lambda v: float(v)) if i is None else (lambda v: float(v[i]))
        assert [float(r[3]), float(r[4]), float(r[5])] == [pick(part["point"]), pick(part["low"]), pick(part["high"])]
        assert int(pick(rpart["n_defined"])) == 16
        if r[1] == "roc_auc":                                    # exact integers on both sides: the same samples, the same quantiles
            assert [float(r[4]), float(r[5])] == [pick(rpart["low"]), pick(rpart["high"])]
