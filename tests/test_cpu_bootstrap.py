"""CPU tests of the bootstrap intervals of the fine-tune evaluation: the numpy restatement of the kernel (tests/bootstrap_ref.py)
against resamples that are materialised row by row and sent through the EXISTING metric path, the host finish of
octcubem_amd.metrics.bootstrap_rank_metrics / bootstrap_compare on that restatement, the derived bounds against three planted
mistakes of a chunked walk, the opt-in of engine_finetune.evaluate_report, and the declaration of the entry point.

Bounds: tests/bootstrap_ref.py derives them (SUM_BOUND, F1_BOUND); none is measured."""
import csv
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from octcubem_amd import _lib, engine_finetune, metrics
from tests import bootstrap_ref as B
from tests import metrics_ref, multitask_ref

KEYS = ("roc_auc", "AP", "auprc", "max_f1")


def problems():
    """name -> (scores [n, C], labels, unit or None, valid or None, mult [R, U]); n <= 300."""
    rng = np.random.default_rng(5)
    out = {}

    def draws(R, U):
        return np.stack([np.bincount(rng.integers(0, U, U), minlength=U) for _ in range(R)]).astype(np.int32)

    n = 120
    y = rng.integers(0, 2, (n, 2))
    out["distinct"] = (rng.permutation(2 * n).reshape(n, 2).astype(np.float32), y, None, None, draws(4, n))
    out["heavy_ties"] = ((rng.integers(0, 6, (n, 2)) / 8).astype(np.float32), y, None, None, draws(4, n))
    out["all_tied"] = (np.full((n, 2), 0.25, dtype=np.float32), y, None, None, draws(3, n))
    s = rng.choice(np.array([np.inf, -np.inf, 0.0, -0.0, 1e-40, -1e-40, 1.5], dtype=np.float32), (n, 2))
    out["inf_and_signed_zero"] = (s, y, None, None, draws(4, n))
    valid = rng.integers(0, 3, (n, 2)) > 0
    out["valid_masks"] = ((rng.integers(0, 12, (n, 2)) / 8).astype(np.float32), y, None, valid, draws(4, n))
    sizes = 1 + np.arange(40) % 9                                # clusters of 1 .. 9 samples
    unit = rng.permutation(np.repeat(np.arange(40), sizes))
    m = unit.size
    ym = rng.integers(0, 2, (m, 2))
    sm = (rng.integers(0, 30, (m, 2)) / 8).astype(np.float32)
    out["clusters"] = (sm, ym, unit, None, draws(4, 40))
    out["clusters_masked"] = (sm, ym, unit, rng.integers(0, 4, (m, 2)) > 0, draws(4, 40))
    # the units at the top of the order are never drawn: the first tie groups weigh nothing
    s1 = np.arange(n, 0, -1, dtype=np.float32)[:, None] // 3
    mult = draws(3, n)
    mult[:, :15] = 0
    mult[1, :60] = 0
    out["zero_weight_at_the_top"] = (s1, rng.integers(0, 2, (n, 1)), None, None, mult)
    # one unit drawn n times, a resample without a positive, one without a negative
    y1 = rng.integers(0, 2, (n, 1))
    y1[:2, 0] = (1, 0)
    special = np.zeros((3, n), dtype=np.int32)
    special[0, 7] = n
    special[1] = (y1[:, 0] == 0) * 2
    special[2] = (y1[:, 0] == 1) * 3
    out["degenerate_rows"] = ((rng.integers(0, 9, (n, 1)) / 8).astype(np.float32), y1, None, None, special)
    return out


PROBLEMS = problems()


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_restatement_equals_materialised_resamples(name):
    s, y, unit, valid, mult = PROBLEMS[name]
    n, C = s.shape
    raw = B.rank_metrics(s, y, mult, unit, valid)
    got = B.finish(raw)
    undefined = 0
    for r in range(mult.shape[0]):
        for c in range(C):
            try:
                want, rows = B.brute_force(s, y, mult[r], unit, valid, c)
            except ValueError:                                   # the existing path raises: one label value (or nothing) in the resample
                assert raw["P"][r, c] == 0 or raw["N"][r, c] == 0
                assert all(np.isnan(got[k][r, c]) for k in KEYS)
                undefined += 1
                continue
            assert raw["P"][r, c] + raw["N"][r, c] == rows
            assert got["roc_auc"][r, c] == want["roc_auc"], (r, c)
            terms = max(n, rows)
            assert abs(got["AP"][r, c] - want["AP"]) <= B.SUM_BOUND(terms), (r, c)
            assert abs(got["auprc"][r, c] - want["auprc"]) <= B.SUM_BOUND(terms), (r, c)
            assert abs(got["max_f1"][r, c] - want["max_f1"]) <= B.F1_BOUND, (r, c)
    assert undefined == (3 if name == "degenerate_rows" else 0)


def test_the_cases_hold_what_they_are_named_for():
    s, y, _, _, mult = PROBLEMS["zero_weight_at_the_top"]
    (uid, _, _, end), = B.sorted_columns(s, y)
    first_two = np.nonzero(end)[0][1] + 1
    assert (mult[:, uid[:first_two]] == 0).all() and end[:first_two].sum() == 2
    s = PROBLEMS["inf_and_signed_zero"][0]
    (_, _, _, end), = B.sorted_columns(s[:, :1], np.zeros_like(s[:, :1]))
    assert end.sum() == 6                                        # seven values, -0.0 ties with 0.0
    assert (np.bincount(PROBLEMS["clusters"][2]).min(), np.bincount(PROBLEMS["clusters"][2]).max()) == (1, 9)


# ---------------------------------------------------------------------------------------------- the bounds catch a fault
def test_the_bounds_catch_three_planted_faults():
    block, chunk, _ = B.kernel_constants()
    rng = np.random.default_rng(11)
    n = 2 * chunk + 77
    s = (rng.integers(0, 400, (n, 1)) / 8).astype(np.float32)
    y = rng.integers(0, 2, (n, 1))
    mult = np.stack([np.bincount(rng.integers(0, n, n), minlength=n) for _ in range(2)]).astype(np.int32)
    (uid, _, _, end), = B.sorted_columns(s, y)
    ends = np.nonzero(end)[0]
    mult[:, uid[:ends[1] + 1]] = 0                               # the first two groups weigh nothing ...
    third = uid[ends[1] + 1:ends[2] + 1]
    y[third], mult[:, third] = 1, 2                              # ... and the first weight is a positive's
    want = B.rank_metrics(s, y, mult)
    assert B.mismatches(B.rank_metrics(s, y, mult), want, n) == []
    faults = {"drop_end": int(end.sum()) // 2, "lose_carry": chunk, "lead_precision_0": None}
    assert set(faults) == set(B.FAULTS)
    for fault, at in faults.items():
        bad = B.mismatches(B.rank_metrics(s, y, mult, fault=fault, fault_at=at), want, n)
        assert bad, f"{fault} went unnoticed"
        hit = {k for k, *_ in bad}
        if fault == "lead_precision_0":
            assert hit == {"auprc"}                              # the one output that reads the precision in front of the first weight
        else:
            assert "U2" in hit and hit & {"ap_sum", "auprc", "max_f1"}


# ---------------------------------------------------------------------------------------------- the host finish
def host_problem():
    rng = np.random.default_rng(21)
    n, C, R = 90, 3, 40
    y = rng.integers(0, 2, (n, C))
    y[:2] = ((1, 1, 1), (0, 0, 0))
    s = (0.5 * y + rng.random((n, C))).astype(np.float32)
    mult = np.stack([np.bincount(rng.integers(0, n, n), minlength=n) for _ in range(R)]).astype(np.int32)
    mult[3] = np.where(y[:, 1] == 1, 0, mult[3])                 # resample 3 draws no positive of class 1
    mult[5] = np.where(y[:, 2] == 0, 0, mult[5])                 # resample 5 draws no negative of class 2
    return s, y, mult


def test_quantiles_counts_and_the_macro_rule():
    s, y, mult = host_problem()
    res = metrics.bootstrap_rank_metrics(s, y, mult=mult, alpha=0.1, kernel=B.rank_metrics, rank_counts=metrics_ref.rank_counts)
    assert res["resamples"] == 40 and res["level"] == "sample"
    samples = B.finish(B.rank_metrics(s, y, mult))
    point = metrics.binary_rank_metrics(metrics_ref.rank_counts(s, y), y)
    for k in KEYS:
        got = res[k]
        assert np.array_equal(got["point"], point[k])
        assert got["samples"].dtype == np.float64 and np.array_equal(got["samples"], samples[k], equal_nan=True)
        assert list(got["n_defined"]) == [40, 39, 39]
        assert np.isnan(got["samples"][3, 1]) and np.isnan(got["samples"][5, 2]) and np.isnan(got["samples"]).sum() == 2
        for c in range(3):
            col = samples[k][:, c]
            col = col[~np.isnan(col)]
            assert got["low"][c] == np.quantile(col, 0.05) and got["high"][c] == np.quantile(col, 0.95)
            assert got["low"][c] <= got["high"][c]
        macro = res["macro"][k]
        keep = [r for r in range(40) if r not in (3, 5)]
        assert macro["n_defined"] == 38 and np.isnan(macro["samples"][[3, 5]]).all()
        assert np.allclose(macro["samples"][keep], samples[k][keep].mean(axis=1), rtol=0, atol=1e-15)
        assert macro["point"] == float(np.mean(point[k]))
        assert macro["low"] == np.quantile(macro["samples"][keep], 0.05) and macro["high"] == np.quantile(macro["samples"][keep], 0.95)


def test_a_class_that_is_never_defined_raises():
    s, y, mult = host_problem()
    mult = np.where(y[:, 1] == 1, 0, mult).astype(np.int32)      # no resample draws a positive of class 1
    with pytest.raises(ValueError, match="class 1"):
        metrics.bootstrap_rank_metrics(s, y, mult=mult, kernel=B.rank_metrics, rank_counts=metrics_ref.rank_counts)
    with pytest.raises(ValueError, match="alpha"):
        metrics.bootstrap_rank_metrics(s, y, mult=mult, alpha=1.0, kernel=B.rank_metrics, rank_counts=metrics_ref.rank_counts)
    with pytest.raises(ValueError, match="mult"):
        metrics.bootstrap_rank_metrics(s, y, mult=mult[:, :-1], kernel=B.rank_metrics, rank_counts=metrics_ref.rank_counts)


def test_drawn_multiplicities_groups_and_masks():
    """Without ``mult`` the draw is bootstrap_multiplicities on the CPU stream; ``groups`` of any hashable type become dense unit ids in
    order of first occurrence; ``valid`` reaches both the counter of the point estimates and the kernel."""
    m = metrics.bootstrap_multiplicities(7, 33, 4, "cpu")
    assert m.dtype == torch.int32 and m.shape == (7, 33) and (m.sum(1) == 33).all() and (m >= 0).all()
    assert torch.equal(m, metrics.bootstrap_multiplicities(7, 33, 4, "cpu")) and not torch.equal(m, metrics.bootstrap_multiplicities(7, 33, 5, "cpu"))
    s, y, _ = host_problem()
    n = s.shape[0]
    groups = [f"patient-{(i * 7) % 30}" for i in range(n)]
    ids, U = metrics._dense_ids(groups)
    assert U == 30 and list(ids[:4]) == [0, 1, 2, 3] and all(groups[i] == groups[j] for i in range(n) for j in range(n) if ids[i] == ids[j])
    valid = np.ones_like(y)
    valid[10:30, 0] = 0
    seen = []

    def kernel(scores, labels, mult, unit=None, valid=None):
        seen.append((np.asarray(mult), None if unit is None else np.asarray(unit), valid))
        return B.rank_metrics(scores, labels, mult, unit, valid)

    res = metrics.bootstrap_rank_metrics(s, y, resamples=12, seed=4, groups=groups, valid=valid, kernel=kernel, rank_counts=multitask_ref.rank_counts)
    (mult, unit, val), = seen
    assert res["level"] == "group" and res["resamples"] == 12
    assert np.array_equal(mult, metrics.bootstrap_multiplicities(12, 30, 4, "cpu").numpy()) and np.array_equal(unit, ids)
    assert np.array_equal(val, valid)
    want = metrics.binary_rank_metrics(multitask_ref.rank_counts_masked(s, y, valid), y, valid=valid)
    assert all(np.array_equal(res[k]["point"], want[k]) for k in KEYS)
    with pytest.raises(ValueError, match="group ids"):
        metrics.bootstrap_rank_metrics(s, y, groups=groups[:-1], kernel=kernel, rank_counts=multitask_ref.rank_counts)
    with pytest.raises(TypeError):                               # no kernel and host arrays: there is no CPU path
        metrics.bootstrap_rank_metrics(s, y, resamples=4, rank_counts=metrics_ref.rank_counts)


def test_compare_identical_and_planted():
    s, y, mult = host_problem()
    kw = dict(mult=mult, kernel=B.rank_metrics, rank_counts=metrics_ref.rank_counts)
    same = metrics.bootstrap_compare(s, s.copy(), y, **kw)
    for k in KEYS:
        for part in (same[k], same["macro"][k]):
            assert np.all(np.asarray(part["delta_point"]) == 0) and np.all(np.asarray(part["delta_low"]) == 0)
            assert np.all(np.asarray(part["delta_high"]) == 0) and np.all(np.asarray(part["p"]) == 1.0)
        assert list(same[k]["n_defined"]) == [40, 39, 39] and same["macro"][k]["n_defined"] == 38
    rng = np.random.default_rng(3)
    better = (2.0 * y + rng.random(y.shape)).astype(np.float32)   # separates the labels; ``s`` overlaps heavily
    res = metrics.bootstrap_compare(better, s, y, **kw)
    for k in KEYS:
        assert (res[k]["delta_low"] > 0).all() and res["macro"][k]["delta_low"] > 0
        assert (res[k]["delta_point"] > 0).all() and (res[k]["delta_high"] >= res[k]["delta_low"]).all()
        assert np.allclose(res[k]["p"], 1.0 / res[k]["n_defined"]) and res["macro"][k]["p"] == 1.0 / 38
    back = metrics.bootstrap_compare(s, better, y, **kw)
    assert all(np.array_equal(back[k]["delta_point"], -res[k]["delta_point"]) and (back[k]["delta_high"] < 0).all() for k in KEYS)


# ---------------------------------------------------------------------------------------------- evaluate_report: off means off
def read_tree(path):
    return {name: open(os.path.join(path, name), "rb").read() for name in sorted(os.listdir(path))}


@pytest.fixture
def host_kernels(monkeypatch):
    """The three device entry points of the report replaced by their numpy restatements (the report itself takes no kernel)."""
    from octcubem_amd import ops
    as_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)   # noqa: E731
    counts = lambda s, l, v=None: torch.from_numpy(multitask_ref.rank_counts(as_np(s), as_np(l), None if v is None else as_np(v)))   # noqa: E731
    monkeypatch.setattr(ops, "rank_counts", counts)
    monkeypatch.setattr(metrics, "_device_rank_counts", counts)
    monkeypatch.setattr(metrics, "_device_rank_counts_masked", counts)
    monkeypatch.setattr(metrics, "_device_bootstrap", lambda s, l, m, u=None, v=None: B.rank_metrics(s, l, m, u, v))


@pytest.mark.parametrize("task_mode", ("multi_cls", "multi_label"))
def test_report_off_means_off_and_on_adds_one_file(task_mode, tmp_path, host_kernels):
    multi_label = task_mode == "multi_label"
    loader, model, _ = B.stub_problem(multi_label)
    crit = torch.nn.BCEWithLogitsLoss() if multi_label else torch.nn.CrossEntropyLoss()
    names = ["amd", "dme", "normal"]

    def run(where, args, epoch=4):
        os.makedirs(where, exist_ok=True)
        return engine_finetune.evaluate_report(loader, model, "cpu", where, epoch, "test", 3, criterion=crit, task_mode=task_mode,
                                               disease_list=names, return_bal_acc=True, args=args)

    ret_none = run(str(tmp_path / "none"), None)
    plain = read_tree(str(tmp_path / "none"))
    assert plain and not any(name.startswith("metrics_ci") for name in plain)
    for tag, args in (("absent", types.SimpleNamespace()), ("zero", types.SimpleNamespace(bootstrap=0)),
                      ("unset", types.SimpleNamespace(bootstrap=None, bootstrap_seed=3))):
        assert run(str(tmp_path / tag), args) == ret_none
        assert read_tree(str(tmp_path / tag)) == plain, tag
    groups = [f"p{i // 2}" for i in range(48)]
    on = types.SimpleNamespace(bootstrap=8, bootstrap_seed=2, bootstrap_alpha=0.2, bootstrap_groups=groups)
    assert run(str(tmp_path / "on"), on) == ret_none
    tree = read_tree(str(tmp_path / "on"))
    assert set(tree) == set(plain) | {"metrics_ci_test.csv"} and all(tree[k] == plain[k] for k in plain)
    rows = list(csv.reader(tree["metrics_ci_test.csv"].decode("utf8").splitlines()))
    assert rows[0] == engine_finetune.CI_HEADER == ["epoch", "metric", "class", "point", "low", "high", "n_defined", "resamples", "alpha",
                                                   "seed", "level"]
    assert [(r[1], r[2]) for r in rows[1:]] == [(k, c) for k in KEYS for c in ["macro"] + names]
    assert all(r[0] == "4" and r[6:] == ["8", "8", "0.2", "2", "group"] for r in rows[1:])
    # the rows are those of the direct call on the scores the report ranks
    with torch.no_grad():
        logits = torch.cat([model(b[0]) for b in loader]).float()
    targets = torch.cat([b[1] for b in loader])
    scores = torch.sigmoid(logits) if multi_label else torch.softmax(logits, dim=1)
    labels = targets != 0 if multi_label else torch.nn.functional.one_hot(targets.long(), 3)
    want = metrics.bootstrap_rank_metrics(scores, labels, resamples=8, seed=2, alpha=0.2, groups=groups)
    for r in rows[1:]:
        part = want["macro"][r[1]] if r[2] == "macro" else {k: v[names.index(r[2])] for k, v in want[r[1]].items() if k != "samples"}
        assert [float(r[3]), float(r[4]), float(r[5])] == [float(part["point"]), float(part["low"]), float(part["high"])]
        assert float(r[4]) <= float(r[5])
    run(str(tmp_path / "on"), on, epoch=5)                      # a second call appends, one header
    again = list(csv.reader(open(tmp_path / "on" / "metrics_ci_test.csv", newline="", encoding="utf8")))
    assert len(again) == 1 + 2 * 16 and again[:17] == rows and again[17][0] == "5"


@pytest.mark.parametrize("mode", ("regression", "multi_task_default", "multi_task"))
def test_unwired_modes_refuse_the_bootstrap_and_name_the_mode(mode, tmp_path):
    with pytest.raises(NotImplementedError, match=f"bootstrap.*{mode}"):
        engine_finetune.evaluate_task_report([], None, "cpu", str(tmp_path), 0, "val", 2, task_mode=mode, args=types.SimpleNamespace(bootstrap=10))


# ---------------------------------------------------------------------------------------------- the entry point
def test_abi_declares_the_bootstrap_kernel():
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"^int octmae_bootstrap_rank_metrics\(", header, re.M)
    assert len(_lib.SIGNATURES["octmae_bootstrap_rank_metrics"]) == 14
    assert _lib.expected_abi_version() >= 33 and re.search(r"^ \* 33: octmae_bootstrap_rank_metrics", header, re.M)
    mk = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bbootstrap\.hip\b", mk, re.M)
    block, chunk, staged = B.kernel_constants()
    assert block % 64 == 0 and chunk % block == 0 and staged * 4 <= 48 * 1024
    for name in ("liboctmae.so", "liboctmae_f16.so"):
        lib = ctypes.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), name))
        assert hasattr(lib, "octmae_bootstrap_rank_metrics") and lib.octmae_abi_version() == _lib.expected_abi_version(), name


def test_the_launcher_refuses_before_any_launch():
    """-2 for every refusal of the header, checked without a GPU: the launcher returns before it touches the device."""
    fn = getattr(_lib.load(), "octmae_bootstrap_rank_metrics")
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    ok = dict(n=4, C=1, R=1, U=4)

    def rc(ptrs=(p,) * 9, **kw):
        a = dict(ok, **kw)
        return fn(*ptrs, a["n"], a["C"], a["R"], a["U"], None)

    for k in range(9):
        assert rc(ptrs=tuple(None if i == k else p for i in range(9))) == -2, k
    for kw in (dict(n=0), dict(C=0), dict(R=0), dict(U=0), dict(n=-1), dict(n=2 ** 31), dict(C=65536), dict(R=2 ** 24), dict(U=2 ** 31)):
        assert rc(**kw) == -2, kw
