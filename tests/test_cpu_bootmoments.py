"""CPU tests of the bootstrap intervals of the regression metrics: the numpy / exact-rational restatement of the two kernels
(tests/bootmoments_ref.py) against resamples materialised with np.repeat and sent through metrics.regression_measures, the float64
finish of octcubem_amd.metrics.bootstrap_regression_measures / bootstrap_compare_regression on that restatement, the derived bounds
against three planted mistakes of an MFMA walk, the opt-ins of coem_finetune.evaluate and engine_finetune.bootstrap_task_report, and
the declaration of the entry points.

Bounds: tests/bootmoments_ref.py derives them (UNIT_BOUND, PRODUCT_BOUND, finish_bound); none is measured."""
import csv
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch

from octcubem_amd import _lib, coem_finetune, engine_finetune, metrics
from tests import bootmoments_ref as B
from tests import bootstrap_ref, multitask_ref

KEYS = ("pearsonr", "r2", "explained_variance", "mse", "mae", "R2")


def draws(rng, R, U):
    return np.stack([np.bincount(rng.integers(0, U, U), minlength=U) for _ in range(R)]).astype(np.int32)


def problem(offset=0.0, n=48, C=2, seed=7):
    rng = np.random.default_rng(seed)
    y = (offset + rng.normal(size=(n, C))).astype(np.float32)
    x = (y + 0.5 * rng.normal(size=(n, C))).astype(np.float32)
    return x, y, rng


# ---------------------------------------------------------------------------------------------- the finish against materialised resamples
@pytest.mark.parametrize("offset", (0.0, 1000.0))
def test_finish_of_exact_moments_equals_materialised_resamples(offset):
    """Tolerance: finish_bound (the first-order propagation of the input bounds, which exact inputs stay far inside) plus the error of
    regression_measures itself, a two-pass centred evaluation over m rows: each centred sum is within (m + 4) u relative, a quotient
    of two of them within 2 (m + 4) u + 2 u, times the size of the quotient (1 for the correlation, D6 / Syy for the shares)."""
    x, y, rng = problem(offset)
    n, C = x.shape
    valid = rng.integers(0, 4, (n, C)) > 0
    unit = rng.permutation(np.repeat(np.arange(16), 3))
    for unit_, valid_, U in ((None, None, n), (unit, None, 16), (unit, valid, 16), (None, valid, n)):
        mult = draws(rng, 5, U)
        centre = B.column_means(x, y, valid_)
        D = B.exact_moments(x, y, mult, unit_, valid_, centre)
        got = metrics.finish_regression_moments(D, centre, n)
        mine = B.finish(D, centre, n)
        bound = B.finish_bound(D, centre, 3, U)
        for k in KEYS:
            assert np.allclose(got[k], mine[k], rtol=4 * B.U53, atol=0, equal_nan=True), k
        for r in range(mult.shape[0]):
            for c in range(C):
                xs, ys = B.materialised(x, y, mult[r], unit_, valid_, c)
                want = metrics.regression_measures(xs, ys)
                own = 4.0 * (xs.size + 8) * B.U53
                for k in KEYS:
                    scale = max(1.0, abs(want[k]), abs(1.0 - want["r2"]))
                    assert abs(got[k][r, c] - want[k]) <= bound[k][r, c] + own * scale, (k, r, c, got[k][r, c], want[k])


def test_group_level_equals_sample_level_on_presummed_units():
    x, y, rng = problem(3.0)
    n, C = x.shape
    unit = np.repeat(np.arange(16), 3)                           # contiguous clusters: the sample sums of a unit in their own order
    centre = B.column_means(x, y)
    Fs = B.unit_moments(x, y, n, None, None, centre)
    Fg = B.unit_moments(x, y, 16, unit, None, centre)
    pre = np.zeros_like(Fg)
    for i in range(n):
        pre[unit[i]] += Fs[i]
    assert np.array_equal(pre, Fg)
    mult = draws(rng, 6, 16)
    assert np.array_equal(B.exact_moments(x, y, mult, unit, None, centre), B.exact_moments(x, y, mult[:, unit], None, None, centre))
    a = metrics.bootstrap_regression_measures(x, y, mult=mult, groups=list(unit), kernel=B.moments)
    b = metrics.bootstrap_regression_measures(x, y, mult=mult[:, unit], kernel=B.moments)
    assert a["level"] == "group" and b["level"] == "sample" and a["resamples"] == b["resamples"] == 6
    bound = B.finish_bound(B.exact_moments(x, y, mult, unit, None, centre), centre, 3, n)
    for k in KEYS:
        assert np.array_equal(a[k]["point"], b[k]["point"])
        assert (np.abs(a[k]["samples"] - b[k]["samples"]) <= 2 * bound[k]).all(), k


# ---------------------------------------------------------------------------------------------- the bounds catch a fault
def test_the_bounds_catch_three_planted_faults():
    rows, tiles, split, waves = B.kernel_constants()
    rng = np.random.default_rng(2)
    C, R, U = 3, rows + 1, 11                                    # a ragged tile (24 of 32 columns), two row blocks, a ragged k-step
    F = rng.normal(size=(U, 8 * C)) + 1000.0
    Fpad = np.full((U, B.cpad8(C)), 7.0)                         # the pad is NOT zero: a correct walk never reads it
    Fpad[:, :8 * C] = F
    mult = draws(rng, R, U)
    mult[:, U - 1] += 1                                          # the last k-step weighs something in every row
    good = B.product(mult, Fpad, 8 * C)
    assert B.product_mismatches(good[:, :8 * C], mult, F) == [] and (good[:, 8 * C:] == 0).all()
    for fault in B.FAULTS:
        bad = B.product(mult, Fpad, 8 * C, fault=fault)
        if fault == "pad_multiplied":
            assert B.product_mismatches(bad[:, :8 * C], mult, F) == [] and (bad[:, 8 * C:] != 0).all()
        else:
            assert B.product_mismatches(bad[:, :8 * C], mult, F), f"{fault} went unnoticed"
    # the same split points as the kernel's, shrunk: a part boundary inside the walk
    small = B.product(mult, Fpad, 8 * C, split=4)
    assert B.product_mismatches(small[:, :8 * C], mult, F) == []
    x, y, _ = problem(1000.0, n=U, C=C)
    centre = B.column_means(x, y)
    Fu = B.unit_moments(x, y, U, None, None, centre)
    assert B.unit_mismatches(Fu, x, y, U, None, None, centre) == []
    Fu[3, 1, 5] *= 1.0 + 2.0 ** -40
    assert [b[:3] for b in B.unit_mismatches(Fu, x, y, U, None, None, centre)] == [(3, 1, 5)]
    assert split % 4 == 0 and rows == 16 and tiles >= 1 and waves >= 1


# ---------------------------------------------------------------------------------------------- the host finish
def test_degenerate_resamples_are_counted_not_redrawn():
    x, y, rng = problem(1000.0, C=1)
    n = x.shape[0]
    x[9] = x[5]                                                  # two samples with equal x
    R = 12
    mult = draws(rng, R, n)
    mult[2] = 0
    mult[2, 7] = n                                               # one sample drawn n times
    mult[4] = 0
    mult[4, 5] = mult[4, 9] = n // 2                             # two samples with equal x, at a mean offset of 1000
    mult[6] = 0                                                  # an all-zero row
    res = metrics.bootstrap_regression_measures(x[:, 0], y[:, 0], mult=mult, kernel=B.moments)
    for k in KEYS:
        undefined = {6} if k in ("mse", "mae") else {2, 4, 6}
        assert int(res[k]["n_defined"][0]) == R - len(undefined), k
        assert set(np.nonzero(np.isnan(res[k]["samples"][:, 0]))[0]) == undefined, k
        col = res[k]["samples"][:, 0]
        col = col[~np.isnan(col)]
        assert res[k]["low"][0] == np.quantile(col, 0.025) and res[k]["high"][0] == np.quantile(col, 0.975)
        assert res[k]["point"][0] == metrics.regression_measures(x[:, 0], y[:, 0])[k]
        assert res[k]["samples"].shape == (R, 1) and res[k]["samples"].dtype == np.float64
    assert res["mse"]["samples"][2, 0] == pytest.approx(float(y[7, 0] - x[7, 0]) ** 2, rel=1e-12)
    only = np.zeros((3, n), dtype=np.int32)
    only[np.arange(3), [1, 2, 3]] = n
    with pytest.raises(ValueError, match="column 0.*pearsonr"):
        metrics.bootstrap_regression_measures(x, y, mult=only, kernel=B.moments)
    with pytest.raises(ValueError, match="alpha"):
        metrics.bootstrap_regression_measures(x, y, mult=mult, alpha=0.0, kernel=B.moments)
    with pytest.raises(ValueError, match="mult"):
        metrics.bootstrap_regression_measures(x, y, mult=mult[:, 1:], kernel=B.moments)
    with pytest.raises(TypeError):                               # no kernel and host arrays: there is no CPU path
        metrics.bootstrap_regression_measures(x, y, resamples=4)


def test_random_multiplicities_are_all_defined_and_match_the_draw():
    x, y, _ = problem(0.0, n=48, C=2)
    seen = []

    def kernel(pred, target, mult, unit=None, valid=None, centre=None):
        seen.append(np.asarray(mult))
        return B.moments(pred, target, mult, unit, valid, centre)

    res = metrics.bootstrap_regression_measures(x, y, resamples=64, seed=3, kernel=kernel)
    assert np.array_equal(seen[0], metrics.bootstrap_multiplicities(64, 48, 3, "cpu").numpy())
    assert res["resamples"] == 64 and all(list(res[k]["n_defined"]) == [64, 64] for k in KEYS)
    assert all((res[k]["low"] <= res[k]["high"]).all() for k in KEYS)
    assert np.array_equal(res["R2"]["samples"], res["pearsonr"]["samples"] ** 2)


def test_compare_identical_and_planted():
    x, y, rng = problem(0.0, n=48, C=2)
    mult = draws(rng, 40, 48)
    same = metrics.bootstrap_compare_regression(x, x.copy(), y, mult=mult, kernel=B.moments)
    for k in KEYS:
        part = same[k]
        assert (part["delta_point"] == 0).all() and (part["delta_low"] == 0).all() and (part["delta_high"] == 0).all()
        assert (part["p"] == 1.0).all() and list(part["n_defined"]) == [40, 40]
    better = (y + 0.01 * rng.normal(size=y.shape)).astype(np.float32)      # strictly better in every resample
    res = metrics.bootstrap_compare_regression(better, x, y, mult=mult, kernel=B.moments)
    for k in KEYS:
        sign = -1 if k in ("mse", "mae") else 1
        assert (sign * res[k]["delta_point"] > 0).all() and (sign * res[k]["delta_low"] > 0).all() and (sign * res[k]["delta_high"] > 0).all()
        assert np.array_equal(res[k]["p"], np.full(2, 1.0 / 40))
    assert res["resamples"] == 40 and res["level"] == "sample"


# ---------------------------------------------------------------------------------------------- the opt-ins: off means off
@pytest.fixture
def host_kernels(monkeypatch):
    """The device entry points behind the two reports replaced by their numpy restatements (the reports take no kernel)."""
    as_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)   # noqa: E731
    counts = lambda s, l, v=None: torch.from_numpy(multitask_ref.rank_counts(as_np(s), as_np(l), None if v is None else as_np(v)))   # noqa: E731
    monkeypatch.setattr(metrics, "_device_rank_counts", counts)
    monkeypatch.setattr(metrics, "_device_rank_counts_masked", counts)
    monkeypatch.setattr(metrics, "_device_bootstrap", lambda s, l, m, u=None, v=None: bootstrap_ref.rank_metrics(as_np(s), as_np(l), as_np(m),
                                                                                                               None if u is None else as_np(u),
                                                                                                               None if v is None else as_np(v)))
    monkeypatch.setattr(metrics, "_device_bootmoments", lambda p, t, m, u=None, v=None, c=None: B.moments(p, t, m, u, v, c))


def read_tree(path):
    out = {}
    for root, _, files in os.walk(path):
        for name in files:
            out[os.path.relpath(os.path.join(root, name), path)] = open(os.path.join(root, name), "rb").read()
    return out


def test_coem_evaluate_off_means_off_and_on_adds_the_stated_keys(tmp_path, host_kernels):
    data, model, args = B.coem_stub()

    def run(tag, **kw):
        where = str(tmp_path / tag)
        os.makedirs(where)
        a = types.SimpleNamespace(**dict(vars(args), save_logs=True, checkpoint_path=where, **kw))
        return coem_finetune.evaluate(model, data, 1, a), read_tree(where)

    plain, tree = run("none")
    assert plain["num_samples"] == 48 and tree
    for tag, kw in (("zero", dict(bootstrap=0)), ("unset", dict(bootstrap=None, bootstrap_seed=3))):
        got, t = run(tag, **kw)
        assert got == plain and list(got) == list(plain) and t == tree, tag
    groups = [f"p{i // 2}" for i in range(48)]
    on, t = run("on", bootstrap=16, bootstrap_seed=2, bootstrap_alpha=0.2, bootstrap_groups=groups)
    new = [f"{k}_{j}_{e}" for j in range(3) for k in ("pearsonr", "r2", "mse", "mae") for e in ("low", "high")] + [f"bootstrap_n_defined_{j}" for j in range(3)]
    assert set(on) == set(plain) | set(new) and all(on[k] == plain[k] for k in plain)
    assert set(t) == set(tree) and all(t[k] == tree[k] for k in tree if not k.endswith(".jsonl"))
    assert json.loads(t["results-val-0.jsonl"].decode()) == json.loads(json.dumps(on))
    with torch.no_grad():
        logits = torch.cat([model(b[0]["oct"], b[0]["ir"])[0] for b in data.dataloader]).float()
    labels = torch.cat([b[0]["label"] for b in data.dataloader])
    want = metrics.bootstrap_regression_measures(logits, labels, resamples=16, seed=2, alpha=0.2, groups=groups)
    for j in range(3):
        for name, key in (("pearsonr", "pearsonr"), ("r2", "R2"), ("mse", "mse"), ("mae", "mae")):
            assert on[f"{name}_{j}_low"] == want[key]["low"][j] and on[f"{name}_{j}_high"] == want[key]["high"][j]
            assert on[f"{name}_{j}_low"] <= on[f"{name}_{j}_high"]
        assert on[f"bootstrap_n_defined_{j}"] == 16
    # a column without a point correlation: NaN bounds, nothing raised, the other columns as before
    data1, model1, args1 = B.coem_stub(constant_column=1)
    flat = coem_finetune.evaluate(model1, data1, 1, types.SimpleNamespace(**dict(vars(args1), bootstrap=16, bootstrap_seed=2)))
    assert np.isnan(flat["pearsonr_1"]) and all(np.isnan(flat[f"{k}_1_{e}"]) for k in ("pearsonr", "r2", "mse", "mae") for e in ("low", "high"))
    assert flat["bootstrap_n_defined_1"] == 0 and flat["bootstrap_n_defined_0"] == 16 and flat["pearsonr_0_low"] <= flat["pearsonr_0_high"]


def test_task_report_regression_rows(tmp_path, host_kernels):
    x, y, _ = problem(2.0, n=48, C=2)
    logits, targets = torch.from_numpy(x), torch.from_numpy(y)
    for args in (None, types.SimpleNamespace(), types.SimpleNamespace(bootstrap=0), types.SimpleNamespace(bootstrap=None)):
        assert engine_finetune.bootstrap_task_report(str(tmp_path / "off"), 1, "val", logits, targets, "regression", args=args) is None
    assert not os.path.exists(tmp_path / "off")
    on = types.SimpleNamespace(bootstrap=8, bootstrap_seed=2, bootstrap_alpha=0.2, device="cpu")
    engine_finetune.bootstrap_task_report(str(tmp_path / "on"), 4, "val", logits, targets, "regression", args=on)
    assert sorted(os.listdir(tmp_path / "on")) == ["metrics_ci_val.csv"]
    rows = list(csv.reader(open(tmp_path / "on" / "metrics_ci_val.csv", newline="", encoding="utf8")))
    assert rows[0] == engine_finetune.CI_HEADER
    assert [(r[1], r[2]) for r in rows[1:]] == [(k, "target") for k in KEYS]
    assert all(r[0] == "4" and r[6:] == ["8", "8", "0.2", "2", "sample"] for r in rows[1:])
    want = metrics.bootstrap_regression_measures(x[:, 0], y[:, 0], resamples=8, seed=2, alpha=0.2, kernel=B.moments)
    for r in rows[1:]:
        assert [float(r[3]), float(r[4]), float(r[5])] == [float(want[r[1]][e][0]) for e in ("point", "low", "high")]
    engine_finetune.bootstrap_task_report(str(tmp_path / "on"), 5, "val", logits, targets, "regression", args=on)
    again = list(csv.reader(open(tmp_path / "on" / "metrics_ci_val.csv", newline="", encoding="utf8")))
    assert len(again) == 1 + 2 * 6 and again[:7] == rows and again[7][0] == "5"
    with pytest.raises(ValueError, match="multi_cls"):
        engine_finetune.bootstrap_task_report(str(tmp_path / "on"), 5, "val", logits, targets, "multi_cls", args=on)


@pytest.mark.parametrize("task_mode", ("multi_task_default", "multi_task"))
def test_task_report_multi_task_rows(task_mode, tmp_path, host_kernels):
    rng = np.random.default_rng(9)
    n, T = 60, 2
    kind = np.arange(n) % 3                                      # 0 normal, 1 task 1, 2 task 2: every population holds both labels
    targets = np.zeros((n, T + 1), dtype=np.float32)
    targets[np.arange(n), kind] = 1
    width = 2 * T if task_mode == "multi_task_default" else T + 1
    logits = rng.normal(size=(n, width)).astype(np.float32)
    if task_mode == "multi_task_default":
        logits[:, 1::2] += 1.5 * targets[:, 1:]
    else:
        logits += 1.5 * targets
    lt, tt = torch.from_numpy(logits), torch.from_numpy(targets)
    names = ["normal", "amd", "dme"]
    on = types.SimpleNamespace(bootstrap=8, bootstrap_seed=1, bootstrap_alpha=0.1, bootstrap_groups=[f"p{i // 3}" for i in range(n)], device="cpu")
    assert engine_finetune.bootstrap_task_report(str(tmp_path), 2, "test", lt, tt, task_mode, disease_list=names, args=types.SimpleNamespace()) is None
    res = engine_finetune.bootstrap_task_report(str(tmp_path), 2, "test", lt, tt, task_mode, disease_list=names, args=on)
    rows = list(csv.reader(open(tmp_path / "metrics_ci_test.csv", newline="", encoding="utf8")))
    assert rows[0] == engine_finetune.CI_HEADER
    assert [(r[1], r[2]) for r in rows[1:]] == [(k, c) for k in metrics.RANK_KEYS for c in ["macro", "amd", "dme"]]
    assert all(r[0] == "2" and r[7:] == ["8", "0.1", "1", "group"] for r in rows[1:])
    s, l, v = metrics.multi_task_problem(tt, lt, task_mode)
    direct = metrics.bootstrap_rank_metrics(s, l, resamples=8, seed=1, alpha=0.1, groups=on.bootstrap_groups, valid=v)
    point = metrics.misc_measures_multi_task(tt, lt, multi_task_type=task_mode)
    for r in rows[1:]:
        samples = direct[r[1]]["samples"].reshape(8, T, 2).mean(axis=2)
        col = samples.mean(axis=1) if r[2] == "macro" else samples[:, names.index(r[2]) - 1]
        col = col[~np.isnan(col)]
        assert int(r[6]) == col.size and float(r[4]) == np.quantile(col, 0.05) and float(r[5]) == np.quantile(col, 0.95)
        want = point["macro"][r[1]] if r[2] == "macro" else point["classwise"][r[1]][names.index(r[2]) - 1]
        assert abs(float(r[3]) - want) <= 1e-12
    assert set(res["tasks"]) == set(metrics.RANK_KEYS)
    with pytest.raises(NotImplementedError):                     # the report itself still refuses the switch for these modes
        engine_finetune.evaluate_task_report([], None, "cpu", str(tmp_path), 0, "val", 2, task_mode=task_mode, args=on)


# ---------------------------------------------------------------------------------------------- the entry points
def test_abi_declares_the_moment_kernels():
    header = open(_lib.HEADER_PATH).read()
    for name, nargs in (("octmae_unit_moments", 14), ("octmae_bootstrap_moments", 8), ("octmae_bootstrap_moments_ws", 3)):
        assert re.search(rf"^(?:long long )?int {name}\(", header, re.M), name
        assert len(_lib.SIGNATURES[name]) == nargs
    assert _lib.expected_abi_version() >= 34 and re.search(r"^ \* 34: octmae_unit_moments, octmae_bootstrap_moments", header, re.M)
    mk = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bbootmoments\.hip\b", mk, re.M)
    for name in ("liboctmae.so", "liboctmae_f16.so"):
        lib = ctypes.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), name))
        assert all(hasattr(lib, f) for f in ("octmae_unit_moments", "octmae_bootstrap_moments", "octmae_bootstrap_moments_ws")), name
        assert lib.octmae_abi_version() == _lib.expected_abi_version(), name


def test_the_launchers_refuse_before_any_launch():
    """-2 for every refusal of the header, checked without a GPU: the launchers return before they touch the device."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    max_c, max_r, max_u = B.limits()
    assert (max_c, max_r, max_u) == (4096, 2 ** 20, 2 ** 24)

    def unit(ptrs=None, **kw):
        a = dict(dict(n=4, C=1, U=4, ps=1, ts=1, vs=1), **kw)
        q = dict(dict(pred=p, target=p, valid=p, centre=p, order=p, start=p, F=p), **(ptrs or {}))
        return lib.octmae_unit_moments(q["pred"], a["ps"], q["target"], a["ts"], q["valid"], a["vs"], q["centre"], q["order"], q["start"], q["F"],
                                       a["n"], a["C"], a["U"], None)

    for k in ("pred", "target", "centre", "order", "start", "F"):
        assert unit(ptrs={k: None}) == -2, k
    for kw in (dict(n=0), dict(C=0), dict(U=0), dict(n=-1), dict(n=2 ** 31), dict(C=max_c + 1, ps=max_c + 1, ts=max_c + 1, vs=max_c + 1),
               dict(U=max_u + 1), dict(C=2, ps=1, ts=2, vs=2), dict(C=2, ps=2, ts=1, vs=2), dict(C=2, ps=2, ts=2, vs=1)):
        assert unit(**kw) == -2, kw

    def prod(ptrs=None, **kw):
        a = dict(dict(R=1, U=4, C=1), **kw)
        q = dict(dict(mult=p, F=p, D=p, ws=p), **(ptrs or {}))
        return lib.octmae_bootstrap_moments(q["mult"], q["F"], q["D"], q["ws"], a["R"], a["U"], a["C"], None)

    _, _, split, _ = B.kernel_constants()
    for k in ("mult", "F", "D"):
        assert prod(ptrs={k: None}) == -2, k
    assert prod(ptrs={"ws": None}, U=split + 1) == -2             # more than one part needs the workspace
    # the last two: R * Cpad8 >= 2^32, which the one-thread-per-element fold cannot index (2^20 x 4096 is 2^32 exactly)
    for kw in (dict(R=0), dict(U=0), dict(C=0), dict(R=-1), dict(R=max_r + 1), dict(U=max_u + 1), dict(C=max_c + 1), dict(R=max_r, C=512),
               dict(R=max_r, C=max_c)):
        assert prod(**kw) == -2, kw
        assert lib.octmae_bootstrap_moments_ws(*(dict(dict(R=1, U=4, C=1), **kw)[k] for k in ("R", "U", "C"))) == -2, kw
    assert lib.octmae_bootstrap_moments_ws(1000, split, 5) == 0
    assert lib.octmae_bootstrap_moments_ws(1000, split + 1, 5) == 2 * 1000 * 48
    assert lib.octmae_bootstrap_moments_ws(max_r - 1, max_u, 512) == (max_u // split) * (max_r - 1) * 4096      # doubles, not bytes
