"""GPU tests of the two kernels of csrc/bootmoments.hip through ops.bootstrap_moments (and, where F itself is the input, through the
C entry point): EQUAL to int64 numpy on integer data at every edge of the walk -- the 16 rows of a wave, the rows of a workgroup, the 4
units of a k-step, the tiles of a wave and the units of a part, all read out of the source --, the operand layout on one-hot
multiplicities, the derived bounds of tests/bootmoments_ref.py on real data at an offset of 1000, the literal zeros beside NaN-filled
buffers, the fixed order, the refusals, the host finish above it and coem_finetune.evaluate end to end on a stub model."""
import csv
import types

import numpy as np
import pytest
import torch

from tests import bootmoments_ref as B

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS, TILES, SPLIT, WAVES = B.kernel_constants()
RS = (1, 15, 16, 17, 33)
# 1 .. 5: around a k-step; 63 .. 65, 257: ragged and whole walks; one unit either side of the kernel's split points (two and three parts)
US = (1, 3, 4, 5, 63, 64, 65, 257, SPLIT - 1, SPLIT, SPLIT + 1, 2 * SPLIT - 1, 2 * SPLIT, 2 * SPLIT + 1)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def integer_case(R, U, C, seed, grouped=False):
    """Integer-valued float32 inputs, an integer centre, one multiplicity of 2^20 and an all-zero row: every term is below 2^10 and
    every row of mult sums to less than 2^21 + 2^13, so every partial sum stays below 2^32 and float64 is exact."""
    rng = np.random.default_rng([R, U, C, seed])
    n = U if not grouped else 2 * U + 3
    x = rng.integers(-8, 9, (n, C)).astype(np.float32)
    y = rng.integers(-8, 9, (n, C)).astype(np.float32)
    centre = rng.integers(-3, 4, (2, C)).astype(np.float64)
    unit = rng.integers(0, U, n) if grouped else None
    mult = rng.integers(0, 4, (R, U)).astype(np.int32)
    mult[0, rng.integers(0, U)] = 2 ** 20
    if R > 1:
        mult[R - 1] = 0
    return x, y, centre, unit, mult


def integer_moments(x, y, centre, unit, U):
    a, b, e = x.astype(np.int64) - centre[0].astype(np.int64), y.astype(np.int64) - centre[1].astype(np.int64), y.astype(np.int64) - x.astype(np.int64)
    terms = np.stack([np.ones_like(a), a, b, a * a, b * b, a * b, e * e, np.abs(e)], axis=2)      # [n, C, 8]
    F = np.zeros((U,) + terms.shape[1:], dtype=np.int64)
    np.add.at(F, np.arange(x.shape[0]) if unit is None else unit, terms)
    return F


def run(x, y, mult, unit=None, valid=None, centre=None):
    from octcubem_amd import ops
    out = ops.bootstrap_moments(x if isinstance(x, torch.Tensor) else dev(x), y if isinstance(y, torch.Tensor) else dev(y), dev(mult),
                                None if unit is None else dev(unit), None if valid is None else (valid if isinstance(valid, torch.Tensor) else dev(valid)),
                                None if centre is None else dev(centre))
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_exact(R, U, C, seed, grouped=False):
    x, y, centre, unit, mult = integer_case(R, U, C, seed, grouped)
    got = run(x, y, mult, unit, None, centre)
    F = integer_moments(x, y, centre, unit, U)
    assert got["unit_moments"].dtype == np.float64 and got["unit_moments"].shape == (U, C, 8)
    assert np.array_equal(got["unit_moments"], F.astype(np.float64)), (R, U, C)
    want = (mult.astype(np.int64) @ F.reshape(U, -1)).reshape(R, C, 8)
    assert got["moments"].dtype == np.float64 and np.array_equal(got["moments"], want.astype(np.float64)), (R, U, C)
    assert np.array_equal(got["centre"], centre)


@pytest.mark.parametrize("C", (1, 2, 3, 5))
def test_exact_on_integers_at_every_edge(C):
    """C = 2 fills one tile exactly, C = 1 and 3 leave a ragged tile with eight pad columns, C = 5 is three tiles."""
    for R in RS:
        for U in US:
            check_exact(R, U, C, 0)


def test_exact_past_a_workgroup_and_past_a_wave_of_tiles():
    """More rows than the waves of one workgroup own, more tiles than one wave owns (a second grid row), and clustered units."""
    block_rows = ROWS * WAVES
    for R in (block_rows - 1, block_rows, block_rows + 1):
        check_exact(R, 65, 3, 1)
    for C in (2 * TILES, 2 * TILES + 1):                         # TILES tiles exactly; one more: a wave with a single, ragged tile
        for U in (5, SPLIT + 1):
            check_exact(17, U, C, 2)
    for U in (1, 5, 65, SPLIT + 1):
        check_exact(17, U, 3, 3, grouped=True)


def raw_product(mult, Fpad, C, guard=0):
    """octmae_bootstrap_moments on a padded F as it lies in memory; with ``guard`` the operands sit inside NaN- (or garbage-) filled
    buffers, ``guard`` elements on either side, and the guards are checked afterwards."""
    from octcubem_amd import _lib, ops
    R, U = mult.shape
    width = Fpad.shape[1]
    m = torch.full((R * U + 2 * guard,), -2 ** 30, dtype=torch.int32, device=DEV)
    f = torch.full((U * width + 2 * guard,), float("nan"), dtype=torch.float64, device=DEV)
    d = torch.full((R * width + 2 * guard,), float("nan"), dtype=torch.float64, device=DEV)
    m[guard:guard + R * U] = dev(mult).reshape(-1)
    f[guard:guard + U * width] = dev(Fpad).reshape(-1)
    nws = int(_lib.load().octmae_bootstrap_moments_ws(R, U, C))
    ws = torch.full((max(nws, 1) + 2 * guard,), float("nan"), dtype=torch.float64, device=DEV)
    _lib.call("octmae_bootstrap_moments", m[guard:].data_ptr(), f[guard:].data_ptr(), d[guard:].data_ptr(), ws[guard:].data_ptr(), R, U, C,
              ops._stream())
    torch.cuda.synchronize()
    if guard:
        assert torch.isnan(d[:guard]).all() and torch.isnan(d[guard + R * width:]).all()
        assert torch.isnan(ws[:guard]).all() and torch.isnan(ws[guard + nws:]).all()
    return d[guard:guard + R * width].reshape(R, width).cpu().numpy()


@pytest.mark.parametrize("C", (2, 3))
def test_layout_one_hot_rows_select_rows_of_F(C):
    rng = np.random.default_rng(C)
    for U in (37, SPLIT + 9):
        R = 33
        F = rng.permutation(U * 8 * C).reshape(U, 8 * C).astype(np.float64) + 1.0      # distinct integers
        Fpad = np.zeros((U, B.cpad8(C)))
        Fpad[:, :8 * C] = F
        pick = rng.integers(0, U, R)
        pick[:3] = (0, U - 1, min(U - 1, SPLIT))
        mult = np.zeros((R, U), dtype=np.int32)
        mult[np.arange(R), pick] = 1
        D = raw_product(mult, Fpad, C)
        assert np.array_equal(D[:, :8 * C], F[pick]) and (D[:, 8 * C:] == 0).all()


def bounded_case():
    rng = np.random.default_rng(41)
    U, C = 41, 3
    sizes = 1 + np.arange(U) % 7                                 # clusters of 1 .. 7 samples ...
    sizes[17] = 0                                                # ... and a unit without one
    unit = rng.permutation(np.repeat(np.arange(U), sizes))
    n = unit.size
    y = (1000.0 + rng.normal(size=(n, C))).astype(np.float32)
    x = (y + 0.5 * rng.normal(size=(n, C))).astype(np.float32)
    valid = rng.integers(0, 4, (n, C)) > 0
    mult = np.stack([np.bincount(rng.integers(0, U, U), minlength=U) for _ in range(33)]).astype(np.int32)
    return x, y, unit, valid, mult, int(sizes.max())


def test_bounded_on_real_data_with_clusters_masks_and_slices():
    x, y, unit, valid, mult, s_max = bounded_case()
    n, C = x.shape
    U = mult.shape[1]
    wide_x = torch.full((n, C + 4), float("nan"), device=DEV)
    wide_y = torch.full((n, C + 2), float("nan"), device=DEV)
    wide_v = torch.ones((n, C + 3), dtype=torch.uint8, device=DEV)
    wide_x[:, 2:2 + C], wide_y[:, 1:1 + C], wide_v[:, :C] = dev(x), dev(y), dev(valid.astype(np.uint8))
    for val, dval in ((None, None), (valid, wide_v[:, :C])):
        got = run(wide_x[:, 2:2 + C], wide_y[:, 1:1 + C], mult, unit, dval)
        centre = got["centre"]
        ref = B.column_means(x, y, val)
        assert (np.abs(centre - ref) <= (n + 2) * B.U53 * np.abs(ref)).all()                  # a float64 sum of n terms of one sign
        assert B.unit_mismatches(got["unit_moments"], x, y, U, unit, val, centre) == []
        assert (got["unit_moments"][17] == 0).all()
        assert B.product_mismatches(got["moments"], mult, got["unit_moments"]) == []
        # end to end: the finish of the kernel's sums against the finish of the exact sums
        exact = B.exact_moments(x, y, mult, unit, val, centre)
        bound = B.finish_bound(exact, centre, s_max, U)
        mine, want = B.finish(got["moments"], centre, n), B.finish(exact, centre, n)
        for k in B.KEYS:
            assert np.isfinite(bound[k]).all() and np.array_equal(np.isnan(mine[k]), np.isnan(want[k])) and not np.isnan(want[k]).any(), k
            assert (np.abs(mine[k] - want[k]) <= bound[k]).all(), (k, float(np.abs(mine[k] - want[k]).max()), float(bound[k].min()))


def test_nan_guard_literal_zeros_beside_nan_filled_buffers():
    """Rows past R, units past U and the pad columns enter as zeros: NaN beside every operand (and IN the pad columns of F) changes
    nothing, bit for bit, and nothing is written beside the outputs."""
    rng = np.random.default_rng(8)
    for C, U in ((1, 7), (3, SPLIT + 3)):
        R = 17
        F = rng.normal(size=(U, 8 * C)) + 1000.0
        mult = np.stack([np.bincount(rng.integers(0, U, U), minlength=U) for _ in range(R)]).astype(np.int32)
        clean = np.zeros((U, B.cpad8(C)))
        clean[:, :8 * C] = F
        dirty = np.full((U, B.cpad8(C)), np.nan)
        dirty[:, :8 * C] = F
        a, b = raw_product(mult, clean, C), raw_product(mult, dirty, C, guard=4096)
        assert np.isfinite(a).all() and np.array_equal(a, b)
    # through the op: views into NaN-filled buffers, a NaN at an invalid position
    x, y, unit, valid, mult, _ = bounded_case()
    n, C = x.shape
    centre = np.full((2, C), 1000.0)
    clean = run(x, y, mult, unit, valid, centre)
    wide_x = torch.full((n + 2, C + 2), float("nan"), device=DEV)
    wide_y = torch.full((n + 2, C + 2), float("nan"), device=DEV)
    wide_x[1:n + 1, 1:C + 1], wide_y[1:n + 1, 1:C + 1] = dev(np.where(valid, x, np.nan)), dev(np.where(valid, y, np.inf))
    dirty = run(wide_x[1:n + 1, 1:C + 1], wide_y[1:n + 1, 1:C + 1], mult, unit, valid, centre)
    for k in ("moments", "unit_moments", "centre"):
        assert np.isfinite(dirty[k]).all() and np.array_equal(clean[k], dirty[k]), k


def test_fixed_order_same_bits_and_rows_independent_of_R():
    rng = np.random.default_rng(12)
    n, C, R = 2 * SPLIT + 77, 3, 33                              # three parts: the fold is in the path
    y = (1000.0 + rng.normal(size=(n, C))).astype(np.float32)
    x = (y + rng.normal(size=(n, C))).astype(np.float32)
    mult = np.stack([np.bincount(rng.integers(0, n, n), minlength=n) for _ in range(R)]).astype(np.int32)
    a, b = run(x, y, mult), run(x, y, mult)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    centre = a["centre"]
    for r in (0, 5, 16, 32):
        one = run(x, y, mult[r:r + 1], centre=centre)
        assert np.array_equal(one["moments"][0], a["moments"][r]), r
    part = run(x, y, mult[:17], centre=centre)
    assert np.array_equal(part["moments"], a["moments"][:17])


def test_refusals_before_any_launch():
    from octcubem_amd import ops
    x, y, unit, valid, mult, _ = bounded_case()
    tx, ty, tm, tu, tv = dev(x), dev(y), dev(mult), dev(unit), dev(valid.astype(np.uint8))
    ok = ops.bootstrap_moments(tx, ty, tm, tu, tv)
    assert ok["moments"].is_cuda and ok["moments"].shape == (33, 3, 8) and ok["centre"].shape == (2, 3) and ok["unit_moments"].shape == (41, 3, 8)
    bad = tu.clone()
    bad[3] = 41
    with pytest.raises(ValueError, match="unit ids"):
        ops.bootstrap_moments(tx, ty, tm, bad, tv)
    bad[3] = -1
    with pytest.raises(ValueError, match="unit ids"):
        ops.bootstrap_moments(tx, ty, tm, bad, tv)
    neg = tm.clone()
    neg[2, 5] = -1
    with pytest.raises(ValueError, match="negative"):
        ops.bootstrap_moments(tx, ty, neg, tu, tv)
    i, j = (int(v) for v in np.argwhere(valid)[0])
    for value in (float("nan"), float("inf")):
        for which in (0, 1):
            planted = [tx.clone(), ty.clone()]
            planted[which][i, j] = value
            with pytest.raises(ValueError, match="not finite"):
                ops.bootstrap_moments(planted[0], planted[1], tm, tu, tv)
    i, j = (int(v) for v in np.argwhere(~valid)[0])
    planted = tx.clone()
    planted[i, j] = float("nan")                                 # at an invalid position: legal
    assert torch.equal(ops.bootstrap_moments(planted, ty, tm, tu, tv, ok["centre"])["moments"], ok["moments"])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.bootstrap_moments(tx.cpu(), ty, tm, tu, tv)
    with pytest.raises(TypeError, match="float32"):
        ops.bootstrap_moments(tx.double(), ty, tm, tu, tv)
    with pytest.raises(TypeError, match="int32"):
        ops.bootstrap_moments(tx, ty, tm.long(), tu, tv)
    with pytest.raises(TypeError, match="centre"):
        ops.bootstrap_moments(tx, ty, tm, tu, tv, ok["centre"].float())
    with pytest.raises(ValueError, match="mult"):
        ops.bootstrap_moments(tx, ty, tm)                        # without unit, U must be n
    with pytest.raises(ValueError, match="stride"):
        ops.bootstrap_moments(tx.t().contiguous().t(), ty, tm, tu, tv)
    with pytest.raises(ValueError, match="centre"):
        ops.bootstrap_moments(tx, ty, tm, tu, tv, ok["centre"][:, :2].contiguous())
    for value in (float("nan"), float("inf")):
        planted = ok["centre"].clone()
        planted[1, 2] = value
        with pytest.raises(ValueError, match="centre is not finite"):
            ops.bootstrap_moments(tx, ty, tm, tu, tv, planted)


def test_host_finish_on_the_device_against_the_helper():
    from octcubem_amd import metrics, ops
    x, y, unit, valid, mult, s_max = bounded_case()
    n, C = x.shape
    groups = [f"patient-{g}" for g in unit]
    unit, U = metrics._dense_ids(groups)                         # ids in order of first occurrence; the empty unit of the case is gone
    assert U == mult.shape[1] - 1
    mult = mult[:, :U].copy()
    mult[4] = 0
    mult[4, 9] = U                                               # one unit drawn U times, and one valid sample in it: a single point
    keep = valid.copy()
    keep[unit == 9] = False
    keep[np.nonzero(unit == 9)[0][0]] = True
    tx, ty, tv = dev(x), dev(y), dev(keep.astype(np.uint8))
    centre = ops.bootstrap_moments(tx, ty, dev(mult), dev(unit), tv)["centre"].cpu().numpy()
    got = metrics.bootstrap_regression_measures(tx, ty, mult=dev(mult), groups=groups, valid=tv)
    ref = metrics.bootstrap_regression_measures(x, y, mult=mult, groups=groups, valid=keep,
                                                kernel=lambda p, t, m, u=None, v=None, c=None: B.moments(p, t, m, u, v, centre))
    exact = B.exact_moments(x, y, mult, unit, keep, centre)
    bound = B.finish_bound(exact, centre, s_max, U)
    want = B.finish(exact, centre, max(n, U))
    assert got["level"] == ref["level"] == "group" and got["resamples"] == 33
    for k in B.KEYS:
        assert np.array_equal(got[k]["n_defined"], ref[k]["n_defined"]), k
        assert list(got[k]["n_defined"]) == ([33] * C if k in ("mse", "mae") else [32] * C), k
        assert np.array_equal(np.isnan(got[k]["samples"]), np.isnan(want[k])), k
        live = ~np.isnan(want[k])
        assert (np.abs(got[k]["samples"] - want[k])[live] <= bound[k][live]).all(), k
        assert (np.abs(ref[k]["samples"] - want[k])[live] <= bound[k][live]).all(), k
        # a quantile moves by no more than the largest move of a sample
        reach = 2 * np.where(live, bound[k], 0).max(axis=0)
        assert (np.abs(got[k]["low"] - ref[k]["low"]) <= reach).all() and (np.abs(got[k]["high"] - ref[k]["high"]) <= reach).all(), k
        assert np.array_equal(got[k]["point"], ref[k]["point"])


def test_coem_evaluate_end_to_end_on_a_stub_model():
    from octcubem_amd import coem_finetune, metrics
    data, model, args = B.coem_stub(device=DEV)
    plain = coem_finetune.evaluate(model, data, 1, args)
    groups = [f"p{i // 2}" for i in range(48)]
    on = coem_finetune.evaluate(model, data, 1, types.SimpleNamespace(**dict(vars(args), bootstrap=64, bootstrap_seed=5, bootstrap_groups=groups)))
    assert all(on[k] == plain[k] for k in plain) and len(on) == len(plain) + 3 * 9
    with torch.no_grad():
        logits = torch.cat([model(b[0]["oct"].to(DEV), b[0]["ir"].to(DEV))[0] for b in data.dataloader]).float()
    labels = torch.cat([b[0]["label"] for b in data.dataloader]).to(DEV)
    want = metrics.bootstrap_regression_measures(logits, labels, resamples=64, seed=5, groups=groups)
    for j in range(3):
        for name, key in (("pearsonr", "pearsonr"), ("r2", "R2"), ("mse", "mse"), ("mae", "mae")):
            low, high = on[f"{name}_{j}_low"], on[f"{name}_{j}_high"]
            assert (low, high) == (float(want[key]["low"][j]), float(want[key]["high"][j])) and low < high
            assert low - (high - low) <= plain[f"{name}_{j}"] <= high + (high - low)        # the point lies at the interval, not far off
        assert on[f"bootstrap_n_defined_{j}"] == 64


def read_rows(path):
    return list(csv.reader(open(path, newline="", encoding="utf8")))


def test_task_report_takes_the_host_tensors_that_evaluate_returns(tmp_path):
    """engine_finetune.evaluate returns ``logits`` and ``targets`` on the host; bootstrap_task_report moves them to the device.  Both
    modes, no kernel replaced: the rows equal the direct metrics calls on device tensors."""
    from octcubem_amd import engine_finetune, metrics
    rng = np.random.default_rng(23)
    n = 90
    groups = [f"p{i // 3}" for i in range(n)]
    on = types.SimpleNamespace(bootstrap=32, bootstrap_seed=4, bootstrap_alpha=0.1, bootstrap_groups=groups)
    # regression: [n, 1] outputs and targets on the host, as the loop collects them; once as tensors, once as numpy arrays
    y = (50.0 + 10.0 * rng.normal(size=(n, 1))).astype(np.float32)
    x = (y + 4.0 * rng.normal(size=(n, 1))).astype(np.float32)
    res = engine_finetune.bootstrap_task_report(str(tmp_path / "reg"), 3, "test", torch.from_numpy(x), torch.from_numpy(y), "regression", args=on)
    engine_finetune.bootstrap_task_report(str(tmp_path / "reg_np"), 3, "test", x, y, "regression", args=on)
    rows = read_rows(tmp_path / "reg" / "metrics_ci_test.csv")
    assert rows == read_rows(tmp_path / "reg_np" / "metrics_ci_test.csv") and rows[0] == engine_finetune.CI_HEADER
    want = metrics.bootstrap_regression_measures(dev(x[:, 0]), dev(y[:, 0]), resamples=32, seed=4, alpha=0.1, groups=groups)
    assert [(r[1], r[2]) for r in rows[1:]] == [(k, "target") for k in B.KEYS] and res["level"] == "group"
    for r in rows[1:]:
        assert [float(r[3]), float(r[4]), float(r[5]), int(r[6])] == [float(want[r[1]][e][0]) for e in ("point", "low", "high")] + [32]
        assert r[0] == "3" and r[7:] == ["32", "0.1", "4", "group"] and float(r[4]) < float(r[5])
    # multi-task: targets [n, T + 1] and logits [n, 2 T] on the host
    T = 2
    kind = np.arange(n) % 3
    targets = np.zeros((n, T + 1), dtype=np.float32)
    targets[np.arange(n), kind] = 1
    logits = rng.normal(size=(n, 2 * T)).astype(np.float32)
    logits[:, 1::2] += 1.5 * targets[:, 1:]
    names = ["normal", "amd", "dme"]
    engine_finetune.bootstrap_task_report(str(tmp_path / "mt"), 3, "test", torch.from_numpy(logits), torch.from_numpy(targets),
                                          "multi_task_default", disease_list=names, args=on)
    rows = read_rows(tmp_path / "mt" / "metrics_ci_test.csv")
    assert [(r[1], r[2]) for r in rows[1:]] == [(k, c) for k in metrics.RANK_KEYS for c in ["macro", "amd", "dme"]]
    s, l, v = metrics.multi_task_problem(dev(targets), dev(logits), "multi_task_default")
    direct = metrics.bootstrap_rank_metrics(s, l, resamples=32, seed=4, alpha=0.1, groups=groups, valid=v)
    point = metrics.misc_measures_multi_task(dev(targets), dev(logits), multi_task_type="multi_task_default")
    for r in rows[1:]:
        samples = direct[r[1]]["samples"].reshape(32, T, 2).mean(axis=2)
        col = samples.mean(axis=1) if r[2] == "macro" else samples[:, names.index(r[2]) - 1]
        col = col[~np.isnan(col)]
        assert int(r[6]) == col.size and float(r[4]) == np.quantile(col, 0.05) and float(r[5]) == np.quantile(col, 0.95)
        want = point["macro"][r[1]] if r[2] == "macro" else point["classwise"][r[1]][names.index(r[2]) - 1]
        assert abs(float(r[3]) - want) <= 1e-12 and r[7:] == ["32", "0.1", "4", "group"]
