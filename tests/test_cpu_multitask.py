"""CPU tests of the multi-task fine-tune mode: metrics.misc_measures_multi_task, losses.multi_task_targets / multi_task_loss, the
``valid=`` path of metrics.binary_rank_metrics and the declaration of octmae_rank_counts_masked.

``misc_measures_multi_task`` is fed with rank counts from the numpy stand-in (tests/multitask_ref.py) and pinned to
tests/golden/metrics_multitask_small.npz, which tools/gen_golden_multitask.py wrote by calling the reference's own functions with
scikit-learn.  The tolerance is the one tests/test_cpu_metrics.py applies to the multi-label golden: its ``TOL`` = 1e-12, absolute
(a handful of float64 divisions and sums of a few dozen terms of size <= 1 agree to a few ulp, 1e-15).

The loss is compared with the float64 loop of tests/multitask_ref.py.  A float32 sum of k terms carries at most about
k * 2^-24 * sum|term| of rounding error, and each term a few more ulp from its log-softmax: the bound is
(k + 8) * 2^-24 * sum|term|, computed from the float64 terms of the case at hand.  For the value the terms are the per-row losses
as they enter the sum; for an element of the gradient they are the softmax share and the target share of every pair that logit
belongs to (two per pair; they cancel where the model is right, so the bound must not be taken from their difference)."""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest
import torch

from octcubem_amd import _lib, losses, metrics
from tests import multitask_ref as M
from tests.test_cpu_metrics import TOL

assert TOL == 1e-12                                       # the multi-label golden's tolerance, as that file states it
N_GOLDEN = 3
EPS = 2.0 ** -24
MACRO = ("micro_AP", "accuracy", "roc_auc", "precision", "recall", "f1", "max_f1", "AP", "auprc", "balanced_acc", "specificity",
         "sensitivity", "mcc", "G", "kappa")


def golden_problem(k):
    """(y_true int64 [n, T + 1], logits float32, multi_task_type), seeded.  0: 30 samples x 3 tasks in the default layout [n, 2T];
    1: 36 x 4 in the shared-column layout [n, T + 1]; 2: 40 x 2, default layout, logits on a grid of halves in [-1, 1], so that ties
    and scores of exactly 0.5 dominate.  Checked here, so that the reference alone never raises: every task's population holds both
    label values in both columns; a task excludes more than a third of the samples; a sample carries the normal and a task label."""
    n, T, kind = ((30, 3, "multi_task_default"), (36, 4, "multi_task"), (40, 2, "multi_task_default"))[k]
    rng = np.random.default_rng(177 + k)
    y = np.zeros((n, T + 1), dtype=np.int64)
    y[:, 0] = rng.random(n) < 0.25
    y[:, 1:] = rng.random((n, T)) < 0.25
    y[0] = 0
    y[0, 0] = 1                                           # the normal label alone
    for t in range(T):
        y[1 + t] = 0
        y[1 + t, 1 + t] = 1                               # task t alone
    y[T + 1] = 0
    y[T + 1, 0] = y[T + 1, 1] = 1                         # normal and task 0 together
    pop = (y[:, :1] + y[:, 1:]) > 0
    for t in range(T):
        for col in (y[pop[:, t], 0], y[pop[:, t], 1 + t]):
            assert 0 < col.sum() < col.size
    assert (~pop).sum(0).max() * 3 > n and (y[:, 0] * y[:, 1:].sum(1) > 0).any()
    if kind == "multi_task_default":
        centre = np.stack([np.repeat(y[:, :1], T, axis=1), y[:, 1:]], axis=2).reshape(n, 2 * T)
    else:
        centre = y
    logits = 1.4 * (centre - 0.5) + rng.standard_normal(centre.shape)
    if k == 2:
        logits = np.clip(np.round(logits * 2) / 2, -1, 1)
    return y, logits.astype(np.float32), kind


def crc(*arrays):
    return zlib.crc32(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "metrics_multitask_small.npz"))


def test_grid_problem_has_ties_and_exact_halves():
    y, logits, kind = golden_problem(2)
    s, _, v = metrics.multi_task_problem(y, logits, kind)
    assert (s[v != 0] == 0.5).sum() >= 8 and np.unique(s[:, 0]).size <= 9


@pytest.mark.parametrize("k", range(N_GOLDEN))
def test_misc_measures_multi_task_equals_the_reference(k, golden):
    assert str(golden["sklearn_version"]) != "absent"
    y, logits, kind = golden_problem(k)
    assert crc(y, logits) == int(golden[f"crc_{k}"]), "the seeded inputs are not the ones the fixture was made from"
    res = metrics.misc_measures_multi_task(y, logits, threshold=0.5, multi_task_type=kind, rank_counts=M.rank_counts)
    assert tuple(res["macro"]) == MACRO and tuple(res["classwise"]) == MACRO[1:]
    for half in ("macro", "classwise"):
        for key, v in res[half].items():
            np.testing.assert_allclose(np.asarray(v, dtype=np.float64), golden[f"{half}_{k}/{key}"], rtol=0, atol=TOL, err_msg=f"{half} {key}")
    as_tensors = metrics.misc_measures_multi_task(torch.from_numpy(y), torch.from_numpy(logits), multi_task_type=kind, rank_counts=M.rank_counts)
    assert as_tensors == res


def test_multi_task_on_a_host_array_needs_a_counter():
    y, logits, kind = golden_problem(0)
    with pytest.raises(TypeError):
        metrics.misc_measures_multi_task(y, logits, multi_task_type=kind)
    with pytest.raises(RuntimeError):
        metrics.misc_measures_multi_task(torch.from_numpy(y), torch.from_numpy(logits), multi_task_type=kind)


@pytest.mark.parametrize("k", range(N_GOLDEN))
def test_multi_task_targets_equal_the_reference(k, golden):
    y, _, _ = golden_problem(k)
    tm, w = losses.multi_task_targets(torch.from_numpy(y))
    assert tm.dtype == torch.int64 and tuple(tm.shape) == (y.shape[0], y.shape[1] - 1, 2) and tuple(w.shape) == tm.shape[:2]
    assert np.array_equal(tm.numpy(), golden[f"target_mt_{k}"]) and np.array_equal(w.numpy(), golden[f"weight_{k}"])
    tf, wf = losses.multi_task_targets(torch.from_numpy(y).float())
    assert tf.dtype == torch.float32 and torch.equal(tf, tm.float()) and torch.equal(wf, w.float())


def check_loss(y, logits, kind, smoothing=0.1, golden_value=None):
    """multi_task_loss (value and input gradient) against the float64 loop, within the term bound; returns the value."""
    want, terms, grad, grad_abs = M.multi_task_loss(logits, y, smoothing, kind)
    bound = (terms.size + 8) * EPS * float(np.abs(terms).sum())
    x = torch.from_numpy(np.ascontiguousarray(logits)).requires_grad_()
    got = losses.multi_task_loss(x, torch.from_numpy(y), losses.WeightedLabelSmoothingCrossEntropy(smoothing), kind)
    assert got.dtype == torch.float32 and got.dim() == 0
    print(f"{kind}: loss {float(got.detach())!r}, float64 loop {want!r}, difference {abs(float(got.detach()) - want):.3e}, bound {bound:.3e}")
    assert abs(float(got.detach()) - want) <= bound
    if golden_value is not None:                          # the reference's own float32 value: it is within the same bound of the loop
        assert abs(float(got.detach()) - float(golden_value)) <= 2 * bound and abs(float(golden_value) - want) <= bound
    got.backward()
    g, gabs, gk = M.grad_of_layout(grad, grad_abs, kind)
    gbound = (gk + 8) * EPS * gabs
    err = np.abs(x.grad.numpy().astype(np.float64) - g)
    print(f"  gradient: largest difference {err.max():.3e}, its bound {gbound.flat[err.argmax()]:.3e}")
    assert x.grad.shape == x.shape and (err <= gbound).all()
    return float(got.detach())


@pytest.mark.parametrize("k", range(N_GOLDEN))
def test_multi_task_loss_against_the_float64_loop_and_the_reference(k, golden):
    y, logits, kind = golden_problem(k)
    check_loss(y, logits, kind, 0.1, golden[f"loss_{k}"])


@pytest.mark.parametrize("kind", ("multi_task_default", "multi_task"))
def test_multi_task_loss_with_a_task_nobody_belongs_to(kind):
    """Task 1 has no valid row: it adds 0 to the value and zeros -- not None, not NaN -- to its logits' gradient."""
    rng = np.random.default_rng(5)
    y = np.zeros((7, 4), dtype=np.int64)
    y[:4, 1] = 1
    y[2:6, 3] = 1                                         # nobody is normal, nobody has task 1; row 6 has no label at all
    logits = rng.standard_normal((7, 6 if kind == "multi_task_default" else 4)).astype(np.float32)
    check_loss(y, logits, kind)
    x = torch.from_numpy(logits).requires_grad_()
    losses.multi_task_loss(x, torch.from_numpy(y), losses.WeightedLabelSmoothingCrossEntropy(0.1), kind).backward()
    dead = x.grad[:, 2:4] if kind == "multi_task_default" else x.grad[:, 2]
    assert bool((dead == 0).all()) and bool((x.grad[6] == 0).all()) and bool(torch.isfinite(x.grad).all())


@pytest.mark.parametrize("kind", ("multi_task_default", "multi_task"))
def test_multi_task_loss_without_any_valid_row(kind):
    y = torch.zeros(5, 3, dtype=torch.int64)
    x = torch.randn(5, 4 if kind == "multi_task_default" else 3, generator=torch.Generator().manual_seed(1)).requires_grad_()
    loss = losses.multi_task_loss(x, y, losses.WeightedLabelSmoothingCrossEntropy(0.1), kind)
    loss.backward()
    assert float(loss.detach()) == 0.0 and x.grad is not None and bool((x.grad == 0).all())


@pytest.mark.parametrize("k", (0, 1))
def test_other_criteria_keep_the_loop(k):
    """Any other criterion is called once per task on [B, 2] logits and [B, 2] targets; with the weighted criterion subclassed (so that
    the batched pass is not taken) the loop must give the batched value."""
    y, logits, kind = golden_problem(k)
    calls = []

    class Spy(torch.nn.Module):
        def forward(self, out, tgt):
            calls.append((tuple(out.shape), tuple(tgt.shape), tgt.dtype))
            return losses.WeightedLabelSmoothingCrossEntropy(0.1)(out, tgt)

    T = y.shape[1] - 1
    x, t = torch.from_numpy(logits), torch.from_numpy(y)
    looped = losses.multi_task_loss(x, t, Spy(), kind)
    assert calls == [((y.shape[0], 2), (y.shape[0], 2), torch.int64)] * T
    batched = losses.multi_task_loss(x, t, losses.WeightedLabelSmoothingCrossEntropy(0.1), kind)
    _, terms, _, _ = M.multi_task_loss(logits, y, 0.1, kind)
    assert abs(float(looped) - float(batched)) <= 2 * (terms.size + 8) * EPS * float(np.abs(terms).sum())


def test_shape_mismatches_raise():
    y, logits, kind = golden_problem(0)                    # 3 tasks: [30, 6] logits
    crit = losses.WeightedLabelSmoothingCrossEntropy(0.1)
    t, x = torch.from_numpy(y), torch.from_numpy(logits)
    for bad_x, bad_kind in ((x[:, :4], kind), (x, "multi_task"), (x[:5], kind), (x[:, :3], "multi_task")):
        with pytest.raises(ValueError):
            losses.multi_task_loss(bad_x, t, crit, bad_kind)
        with pytest.raises(ValueError):
            metrics.misc_measures_multi_task(y, bad_x.numpy(), multi_task_type=bad_kind, rank_counts=M.rank_counts)
    with pytest.raises(ValueError):
        losses.multi_task_targets(t[:, :1])
    with pytest.raises(ValueError):
        metrics.misc_measures_multi_task(y[:, :1], logits, multi_task_type=kind, rank_counts=M.rank_counts)


def test_one_class_and_empty_populations_raise_and_name_the_task():
    y, logits, kind = golden_problem(0)
    one = y.copy()
    one[one[:, 2] == 1, 0] = 1                            # every task-1 sample is normal too: column 0 of task 1 is all ones
    with pytest.raises(ValueError, match="task 1"):
        metrics.misc_measures_multi_task(one, logits, multi_task_type=kind, rank_counts=M.rank_counts)
    none = y.copy()
    none[:, 0] = 0                                        # no normal sample: every population holds positives only in column 1
    with pytest.raises(ValueError, match="task 0"):
        metrics.misc_measures_multi_task(none, logits, multi_task_type=kind, rank_counts=M.rank_counts)
    only = np.zeros_like(y)
    only[:, 2] = 1
    only[0, 0] = 1                                        # tasks 0 and 2 hold the one normal sample alone
    with pytest.raises(ValueError, match="task 0"):
        metrics.misc_measures_multi_task(only, logits, multi_task_type=kind, rank_counts=M.rank_counts)
    void = np.zeros_like(y)
    with pytest.raises(ValueError, match="task 0.*empty"):
        metrics.misc_measures_multi_task(void, logits, multi_task_type=kind, rank_counts=M.rank_counts)


def test_binary_rank_metrics_with_an_all_ones_mask_is_the_unmasked_call():
    rng = np.random.default_rng(3)
    s = (rng.integers(0, 8, size=(41, 3)) / 8).astype(np.float32)
    lab = rng.integers(0, 2, size=(41, 3)).astype(np.uint8)
    ones = np.ones_like(lab)
    counts = M.rank_counts(s, lab)
    assert np.array_equal(M.rank_counts(s, lab, ones), counts)
    plain, masked = metrics.binary_rank_metrics(counts, lab), metrics.binary_rank_metrics(counts, lab, valid=ones)
    assert set(plain) == set(masked) == {"roc_auc", "AP", "auprc", "max_f1"}
    for key in plain:
        assert np.array_equal(plain[key], masked[key]), key


def test_binary_rank_metrics_with_a_mask_is_the_filtered_problem():
    rng = np.random.default_rng(4)
    s = (rng.integers(0, 8, size=(50, 2)) / 8).astype(np.float32)
    lab = rng.integers(0, 2, size=(50, 2)).astype(np.uint8)
    val = (rng.random((50, 2)) < 0.5).astype(np.uint8)
    got = metrics.binary_rank_metrics(M.rank_counts(s, lab, val), lab, valid=val)
    for c in range(2):
        keep = val[:, c] != 0
        want = metrics.binary_rank_metrics(M.rank_counts(s[keep, c:c + 1], lab[keep, c:c + 1]), lab[keep, c:c + 1])
        for key in want:
            assert got[key][c] == want[key][0], key
    with pytest.raises(ValueError):
        metrics.binary_rank_metrics(M.rank_counts(s, lab, val), lab, valid=val[:, :1])
    with pytest.raises(ValueError, match="empty"):
        metrics.binary_rank_metrics(M.rank_counts(s, lab, val * 0), lab, valid=val * 0)


def test_abi_declares_rank_counts_masked():
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"^int octmae_rank_counts_masked\(", header, re.M)
    assert "octmae_rank_counts_masked" in _lib.SIGNATURES and len(_lib.SIGNATURES["octmae_rank_counts_masked"]) == 10
    assert _lib.expected_abi_version() >= 21                 # 20 before this entry point
    assert re.search(r"^ \* 21: octmae_rank_counts_masked", header, re.M)
    here = os.path.dirname(_lib.LIB_PATH)
    for name in ("liboctmae.so", "liboctmae_f16.so"):
        lib = ctypes.CDLL(os.path.join(here, name))
        assert hasattr(lib, "octmae_rank_counts_masked") and lib.octmae_abi_version() == _lib.expected_abi_version(), name
