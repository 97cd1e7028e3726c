"""CPU tests of the fine-tune evaluation's metric code (octcubem_amd/metrics.py, the host half of engine_finetune.evaluate_report).

The host finish is fed with rank counts from the numpy restatement (tests/metrics_ref.py: rank_counts) and must equal the independent
sort-based float64 values of the same file to 1e-12: both are a handful of float64 divisions and one sum of at most 60 terms of size
<= 1, so they agree to a few ulp (1e-15); 1e-12 is what the issue sets.  Five hand cases carry their values as fractions.

``misc_measures`` / ``misc_measures_multi_label`` are pinned to tests/golden/metrics_small.npz, which tools/gen_golden_metrics.py wrote by
calling the reference's own functions.  That file was written WITH scikit-learn (``sklearn_version``), so every key of the reference's
dict is pinned: accuracy, roc_auc, precision, recall, f1, AP, auprc, specificity, sensitivity, mcc, G, micro_AP (macro only),
balanced_acc, kappa, max_f1.  A file written without it would hold ``misc_measures`` alone, and the test says so instead of passing."""
import os
import re
import zlib
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

from octcubem_amd import _lib, engine_finetune, metrics
from tests import metrics_ref as R

TOL = 1e-12
N_GOLDEN = 3
KEYS = ("roc_auc", "AP", "auprc", "max_f1")


def reference_values(scores, labels):
    s, y = np.asarray(scores, dtype=np.float32), np.asarray(labels)
    return {"roc_auc": [R.auroc(s[:, c], y[:, c]) for c in range(s.shape[1])],
            "AP": [R.average_precision(s[:, c], y[:, c]) for c in range(s.shape[1])],
            "auprc": [R.auprc(s[:, c], y[:, c]) for c in range(s.shape[1])],
            "max_f1": [R.max_f1(s[:, c], y[:, c]) for c in range(s.shape[1])]}


def finish(scores, labels):
    s, y = np.asarray(scores, dtype=np.float32), np.asarray(labels, dtype=np.uint8)
    return metrics.binary_rank_metrics(R.rank_counts(s, y), y)


# scores, labels, AUROC, AP, trapezoid AUPRC -- worked out by hand from the curves (one point per distinct score)
HAND = [
    ([.1, .4, .35, .8], [0, 0, 1, 1], Fr(3, 4), Fr(5, 6), Fr(19, 24)),           # scikit-learn's own documentation example
    ([.5, .5, .5, .5, .5], [1, 0, 1, 0, 0], Fr(1, 2), Fr(2, 5), Fr(7, 10)),      # all tied: AUROC 1/2, AP = P / n
    ([.9, .8, .2, .1], [1, 1, 0, 0], Fr(1), Fr(1), Fr(1)),                       # separated
    ([.1, .2, .8, .9], [1, 1, 0, 0], Fr(0), Fr(5, 12), Fr(7, 24)),               # inverted
    ([.5, .5, .3, .3, .1], [1, 0, 1, 0, 0], Fr(2, 3), Fr(1, 2), Fr(5, 8)),       # two ties that mix the labels
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_hand_cases_as_fractions(case):
    s, y, auroc, ap, auprc = HAND[case]
    s, y = np.array(s, dtype=np.float32)[:, None], np.array(y)[:, None]
    got, ref = finish(s, y), reference_values(s, y)
    for key, want in (("roc_auc", auroc), ("AP", ap), ("auprc", auprc)):
        assert abs(got[key][0] - float(want)) <= TOL, (key, got[key][0], want)
        assert abs(ref[key][0] - float(want)) <= TOL, ("reference", key, ref[key][0], want)
    assert abs(got["max_f1"][0] - ref["max_f1"][0]) <= TOL


def test_signed_zero_ties_and_infinities_order():
    """-0.0 ties with 0.0; +-inf are the extreme values."""
    s = np.array([0.0, -0.0, np.inf, -np.inf, 1e-40], dtype=np.float32)[:, None]
    y = np.array([1, 0, 1, 0, 0])[:, None]
    got = finish(s, y)
    # positives: +inf beats all 3 negatives; 0.0 beats -inf, ties with -0.0, loses to 1e-40 (a denormal above zero)
    assert abs(got["roc_auc"][0] - float(Fr(3 + 1 + Fr(1, 2), 6))) <= TOL
    assert abs(got["roc_auc"][0] - R.auroc(s[:, 0], y[:, 0])) <= TOL


@pytest.mark.parametrize("seed", range(50))
def test_random_quantised_cases(seed):
    rng = np.random.default_rng(1000 + seed)
    n, C = int(rng.integers(5, 61)), int(rng.integers(1, 4))
    s = (rng.integers(0, 8, size=(n, C)) / 8).astype(np.float32)
    y = rng.integers(0, 2, size=(n, C))
    y[0], y[1] = 1, 0                                         # both label values in every class
    got, ref = finish(s, y), reference_values(s, y)
    for key in KEYS:
        np.testing.assert_allclose(got[key], ref[key], rtol=0, atol=TOL, err_msg=key)


def test_one_label_value_raises():
    s = np.array([.1, .2, .3], dtype=np.float32)[:, None]
    for y in ([0, 0, 0], [1, 1, 1]):
        y = np.array(y)[:, None]
        with pytest.raises(ValueError):
            finish(s, y)
        with pytest.raises(ValueError):
            R.auroc(s[:, 0], y[:, 0])
    with pytest.raises(ValueError):                          # one bad class among good ones
        finish(np.tile(s, (1, 2)), np.array([[0, 1], [1, 1], [0, 1]]))


@pytest.mark.parametrize("mode", ("regression", "multi_task_default", "multi_task"))
def test_unbuilt_task_modes_raise_and_name_the_mode(mode, tmp_path):
    with pytest.raises(NotImplementedError, match=mode):
        engine_finetune.evaluate_report([], None, "cpu", str(tmp_path), 0, "val", 2, task_mode=mode)


def test_unbuilt_arguments_are_refused(tmp_path):
    import types
    for name in ("frame_inference_all", "return_embeddings", "variable_joint"):
        with pytest.raises(AssertionError, match=name):
            engine_finetune.evaluate_report([], None, "cpu", str(tmp_path), 0, "val", 2, args=types.SimpleNamespace(**{name: True}))


def test_abi_declares_rank_counts():
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"^int octmae_rank_counts\(", header, re.M)
    assert "octmae_rank_counts" in _lib.SIGNATURES and len(_lib.SIGNATURES["octmae_rank_counts"]) == 8
    assert _lib.expected_abi_version() >= 18                 # 17 before this entry point
    assert re.search(r"^ \* 18: octmae_rank_counts", header, re.M)
    mk = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bmetrics\.hip\b", mk, re.M)


# ---------------------------------------------------------------------------------------------- the reference's two functions
def golden_problem(k):
    """(true_idx [n], pred_idx [n], num_class, y_true [n, C] int64, y_prob [n, C] float32), seeded.  Problem 2 has scores on a grid of
    eighths, so ties dominate and some sit exactly on the 0.5 threshold."""
    n, num_class, C = ((12, 2, 3), (25, 4, 4), (40, 3, 2))[k]
    rng = np.random.default_rng(77 + k)
    true_idx = rng.integers(0, num_class, size=n)
    true_idx[:num_class] = np.arange(num_class)
    pred_idx = np.where(rng.random(n) < 0.6, true_idx, rng.integers(0, num_class, size=n))
    y_true = rng.integers(0, 2, size=(n, C))
    y_true[0], y_true[1] = 1, 0
    y_prob = np.clip(0.35 * y_true + 0.75 * rng.random((n, C)), 0, 1)
    if k == 2:
        y_prob = np.round(y_prob * 8) / 8
    return true_idx.astype(np.int64), pred_idx.astype(np.int64), num_class, y_true.astype(np.int64), y_prob.astype(np.float32)


def crc(*arrays):
    return zlib.crc32(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays))


def one_vs_rest(true_idx, pred_idx, num_class):
    """[[tn, fp], [fn, tp]] per class, written out."""
    out = np.zeros((num_class, 2, 2), dtype=np.int64)
    for c in range(num_class):
        t, p = true_idx == c, pred_idx == c
        out[c] = [[(~t & ~p).sum(), (~t & p).sum()], [(t & ~p).sum(), (t & p).sum()]]
    return out


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "metrics_small.npz"))


@pytest.mark.parametrize("k", range(N_GOLDEN))
def test_misc_measures_equals_the_reference(k, golden):
    true_idx, pred_idx, num_class, y_true, y_prob = golden_problem(k)
    assert crc(true_idx, pred_idx, y_true, y_prob) == int(golden[f"crc_{k}"]), "the seeded inputs are not the ones the fixture was made from"
    ovr = metrics.multilabel_confusion(torch.from_numpy(true_idx), torch.from_numpy(pred_idx), num_class)
    assert ovr.dtype == torch.int64 and np.array_equal(ovr.numpy(), golden[f"ovr_{k}"])
    assert np.array_equal(one_vs_rest(true_idx, pred_idx, num_class), golden[f"ovr_{k}"])
    got = metrics.misc_measures(ovr.numpy())
    assert len(got) == 8
    np.testing.assert_allclose(np.array(got, dtype=np.float64), golden[f"measures_{k}"], rtol=0, atol=TOL)
    full = metrics.confusion_counts(torch.from_numpy(true_idx), torch.from_numpy(pred_idx), num_class).numpy()
    assert full.sum() == true_idx.size and np.array_equal(np.diag(full), golden[f"ovr_{k}"][:, 1, 1])


MACRO = ("accuracy", "roc_auc", "precision", "recall", "f1", "AP", "auprc", "specificity", "sensitivity", "mcc", "G", "micro_AP",
         "balanced_acc", "kappa", "max_f1")


@pytest.mark.parametrize("k", range(N_GOLDEN))
def test_misc_measures_multi_label_equals_the_reference(k, golden):
    assert str(golden["sklearn_version"]) != "absent", "the fixture was written without scikit-learn: only misc_measures is pinned"
    _, _, _, y_true, y_prob = golden_problem(k)
    res = metrics.misc_measures_multi_label(y_true, y_prob, threshold=0.5, rank_counts=R.rank_counts)
    assert tuple(res["macro"]) == MACRO and tuple(res["classwise"]) == tuple(m for m in MACRO if m != "micro_AP")
    for half in ("macro", "classwise"):
        for key, v in res[half].items():
            np.testing.assert_allclose(np.asarray(v, dtype=np.float64), golden[f"{half}_{k}/{key}"], rtol=0, atol=TOL, err_msg=f"{half} {key}")


def test_multi_label_on_a_host_array_needs_a_counter():
    """Without ``rank_counts`` the counts come from the HIP kernel, which takes GPU tensors only: no silent CPU path."""
    _, _, _, y_true, y_prob = golden_problem(0)
    with pytest.raises(TypeError):
        metrics.misc_measures_multi_label(y_true, y_prob)
    with pytest.raises(RuntimeError):
        metrics.misc_measures_multi_label(torch.from_numpy(y_true), torch.from_numpy(y_prob))
