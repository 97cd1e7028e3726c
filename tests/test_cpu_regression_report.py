"""CPU tests of the regression mode of the fine-tune evaluation (metrics.regression_measures, engine_finetune.evaluate_task_report)
and of evaluate_task_report's dispatch.

The seven values are pinned to tests/golden/metrics_multitask_small.npz (tools/gen_golden_multitask.py: the reference's five scipy /
scikit-learn calls; R2 is the square of the first, the loss is the criterion's).  The fixture holds them twice:

  ``reg_f64_<k>``  scipy 1.15 / scikit-learn 1.7 called on the float64 copies of the vectors.  Measured once against the installed
                   libraries: the largest relative difference of regression_measures over both problems and all five values is
                   1.2e-16 (one ulp, on pearsonr of the small problem; the other nine are equal) -- float64 sums of 57 / 3000
                   terms.  Bound: 8 x that is 9.0e-16, below the floor, so 1e-12 relative.
  ``reg_<k>``      the same calls on the float32 vectors themselves, as the reference makes them: both libraries then work in
                   float32 (scipy's pearsonr takes its dtype from the inputs, scikit-learn averages in the input's precision).
                   Measured once: largest relative difference 3.1e-07 (explained variance of the small problem, a few
                   float32 ulp of a difference of two float32 variances).  Bound: 8 x that, 2.5e-06 relative.

The bounds come from those two measurements against the libraries, not from runs of this package against itself."""
import csv
import os
import types

import numpy as np
import pytest
import torch

from octcubem_amd import engine_finetune, metrics
from tests.test_cpu_multitask import crc

N_REGRESSION = 2
KEYS = ("pearsonr", "r2", "explained_variance", "mse", "mae")
RTOL_F64 = max(8 * 1.2e-16, 1e-12)
RTOL_F32 = 8 * 3.1e-07


def regression_problem(k):
    """(pred float32 [n], target float32 [n]), seeded: 57 samples of a weak fit, 3000 of a good one with an offset."""
    n, slope, offset, noise = ((57, 0.4, 0.0, 1.0), (3000, 1.1, 0.7, 0.3))[k]
    rng = np.random.default_rng(300 + k)
    target = (2.0 + 1.5 * rng.standard_normal(n)).astype(np.float32)
    pred = (slope * target + offset + noise * rng.standard_normal(n)).astype(np.float32)
    return pred, target


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "metrics_multitask_small.npz"))


@pytest.mark.parametrize("k", range(N_REGRESSION))
def test_regression_measures_equal_scipy_and_scikit_learn(k, golden):
    pred, target = regression_problem(k)
    assert crc(pred, target) == int(golden[f"reg_crc_{k}"]), "the seeded inputs are not the ones the fixture was made from"
    got = metrics.regression_measures(pred, target)
    assert tuple(got) == KEYS + ("R2",)
    vals = np.array([got[key] for key in KEYS])
    for name, rtol in (("reg_f64", RTOL_F64), ("reg", RTOL_F32)):
        want = golden[f"{name}_{k}"]
        rel = np.abs(vals - want) / np.abs(want)
        print(f"problem {k} against {name}: relative differences {rel}")
        assert (rel <= rtol).all(), (name, rel)
    assert got["R2"] == got["pearsonr"] ** 2 and abs(got["R2"] - golden[f"reg_f64_{k}"][0] ** 2) <= RTOL_F64 * 2
    as_tensors = metrics.regression_measures(torch.from_numpy(pred), torch.from_numpy(target))
    assert as_tensors == got


def test_constant_inputs_raise():
    pred, target = regression_problem(0)
    flat = np.full_like(pred, 1.25)
    for a, b, word in ((pred, flat, "targets"), (flat, target, "predictions"), (flat, flat, "predictions")):
        with pytest.raises(ValueError, match=word):
            metrics.regression_measures(a, b)
    with pytest.raises(ValueError):
        metrics.regression_measures(pred[:1], target[:1])
    with pytest.raises(ValueError):
        metrics.regression_measures(pred, target[:-1])


class Linear(torch.nn.Module):
    """A CPU stub: ``classes`` fixed linear read-outs of the sample's mean and first value."""

    def __init__(self, classes):
        super().__init__()
        self.w = torch.nn.Parameter(torch.linspace(-1.0, 1.5, 2 * classes).reshape(2, classes))

    def forward(self, x):
        f = x.flatten(1)
        return torch.stack([f.mean(1), f[:, 0]], dim=1) @ self.w + 0.1


def regression_loader(two_d):
    g = torch.Generator().manual_seed(9)
    x = torch.rand(11, 1, 4, 4, generator=g)
    t = 0.8 * x.flatten(1).mean(1) + 0.2 * torch.rand(11, generator=g)
    t = torch.stack([t, torch.zeros(11)], dim=1) if two_d else t.unsqueeze(1)
    return [(x[i:i + 4], t[i:i + 4]) for i in range(0, 11, 4)], x, t


@pytest.mark.parametrize("two_d", (False, True))
def test_regression_report_on_a_stub_model(two_d, tmp_path):
    classes = 2 if two_d else 1
    model, crit = Linear(classes), torch.nn.MSELoss()
    loader, x, t = regression_loader(two_d)
    with torch.no_grad():
        out = model(x)
        want_loss = sum(float(crit(model(b[0]), b[1])) * b[0].shape[0] for b in loader) / 11
    want = metrics.regression_measures(out[:, 0].numpy(), t[:, 0].numpy())
    task = str(tmp_path / "rep")
    res = engine_finetune.evaluate_task_report(loader, model, "cpu", task, 2, "val", classes, criterion=crit, task_mode="regression")
    assert tuple(res) == ("pearsonr", "r2", "explained_variance", "mse", "mae", "R2", "loss") and not model.training
    for key in want:
        assert abs(res[key] - want[key]) <= 1e-12 * max(1.0, abs(want[key])), key
    assert abs(res["loss"] - want_loss) <= 1e-6
    engine_finetune.evaluate_task_report(loader, model, "cpu", task, 3, "val", classes, criterion=crit, task_mode="regression")
    with open(os.path.join(task, "regression_metrics_val.csv"), newline="", encoding="utf8") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["Pearsonr", "R²", "ExplainedVariance", "MSE", "MAE", "R2", "Loss"] == engine_finetune.REGRESSION_HEADER
    assert len(rows) == 3 and rows[1] == rows[2] == [f"{res[key]:.4f}" for key in res]
    assert all(len(v.split(".")[1]) == 4 for v in rows[1])


def test_regression_report_refuses_constant_targets(tmp_path):
    loader, x, t = regression_loader(False)
    loader = [(b[0], torch.ones_like(b[1])) for b in loader]
    with pytest.raises(ValueError, match="constant targets"):
        engine_finetune.evaluate_task_report(loader, Linear(1), "cpu", str(tmp_path), 0, "val", 1, criterion=torch.nn.MSELoss(),
                                             task_mode="regression")


def test_unknown_mode_and_unbuilt_arguments(tmp_path):
    with pytest.raises(ValueError, match="no_such_mode"):
        engine_finetune.evaluate_task_report([], None, "cpu", str(tmp_path), 0, "val", 2, task_mode="no_such_mode")
    for mode in ("regression", "multi_task_default"):
        for name in ("frame_inference_all", "return_embeddings", "variable_joint"):
            with pytest.raises(AssertionError, match=name):
                engine_finetune.evaluate_task_report([], None, "cpu", str(tmp_path), 0, "val", 2, task_mode=mode,
                                                     args=types.SimpleNamespace(**{name: True}))
    with pytest.raises(ValueError, match="no sample"):
        engine_finetune.evaluate_task_report([], Linear(1), "cpu", str(tmp_path), 0, "val", 1, task_mode="regression")


def test_classification_modes_are_forwarded_to_evaluate_report(tmp_path, monkeypatch):
    """binary_cls / multi_cls / multi_label reach evaluate_report with every argument unchanged, and its result comes back as it is."""
    seen = []

    def spy(*a, **kw):
        seen.append((a, kw))
        return "result"

    monkeypatch.setattr(engine_finetune, "evaluate_report", spy)
    crit, args, loader, model = torch.nn.BCEWithLogitsLoss(), types.SimpleNamespace(), [1], Linear(2)
    for mode in ("binary_cls", "multi_cls", "multi_label"):
        got = engine_finetune.evaluate_task_report(loader, model, "cpu", str(tmp_path), 5, "test", 2, criterion=crit, task_mode=mode,
                                                   disease_list=["a", "b"], return_bal_acc=True, args=args)
        assert got == "result"
        a, kw = seen.pop()
        assert a[0] is loader and a[1] is model and a[2:] == ("cpu", str(tmp_path), 5, "test", 2)
        assert kw == dict(criterion=crit, task_mode=mode, disease_list=["a", "b"], return_bal_acc=True, args=args)


def test_binary_cls_through_the_forward_fails_where_evaluate_report_fails(tmp_path):
    """Not a stub: the real evaluate_report behind the forward needs the HIP kernel for its rank counts, so on CPU tensors it raises
    what ops.rank_counts raises -- there is no silent CPU path behind the new entry point either."""
    g = torch.Generator().manual_seed(2)
    loader = [(torch.rand(4, 1, 4, 4, generator=g), torch.tensor([0, 1, 0, 1]))]
    with pytest.raises(RuntimeError, match="GPU tensors"):
        engine_finetune.evaluate_task_report(loader, Linear(2), "cpu", str(tmp_path), 0, "val", 2, task_mode="binary_cls")
