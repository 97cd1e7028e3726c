"""GPU tests of the multi-task and regression fine-tune modes: octmae_rank_counts_masked (ops.rank_counts_masked) against the numpy
restatement of tests/multitask_ref.py (compress, count, scatter) -- EQUAL, as integers -- at every edge of the 256-wide block of i
and the 1024-wide LDS tile of j, for four score families and seven mask families, once more on the half-operand build in a child
process (tests/f16_worker.py, started gated before this process touches the GPU: tests/children.py), and engine_finetune.evaluate_task_report /
train_one_epoch end to end on the small ST ViT of tests/test_gpu_metrics.py.

End to end the report is recomputed by metrics.misc_measures_multi_task with the numpy stand-in on the logits THE RUN produced (a
forward hook keeps them: a repeated forward is not promised bit for bit) to the 1e-12 of the goldens (tests/test_cpu_metrics.py: TOL),
and the loss is held against the float64 loop within (k + 8) * 2^-24 * sum|term| (tests/test_cpu_multitask.py)."""
import csv
import functools
import os
import types

import numpy as np
import pytest
import torch

from tests import children
from tests import multitask_ref as M
from tests.test_cpu_metrics import TOL
from tests.test_gpu_metrics import FAMILIES, NS, SPECIAL, small_vit

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_F16 = os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so")
EPS = 2.0 ** -24

assert NS == (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 2051)      # the wave, the block of i, the LDS tile of j, its scalar tail
CS = (1, 2, 6)
MASKS = ("all", "none", "bernoulli", "paired", "single", "last_rows", "second_tile")


def mask_applies(n, C, mask):
    """The families that are another family at this size are not repeated: no row past a multiple of four, no second tile, no pair."""
    return not ((mask == "last_rows" and n % 4 == 0) or (mask == "second_tile" and n <= 1024) or (mask == "paired" and C < 2))


MASKED_CASES = [(n, C, f, m) for n in NS for C in CS for f in FAMILIES for m in MASKS if mask_applies(n, C, m)]


@functools.lru_cache(maxsize=None)
def scores_and_labels(n, C, family):
    rng = np.random.default_rng([n, C, FAMILIES.index(family), 21])
    if family == "continuous":
        s = rng.standard_normal((n, C)).astype(np.float32)
    elif family == "quantised":
        s = (rng.integers(0, 8, size=(n, C)) / 8).astype(np.float32)
    elif family == "equal":
        s = np.full((n, C), 0.25, dtype=np.float32)
    else:
        s = SPECIAL[rng.integers(0, SPECIAL.size, size=(n, C))]
    lab = rng.integers(0, 2, size=(n, C)).astype(np.uint8)
    for a in (s, lab):
        a.setflags(write=False)
    return s, lab


def make_mask(n, C, mask):
    rng = np.random.default_rng([n, C, MASKS.index(mask), 22])
    v = np.zeros((n, C), dtype=np.uint8)
    if mask == "all":
        v[:] = 1
    elif mask == "bernoulli":
        v[:] = rng.random((n, C)) < 0.5
    elif mask == "paired":                                  # columns (2k, 2k + 1) share a mask, as the two columns of a task do
        half = rng.random((n, (C + 1) // 2)) < 0.5
        v[:] = np.repeat(half, 2, axis=1)[:, :C]
    elif mask == "single":
        v[rng.integers(0, n, size=C), np.arange(C)] = 1
    elif mask == "last_rows":
        v[n - n % 4:] = 1
    elif mask == "second_tile":
        v[1024:] = 1
    return v


@functools.lru_cache(maxsize=None)
def masked_case(n, C, family, mask):
    """(scores, labels, valid, the reference counts), seeded; computed once per session and left unchanged."""
    s, lab = scores_and_labels(n, C, family)
    v = make_mask(n, C, mask)
    want = M.rank_counts_masked(s, lab, v)
    for a in (v, want):
        a.setflags(write=False)
    return s, lab, v, want


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                # a copy: the cached cases are read-only


def check_masked(n, C, family, mask):
    from octcubem_amd import ops
    s, lab, v, want = masked_case(n, C, family, mask)
    got = ops.rank_counts_masked(dev(s), dev(lab), dev(v))
    assert got.dtype == torch.int32 and tuple(got.shape) == (n, C, 4) and got.is_contiguous()
    got = got.cpu().numpy()
    assert np.array_equal(got, want), f"n={n} C={C} {family} {mask}: {int((got != want).sum())} counts differ"
    if mask == "all":
        assert np.array_equal(got, ops.rank_counts(dev(s), dev(lab)).cpu().numpy())
    elif mask == "none":
        assert not got.any()
    elif mask == "single":
        rows, cols = np.nonzero(v)
        assert rows.size == C and np.array_equal(got[rows, cols, 2], np.ones(C, dtype=np.int32))
        assert np.array_equal(got[rows, cols, 3], (lab[rows, cols] != 0).astype(np.int32)) and got.sum() == C + int((lab[rows, cols] != 0).sum())


@pytest.mark.parametrize("n,C,family,mask", MASKED_CASES)
def test_masked_rank_counts_equal_compress_count_scatter(n, C, family, mask):
    check_masked(n, C, family, mask)


def test_the_mask_families_cover_what_they_claim():
    from octcubem_amd import ops
    assert callable(ops.rank_counts_masked)                 # the cases below are made for it
    assert len({(n, C) for n, C, _, _ in MASKED_CASES}) == len(NS) * len(CS)
    v = make_mask(2051, 6, "paired")
    assert np.array_equal(v[:, 0], v[:, 1]) and np.array_equal(v[:, 4], v[:, 5]) and not np.array_equal(v[:, 0], v[:, 2])
    assert make_mask(2051, 2, "last_rows").sum() == 2 * 3 and make_mask(1025, 1, "second_tile").sum() == 1
    b = make_mask(2051, 6, "bernoulli")
    assert 0.4 < b.mean() < 0.6 and not np.array_equal(b[:, 0], b[:, 1])
    s, _ = scores_and_labels(2051, 6, "special")
    assert np.isposinf(s).any() and np.isneginf(s).any() and (np.signbit(s) & (s == 0)).any()


@pytest.mark.parametrize("n", (65, 257, 1025))
def test_column_slices_of_wider_buffers(n):
    from octcubem_amd import ops
    rng = np.random.default_rng(n)
    wide_s = (rng.integers(0, 8, size=(n, 7)) / 8).astype(np.float32)
    wide_l = rng.integers(0, 2, size=(n, 9)).astype(np.uint8)
    wide_v = rng.integers(0, 2, size=(n, 11)).astype(np.uint8)
    ds, dl, dv = dev(wide_s), dev(wide_l), dev(wide_v)
    vs, vl, vv = ds[:, 2:5], dl[:, 1:4], dv[:, 6:9]
    assert (vs.stride(0), vl.stride(0), vv.stride(0)) == (7, 9, 11) and not vv.is_contiguous()
    got = ops.rank_counts_masked(vs, vl, vv).cpu().numpy()
    assert np.array_equal(got, M.rank_counts_masked(wide_s[:, 2:5], wide_l[:, 1:4], wide_v[:, 6:9]))
    rows = ops.rank_counts_masked(ds[::2, :3], dl[::2, :3], dv[::2, 8:]).cpu().numpy()          # every second row: 14 / 18 / 22
    assert np.array_equal(rows, M.rank_counts_masked(wide_s[::2, :3], wide_l[::2, :3], wide_v[::2, 8:]))
    as_bool = ops.rank_counts_masked(vs, vl.contiguous().bool(), vv.contiguous().bool()).cpu().numpy()
    assert np.array_equal(as_bool, got)


def test_a_nan_is_refused_only_where_it_is_valid():
    from octcubem_amd import ops
    s, lab, v, _ = masked_case(257, 2, "continuous", "bernoulli")
    out_r, in_r = int(np.nonzero(v[:, 1] == 0)[0][3]), int(np.nonzero(v[:, 1] != 0)[0][3])
    bad = s.copy()
    bad[out_r, 1] = np.nan
    got = ops.rank_counts_masked(dev(bad), dev(lab), dev(v)).cpu().numpy()
    assert np.array_equal(got, M.rank_counts_masked(s, lab, v)) and not got[out_r, 1].any()
    bad[in_r, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        ops.rank_counts_masked(dev(bad), dev(lab), dev(v))


def test_bad_arguments_raise():
    from octcubem_amd import ops
    s, lab, v, _ = masked_case(65, 2, "continuous", "bernoulli")
    ds, dl, dv = dev(s), dev(lab), dev(v)
    for args in ((torch.from_numpy(s), dl, dv), (ds, dl, torch.from_numpy(v)), (ds.double(), dl, dv), (ds, dl, dv.long()),
                 (ds, dl.float(), dv), (ds, dl, dv[:, :1]), (ds, dl, dv[:64]), (ds[:0], dl[:0], dv[:0]),
                 (ds, dl, dv.t().contiguous().t()), (ds, dl, torch.zeros(65, 4, dtype=torch.uint8, device=DEV)[:, ::2])):
        with pytest.raises(Exception):
            ops.rank_counts_masked(*args)
    assert not ops.rank_counts_masked(ds.requires_grad_(), dl, dv).requires_grad


def test_the_entry_point_refuses_a_null_mask_and_writes_every_count():
    from octcubem_amd import _lib
    fn = _lib.load().octmae_rank_counts_masked
    s, lab = torch.zeros(4, 1, device=DEV), torch.ones(4, 1, dtype=torch.uint8, device=DEV)
    v = torch.zeros(4, 1, dtype=torch.uint8, device=DEV)
    out = torch.full((4, 1, 4), 0x7f7f7f7f, dtype=torch.int32, device=DEV)
    p = (s.data_ptr(), 1, lab.data_ptr(), 1, v.data_ptr(), 1, out.data_ptr(), 4, 1)
    for k, bad in ((4, None), (0, None), (2, None), (6, None), (5, 0), (7, 0), (8, 0), (7, 2 ** 31), (8, 65536)):
        assert fn(*(p[:k] + (bad,) + p[k + 1:]), None) == -2, k
    assert fn(s.data_ptr(), 1, lab.data_ptr(), 1, v.data_ptr(), 1, out.data_ptr(), 2, 2, None) == -2       # strides below C
    torch.cuda.synchronize()
    assert bool((out == 0x7f7f7f7f).all())                                  # refused before any launch
    assert fn(*p, None) == 0
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0                                        # nobody is valid: zeros, not the bytes that were there


def test_masked_rank_counts_ignore_autocast():
    from octcubem_amd import ops
    s, lab, v, want = masked_case(257, 2, "continuous", "bernoulli")
    with torch.autocast("cuda", dtype=torch.float16):
        got = ops.rank_counts_masked(dev(s), dev(lab), dev(v))
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------- end to end
N_EVAL, BATCH, TASKS = 13, 4, 3
NAMES = ["normal", "amd", "dme", "rvo"]


def multi_task_targets_for_eval():
    """int64 [13, 4]: no degenerate population (checked), one sample normal and ill, one without any label, task 1 leaves out 6 of 13."""
    t = torch.tensor([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1, 1, 0, 0], [0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 1, 0],
                      [0, 0, 1, 0], [1, 0, 0, 0], [0, 1, 0, 1], [0, 0, 0, 1], [0, 1, 0, 0]])
    pop = (t[:, :1] + t[:, 1:]) > 0
    for i in range(TASKS):
        for col in (t[pop[:, i], 0], t[pop[:, i], 1 + i]):
            assert 0 < int(col.sum()) < col.numel()
    assert int((~pop[:, 1]).sum()) == 6
    return t


def eval_loader(targets):
    x = torch.rand(N_EVAL, 1, 6, 32, 32, generator=torch.Generator().manual_seed(5))
    return [(x[i:i + BATCH], targets[i:i + BATCH]) for i in range(0, N_EVAL, BATCH)]


def keep_outputs(model):
    kept = []
    handle = model.register_forward_hook(lambda mod, inp, out: kept.append(out.detach().float().cpu()))
    return kept, handle


def read_rows(path):
    with open(path, newline="", encoding="utf8") as f:
        return list(csv.reader(f))


def test_evaluate_task_report_multi_task_end_to_end(tmp_path):
    from octcubem_amd import engine_finetune, losses, metrics
    model = small_vit(2 * TASKS, seed=12)
    targets = multi_task_targets_for_eval()
    loader = eval_loader(targets)
    crit = losses.WeightedLabelSmoothingCrossEntropy(0.1)
    kept, handle = keep_outputs(model)
    task = str(tmp_path / "report")
    stats, roc, pr = engine_finetune.evaluate_task_report(loader, model, torch.device(DEV), task, 3, "test", 2 * TASKS, criterion=crit,
                                                          task_mode="multi_task_default", disease_list=NAMES)
    logits = torch.cat(kept).numpy()
    del kept[:]
    assert logits.shape == (N_EVAL, 2 * TASKS) and not model.training and set(stats) == {"loss", "acc1"}
    want = metrics.misc_measures_multi_task(targets.numpy(), logits, multi_task_type="multi_task_default", rank_counts=M.rank_counts)
    print(f"multi_task_default: loss {stats['loss']!r}, acc1 {stats['acc1']!r}, roc_auc {roc!r} / {want['macro']['roc_auc']!r}, "
          f"auprc {pr!r} / {want['macro']['auprc']!r}")
    assert abs(roc - want["macro"]["roc_auc"]) <= TOL and abs(pr - want["macro"]["auprc"]) <= TOL
    assert abs(stats["acc1"] - want["macro"]["accuracy"]) <= TOL
    # the loss: multi_task_loss of the concatenated batch, against the float64 loop
    loop, terms, _, _ = M.multi_task_loss(logits, targets.numpy(), 0.1, "multi_task_default")
    bound = (terms.size + 8) * EPS * float(np.abs(terms).sum())
    print(f"  loss against the float64 loop: difference {abs(stats['loss'] - loop):.3e}, bound {bound:.3e}")
    assert abs(stats["loss"] - loop) <= bound
    on_device = float(losses.multi_task_loss(torch.from_numpy(logits).to(DEV), targets.to(DEV), crit, "multi_task_default"))
    assert abs(stats["loss"] - on_device) <= 2 * bound
    # the files
    rows = read_rows(os.path.join(task, "macro_metrics_test.csv"))
    assert rows[0] == engine_finetune.MACRO_HEADER and len(rows) == 2
    got_macro = dict(zip(rows[0], (float(v) for v in rows[1])))
    assert got_macro["loss"] == stats["loss"] and got_macro["ROC AUC"] == roc and got_macro["AUPRC"] == pr
    for head, key in zip(engine_finetune.MACRO_HEADER[:-1], engine_finetune._MACRO_KEYS):
        assert abs(got_macro[head] - want["macro"][key]) <= TOL, key
    pop = ((targets[:, :1] + targets[:, 1:]) > 0).numpy()
    for i in range(TASKS):
        per = read_rows(os.path.join(task, f"class_{i + 1}_{NAMES[i + 1]}_metrics_test.csv"))
        assert per[0] == engine_finetune.CLASS_HEADER and len(per) == 2
        for j, key in enumerate(engine_finetune._CLASS_KEYS):
            assert abs(float(per[1][j]) - want["classwise"][key][i]) <= TOL, (i, key)
        cm = np.array(read_rows(os.path.join(task, f"confusion_matrix_test_{i + 1}_{NAMES[i + 1]}_epoch_3.csv")), dtype=np.int64)
        assert cm.shape == (2, 2) and cm.sum() == pop[:, i].sum() and cm[1].sum() == int(targets[pop[:, i], i + 1].sum())
        assert abs((cm[0, 0] + cm[1, 1]) / (cm.sum() + 1e-8) - want["classwise"]["accuracy"][i]) <= TOL
    # names through multi_task_idx, a validation mode (no confusion matrices), return_bal_acc, inside autocast
    args = types.SimpleNamespace(multi_task_idx=[3, 1, 2])
    with torch.autocast("cuda", dtype=torch.float16):
        stats2, roc2, (pr2, bal) = engine_finetune.evaluate_task_report(loader, model, torch.device(DEV), str(tmp_path / "idx"), 0, "val",
                                                                        2 * TASKS, criterion=crit, task_mode="multi_task_default",
                                                                        disease_list=NAMES, return_bal_acc=True, args=args)
    handle.remove()
    again = metrics.misc_measures_multi_task(targets.numpy(), torch.cat(kept).numpy(), multi_task_type="multi_task_default",
                                             rank_counts=M.rank_counts)
    assert abs(roc2 - again["macro"]["roc_auc"]) <= TOL and abs(pr2 - again["macro"]["auprc"]) <= TOL
    assert abs(bal - again["macro"]["balanced_acc"]) <= TOL and abs(stats2["loss"] - stats["loss"]) <= 1e-6
    assert sorted(os.listdir(str(tmp_path / "idx"))) == sorted(
        ["macro_metrics_val.csv", "class_1_rvo_metrics_val.csv", "class_2_amd_metrics_val.csv", "class_3_dme_metrics_val.csv"])
    # without a list the tasks are numbered; not_save_figs keeps the matrices away in a test mode too
    engine_finetune.evaluate_task_report(loader, model, torch.device(DEV), str(tmp_path / "bare"), 0, "test", 2 * TASKS, criterion=crit,
                                         task_mode="multi_task_default", args=types.SimpleNamespace(not_save_figs=True))
    assert sorted(os.listdir(str(tmp_path / "bare"))) == sorted(["macro_metrics_test.csv"] + [f"class_{i}_{i}_metrics_test.csv" for i in (1, 2, 3)])


def test_evaluate_task_report_shared_column_layout_and_errors(tmp_path):
    from octcubem_amd import engine_finetune, losses, metrics
    model = small_vit(TASKS + 1, seed=13)
    targets = multi_task_targets_for_eval()
    kept, handle = keep_outputs(model)
    crit = losses.WeightedLabelSmoothingCrossEntropy(0.1)
    stats, roc, pr = engine_finetune.evaluate_task_report(eval_loader(targets), model, torch.device(DEV), str(tmp_path / "s"), 0, "val",
                                                          TASKS + 1, criterion=crit, task_mode="multi_task", disease_list=NAMES)
    handle.remove()
    logits = torch.cat(kept).numpy()
    want = metrics.misc_measures_multi_task(targets.numpy(), logits, multi_task_type="multi_task", rank_counts=M.rank_counts)
    loop, terms, _, _ = M.multi_task_loss(logits, targets.numpy(), 0.1, "multi_task")
    assert abs(roc - want["macro"]["roc_auc"]) <= TOL and abs(pr - want["macro"]["auprc"]) <= TOL
    assert abs(stats["loss"] - loop) <= (terms.size + 8) * EPS * float(np.abs(terms).sum())
    with pytest.raises(ValueError, match="num_class"):
        engine_finetune.evaluate_task_report(eval_loader(targets), model, torch.device(DEV), str(tmp_path / "e"), 0, "val", 2 * TASKS,
                                             criterion=crit, task_mode="multi_task")
    nobody_normal = targets.clone()
    nobody_normal[:, 0] = 0
    with pytest.raises(ValueError, match="task 0"):
        engine_finetune.evaluate_task_report(eval_loader(nobody_normal), model, torch.device(DEV), str(tmp_path / "e"), 0, "val", TASKS + 1,
                                             criterion=crit, task_mode="multi_task")


def test_one_train_step_in_multi_task_mode():
    """One step of train_one_epoch (accum_iter 2, so the gradients of the one batch stay in place): with task_mode
    'multi_task_default' and the weighted criterion the loss is multi_task_loss of the batch -- held against the float64 loop on the
    logits of that forward -- and every parameter that a plain step reaches gets a gradient; without task_mode, with another task_mode
    or with another criterion the step is today's ``criterion(outputs, targets)``, bit for bit."""
    from octcubem_amd import engine_finetune, losses
    targets = multi_task_targets_for_eval()[:8]
    x = torch.rand(8, 1, 6, 32, 32, generator=torch.Generator().manual_seed(6))
    wide = torch.cat([targets, targets[:, 1:3]], dim=1)                    # [8, 6]: what the criterion needs when it sees [8, 6] logits
    weighted = losses.WeightedLabelSmoothingCrossEntropy(0.1)

    def step(criterion, tgt, **mode):
        args = types.SimpleNamespace(accum_iter=2, lr=1e-3, min_lr=1e-6, warmup_epochs=1, epochs=4, **mode)
        model = small_vit(2 * TASKS, seed=14)
        kept, handle = keep_outputs(model)
        opt = torch.optim.SGD(model.parameters(), lr=0.0)

        def scaler(loss, optimizer, **kw):
            assert kw["update_grad"] is False
            loss.backward()

        stats = engine_finetune.train_one_epoch(model, criterion, [(x, tgt)], opt, torch.device(DEV), 0, scaler, 0, None, None, args)
        handle.remove()
        torch.cuda.synchronize()
        assert stats is not None and len(kept) == 1
        return stats["loss"], kept[0].numpy(), {k: (None if p.grad is None else p.grad.clone()) for k, p in model.named_parameters()}

    def today(criterion, tgt):
        model = small_vit(2 * TASKS, seed=14)
        model.train(True)
        loss = criterion(model(x.to(DEV)), tgt.to(DEV))
        (loss / 2).backward()
        torch.cuda.synchronize()
        return float(loss.detach()), {k: (None if p.grad is None else p.grad.clone()) for k, p in model.named_parameters()}

    base_loss, base = today(weighted, wide)
    assert any(g is not None for g in base.values())
    loss, logits, grads = step(weighted, targets, task_mode="multi_task_default")
    loop, terms, _, _ = M.multi_task_loss(logits, targets.numpy(), 0.1, "multi_task_default")
    bound = (terms.size + 8) * EPS * float(np.abs(terms).sum())
    print(f"train step: loss {loss!r}, float64 loop {loop!r}, difference {abs(loss - loop):.3e}, bound {bound:.3e}")
    assert abs(loss - loop) <= bound
    for k, g in grads.items():
        assert (g is not None) == (base[k] is not None), k
        assert g is None or bool(torch.isfinite(g).all()), k
    missing = [k for k, g in grads.items() if g is None]
    print(f"  parameters without a gradient (the same in a plain step): {missing}")
    head = [k for k in grads if k.startswith("head.") and k.endswith("weight")]
    assert head and bool((grads[head[0]].abs().sum(dim=1) > 0).all())          # all 2T outputs are reached
    # not dispatched: no task_mode, another task_mode, another criterion -- today's step
    for criterion, mode in ((weighted, {}), (weighted, {"task_mode": "multi_label"}),
                            (lambda o, t: weighted(o, t), {"task_mode": "multi_task_default"})):
        loss_n, _, grads_n = step(criterion, wide, **mode)
        assert loss_n == base_loss, mode
        for k, g in base.items():
            assert (g is None and grads_n[k] is None) or torch.equal(g, grads_n[k]), (mode, k)


def test_evaluate_task_report_regression_end_to_end(tmp_path):
    from octcubem_amd import engine_finetune, metrics
    model = small_vit(1, seed=15)
    g = torch.Generator().manual_seed(7)
    x = torch.rand(N_EVAL, 1, 6, 32, 32, generator=g)
    t = torch.rand(N_EVAL, 1, generator=g)
    loader = [(x[i:i + BATCH], t[i:i + BATCH]) for i in range(0, N_EVAL, BATCH)]
    crit = torch.nn.MSELoss()
    kept, handle = keep_outputs(model)
    task = str(tmp_path / "reg")
    res = engine_finetune.evaluate_task_report(loader, model, torch.device(DEV), task, 0, "test", 1, criterion=crit, task_mode="regression")
    handle.remove()
    out = torch.cat(kept)
    assert out.shape == (N_EVAL, 1) and tuple(res) == ("pearsonr", "r2", "explained_variance", "mse", "mae", "R2", "loss")
    want = metrics.regression_measures(out[:, 0].numpy(), t[:, 0].numpy())
    print(f"regression: {res}")
    for key, v in want.items():
        assert abs(res[key] - v) <= 1e-12 * max(1.0, abs(v)), key              # the same float64 finish on the same float32 vectors
    want_loss = float(((out.double() - t.double()) ** 2).mean())               # batches of one column: the mean over samples is the MSE
    assert abs(res["loss"] - want_loss) <= 1e-6 * want_loss and abs(res["loss"] - res["mse"]) <= 1e-6 * want_loss
    rows = read_rows(os.path.join(task, "regression_metrics_test.csv"))
    assert rows[0] == engine_finetune.REGRESSION_HEADER and rows[1] == [f"{res[k]:.4f}" for k in res] and len(rows) == 2


def test_the_new_loss_functions_ignore_autocast():
    from octcubem_amd import losses
    from tests.test_cpu_multitask import golden_problem
    crit = losses.WeightedLabelSmoothingCrossEntropy(0.1)
    for k in (0, 1):
        y, logits, kind = golden_problem(k)
        t = torch.from_numpy(y).to(DEV)
        results = []
        for ctx in (lambda: torch.autocast("cuda", enabled=False), lambda: torch.autocast("cuda", dtype=torch.float16),
                    lambda: torch.autocast("cuda", dtype=torch.bfloat16)):
            x = torch.from_numpy(logits).to(DEV).requires_grad_()
            with ctx():
                loss = losses.multi_task_loss(x, t, crit, kind)
                looped = losses.multi_task_loss(x, t, lambda o, tt: crit(o, tt), kind)
                tm, w = losses.multi_task_targets(t.float())
            loss.backward()
            results.append((loss.detach(), looped.detach(), x.grad.clone(), tm, w))
        for r in results:
            assert r[0].dtype == torch.float32 and r[3].dtype == torch.float32
            for a, b in zip(r, results[0]):
                assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- the half build
def half_build_cases():
    """What tests/f16_worker.py runs on the half-operand build."""
    for case in MASKED_CASES:
        check_masked(*case)
    return {"passed": [list(c) for c in MASKED_CASES]}


def start_children():
    """tests/conftest.py calls this once the collection holds a test of this module, before this process has touched the GPU;
    tests/children.py releases the worker when the GPU has room for it."""
    if os.path.exists(LIB_F16):
        children.spawn_f16_worker("multitask_f16", "tests.test_gpu_multitask:half_build_cases", limit_s=240)


def test_half_build_runs_the_same_masked_kernel():
    """The entry point has no 16-bit operand: liboctmae_f16.so must give the same counts on every masked case.  The child was started
    before this process touched the GPU; it is released here and then runs under its own time limit."""
    assert os.path.exists(LIB_F16), "make -C octcubem_amd/csrc both"
    start_children()
    res = children.f16_worker_result("multitask_f16")
    assert res["lib"] == "liboctmae_f16.so" and res["lp_is_f16"] is True
    assert res["passed"] == [list(c) for c in MASKED_CASES], res
