"""GPU tests of the fine-tune evaluation: octmae_rank_counts (ops.rank_counts) against the numpy comparison table of
tests/metrics_ref.py -- EQUAL, as integers -- at every edge of the 256-wide block of i and the 1024-wide LDS tile of j, once more on
the half-operand build in a child process (tests/f16_worker.py, started before this process touches the GPU), and
engine_finetune.evaluate_report end to end on a small ST ViT.

End to end: ``loss`` and ``acc1`` against the existing ``evaluate`` on the same loader to 1e-6 (the same per-batch fp32 losses, summed in
float64 on the device instead of on the host), ``auc_roc`` / ``auc_pr`` against the sort-based float64 references applied to the
logits ``evaluate`` returns to 1e-12 (a few float64 divisions and sums of at most 13 terms: a few ulp), the CSV row parsed back."""
import csv
import functools
import os
from functools import partial

import numpy as np
import pytest
import torch

from tests import children
from tests import metrics_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_F16 = os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so")

# 1 / 2: below a wave; 63 / 64 / 65: the wave; 255 / 256 / 257: the block of i, a second workgroup; 1023 / 1025: the LDS tile of j,
# a second tile with one value (the scalar tail after the groups of four); 2051: three tiles, nine workgroups, n % 4 = 3
NS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 2051)
CS = (1, 2, 5)
FAMILIES = ("continuous", "quantised", "equal", "special")
SPECIAL = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, np.inf, -np.inf, 1.0, -1.0, 3.4e38], dtype=np.float32)
COUNT_CASES = [(n, C, f) for n in NS for C in CS for f in FAMILIES]


@functools.lru_cache(maxsize=None)
def count_case(n, C, family):
    """(scores float32 [n, C], labels uint8 [n, C], the reference counts), seeded; computed once per session."""
    rng = np.random.default_rng([n, C, FAMILIES.index(family)])
    if family == "continuous":
        s = rng.standard_normal((n, C)).astype(np.float32)
    elif family == "quantised":
        s = (rng.integers(0, 8, size=(n, C)) / 8).astype(np.float32)
    elif family == "equal":
        s = np.full((n, C), 0.25, dtype=np.float32)
    else:
        s = SPECIAL[rng.integers(0, SPECIAL.size, size=(n, C))]
    lab = rng.integers(0, 2, size=(n, C)).astype(np.uint8)
    want = R.rank_counts(s, lab)
    for a in (s, lab, want):
        a.setflags(write=False)
    return s, lab, want


def check_counts(n, C, family):
    from octcubem_amd import ops
    s, lab, want = count_case(n, C, family)
    got = ops.rank_counts(torch.from_numpy(s).to(DEV), torch.from_numpy(lab).to(DEV))
    assert got.dtype == torch.int32 and tuple(got.shape) == (n, C, 4) and got.is_contiguous()
    got = got.cpu().numpy()
    assert np.array_equal(got, want), f"n={n} C={C} {family}: {int((got != want).sum())} counts differ"


@pytest.mark.parametrize("n,C,family", COUNT_CASES)
def test_rank_counts_equal_the_comparison_table(n, C, family):
    check_counts(n, C, family)


def test_special_values_are_all_drawn():
    s, _, _ = count_case(2051, 5, "special")
    assert np.isposinf(s).any() and np.isneginf(s).any() and (np.signbit(s) & (s == 0)).any() and ((s != 0) & (np.abs(s) < 1.2e-38)).any()


@pytest.mark.parametrize("n", (65, 257, 1025))
def test_column_slices_of_wider_buffers(n):
    from octcubem_amd import ops
    rng = np.random.default_rng(n)
    wide_s = (rng.integers(0, 8, size=(n, 7)) / 8).astype(np.float32)
    wide_l = rng.integers(0, 2, size=(n, 9)).astype(np.uint8)
    ds, dl = torch.from_numpy(wide_s).to(DEV), torch.from_numpy(wide_l).to(DEV)
    vs, vl = ds[:, 2:5], dl[:, 1:4]
    assert not vs.is_contiguous() and vs.stride(0) == 7 and vl.stride(0) == 9
    got = ops.rank_counts(vs, vl).cpu().numpy()
    assert np.array_equal(got, R.rank_counts(wide_s[:, 2:5], wide_l[:, 1:4]))
    rows = ops.rank_counts(ds[::2, :3], dl[::2, :3]).cpu().numpy()                 # every second row: stride 14 / 18
    assert np.array_equal(rows, R.rank_counts(wide_s[::2, :3], wide_l[::2, :3]))


@pytest.mark.parametrize("value", (0, 1))
def test_labels_all_zero_and_all_one(value):
    from octcubem_amd import ops
    s, _, _ = count_case(257, 2, "quantised")
    lab = np.full(s.shape, value, dtype=np.uint8)
    got = ops.rank_counts(torch.from_numpy(s).to(DEV), torch.from_numpy(lab).to(DEV)).cpu().numpy()
    assert np.array_equal(got, R.rank_counts(s, lab))
    assert np.array_equal(got[..., 1], got[..., 0] * value) and np.array_equal(got[..., 3], got[..., 2] * value)
    as_bool = ops.rank_counts(torch.from_numpy(s).to(DEV), torch.from_numpy(lab).to(DEV).bool()).cpu().numpy()
    assert np.array_equal(as_bool, got)


def test_bad_arguments_raise():
    from octcubem_amd import ops
    s, lab, _ = count_case(65, 2, "continuous")
    ds, dl = torch.from_numpy(s).to(DEV), torch.from_numpy(lab).to(DEV)
    bad = ds.clone()
    bad[7, 1] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        ops.rank_counts(bad, dl)
    with pytest.raises(Exception):
        ops.rank_counts(torch.from_numpy(s), dl)                                    # a CPU tensor
    with pytest.raises(Exception):
        ops.rank_counts(ds, torch.from_numpy(lab))
    with pytest.raises(Exception):
        ops.rank_counts(ds.double(), dl)
    with pytest.raises(Exception):
        ops.rank_counts(ds.half(), dl)
    with pytest.raises(Exception):
        ops.rank_counts(ds, dl.long())
    with pytest.raises(Exception):
        ops.rank_counts(ds.t().contiguous().t(), dl)                                # column stride n, row stride 1
    with pytest.raises(Exception):
        ops.rank_counts(ds, torch.zeros(65, 4, dtype=torch.uint8, device=DEV)[:, ::2])   # column stride 2
    with pytest.raises(Exception):
        ops.rank_counts(ds, dl[:, :1])                                              # shapes differ
    with pytest.raises(Exception):
        ops.rank_counts(ds[:0], dl[:0])                                             # empty


def test_the_entry_point_refuses_before_any_launch():
    from octcubem_amd import _lib
    out = torch.zeros(4, 1, 4, dtype=torch.int32, device=DEV)
    s = torch.zeros(4, 1, device=DEV)
    lab = torch.zeros(4, 1, dtype=torch.uint8, device=DEV)
    fn = _lib.load().octmae_rank_counts
    for args in ((None, 1, lab.data_ptr(), 1, out.data_ptr(), 4, 1), (s.data_ptr(), 1, None, 1, out.data_ptr(), 4, 1),
                 (s.data_ptr(), 1, lab.data_ptr(), 1, None, 4, 1), (s.data_ptr(), 1, lab.data_ptr(), 1, out.data_ptr(), 0, 1),
                 (s.data_ptr(), 1, lab.data_ptr(), 1, out.data_ptr(), 4, 0), (s.data_ptr(), 1, lab.data_ptr(), 1, out.data_ptr(), 2, 2),
                 (s.data_ptr(), 2, lab.data_ptr(), 1, out.data_ptr(), 2, 2), (s.data_ptr(), 1, lab.data_ptr(), 1, out.data_ptr(), 2 ** 31, 1)):
        assert fn(*args, None) == -2
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0


def test_rank_counts_ignore_autocast():
    from octcubem_amd import ops
    s, lab, want = count_case(257, 2, "continuous")
    with torch.autocast("cuda", dtype=torch.float16):
        got = ops.rank_counts(torch.from_numpy(s).to(DEV), torch.from_numpy(lab).to(DEV))
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------- end to end
N_EVAL, BATCH = 13, 4


def small_vit(num_classes, seed):
    from octcubem_amd import models_vit_st
    torch.manual_seed(seed)
    return models_vit_st.VisionTransformer(num_frames=6, t_patch_size=3, img_size=32, patch_size=16, in_chans=1, num_classes=num_classes,
                                           embed_dim=64, depth=1, num_heads=2, mlp_ratio=4, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
                                           sep_pos_embed=True, cls_embed=True, global_pool=True).to(DEV)


def loader_for(task_mode, num_class):
    """13 samples in batches of 4, 4, 4, 1; every class carries both label values (checked, not assumed)."""
    g = torch.Generator().manual_seed(5)
    x = torch.rand(N_EVAL, 1, 6, 32, 32, generator=g)
    if task_mode == "multi_label":
        t = torch.randint(0, 2, (N_EVAL, num_class), generator=g)
        assert bool(((t.sum(0) > 0) & (t.sum(0) < N_EVAL)).all())
    else:
        t = torch.randint(0, num_class, (N_EVAL,), generator=g)
        assert bool(((torch.bincount(t, minlength=num_class) > 0) & (torch.bincount(t, minlength=num_class) < N_EVAL)).all())
    return [(x[i:i + BATCH], t[i:i + BATCH]) for i in range(0, N_EVAL, BATCH)]


def read_rows(path):
    with open(path, newline="", encoding="utf8") as f:
        return list(csv.reader(f))


MODES = (("binary_cls", 2), ("multi_cls", 3), ("multi_label", 3))


def same(stats_a, roc_a, pr_a, stats_b, roc_b, pr_b):
    """Two passes over the same loader: the loss to 1e-6 (a repeated forward is not promised bit for bit), the rest to 1e-12."""
    return (abs(stats_a["loss"] - stats_b["loss"]) <= 1e-6 and stats_a["acc1"] == stats_b["acc1"] and abs(roc_a - roc_b) <= 1e-12
            and abs(pr_a - pr_b) <= 1e-12)


@pytest.mark.parametrize("task_mode,num_class", MODES)
def test_evaluate_report_end_to_end(task_mode, num_class, tmp_path):
    from octcubem_amd import engine_finetune
    model = small_vit(num_class, seed=11)
    loader = loader_for(task_mode, num_class)
    assert [b[0].shape[0] for b in loader] == [4, 4, 4, 1]
    crit = torch.nn.BCEWithLogitsLoss() if task_mode == "multi_label" else torch.nn.CrossEntropyLoss()
    base = engine_finetune.evaluate(loader, model, torch.device(DEV), crit)
    task = str(tmp_path / "report")
    stats, auc_roc, auc_pr = engine_finetune.evaluate_report(loader, model, torch.device(DEV), task, 3, "test", num_class, criterion=crit,
                                                             task_mode=task_mode)
    print(f"{task_mode}: loss {stats['loss']!r} / {base['loss']!r}, acc1 {stats['acc1']!r} / {base['acc1']!r}, auc_roc {auc_roc!r}, auc_pr {auc_pr!r}")
    assert not model.training and set(stats) == {"loss", "acc1"}
    assert abs(stats["loss"] - base["loss"]) <= 1e-6 and abs(stats["acc1"] - base["acc1"]) <= 1e-6
    logits = base["logits"]
    assert logits.shape == (N_EVAL, num_class) and logits.dtype == torch.float32
    if task_mode == "multi_label":
        scores, onehot = torch.sigmoid(logits).numpy(), base["targets"].numpy()
        want_pr = R.macro(R.auprc, scores, onehot)
    else:
        scores = torch.softmax(logits, dim=1).numpy()
        onehot = torch.nn.functional.one_hot(base["targets"], num_class).numpy()
        want_pr = R.macro(R.average_precision, scores, onehot)
    want_roc = R.macro(R.auroc, scores, onehot)
    print(f"  references: auc_roc {want_roc!r}, auc_pr {want_pr!r}")
    assert abs(auc_roc - want_roc) <= 1e-12 and abs(auc_pr - want_pr) <= 1e-12
    # the files
    if task_mode == "multi_label":
        rows = read_rows(os.path.join(task, "macro_metrics_test.csv"))
        assert rows[0] == engine_finetune.MACRO_HEADER and len(rows) == 2
        vals = dict(zip(rows[0], (float(v) for v in rows[1])))
        assert vals["ROC AUC"] == auc_roc and vals["AUPRC"] == auc_pr and vals["loss"] == stats["loss"]
        for i in range(num_class):
            per = read_rows(os.path.join(task, f"class_{i}_{i}_metrics_test.csv"))
            assert per[0] == engine_finetune.CLASS_HEADER and len(per) == 2
            assert abs(float(per[1][1]) - R.auroc(scores[:, i], onehot[:, i])) <= 1e-12
            cm = np.array(read_rows(os.path.join(task, f"confusion_matrix_test_{i}_{i}_epoch_3.csv")), dtype=np.int64)
            assert cm.shape == (2, 2) and cm.sum() == N_EVAL and cm[1].sum() == int(onehot[:, i].sum())
    else:
        rows = read_rows(os.path.join(task, "metrics_test.csv"))
        assert rows[0] == engine_finetune.METRICS_HEADER and len(rows) == 2
        vals = dict(zip(rows[0], (float(v) for v in rows[1])))
        assert vals["auc_roc"] == auc_roc and vals["auc_pr"] == auc_pr and vals["loss"] == stats["loss"]
        assert abs(vals["acc"] - (1 - 2 * (1 - stats["acc1"]) / num_class)) <= 1e-6      # the mean one-vs-rest accuracy
        cm = np.array(read_rows(os.path.join(task, "confusion_matrix_test_epoch_3.csv")), dtype=np.int64)
        assert cm.shape == (num_class, num_class) and cm.sum() == N_EVAL
        assert np.array_equal(cm.sum(1), np.bincount(base["targets"].numpy(), minlength=num_class))
        assert abs(np.trace(cm) / N_EVAL - stats["acc1"]) <= 1e-12
    # a second call appends a row and keeps one header; return_bal_acc pairs the third value
    stats2, roc2, (pr2, bal) = engine_finetune.evaluate_report(loader, model, torch.device(DEV), task, 4, "test", num_class, criterion=crit,
                                                               task_mode=task_mode, return_bal_acc=True)
    assert same(stats2, roc2, pr2, stats, auc_roc, auc_pr) and 0.0 <= bal <= 1.0
    rows = read_rows(os.path.join(task, "macro_metrics_test.csv" if task_mode == "multi_label" else "metrics_test.csv"))
    assert len(rows) == 3 and rows[0][0] != rows[1][0] and len(rows[2]) == len(rows[1])
    np.testing.assert_allclose([float(v) for v in rows[2]], [float(v) for v in rows[1]], rtol=0, atol=1e-6)
    # the same inside an autocast context
    with torch.autocast("cuda", dtype=torch.float16):
        stats3, roc3, pr3 = engine_finetune.evaluate_report(loader, model, torch.device(DEV), str(tmp_path / "ac"), 0, "val", num_class,
                                                            criterion=crit, task_mode=task_mode)
    assert same(stats3, roc3, pr3, stats, auc_roc, auc_pr)
    assert not any(f.startswith("confusion_matrix") for f in os.listdir(str(tmp_path / "ac")))       # not a test mode


def test_evaluate_report_raises_when_a_class_is_missing(tmp_path):
    from octcubem_amd import engine_finetune
    model = small_vit(3, seed=11)
    g = torch.Generator().manual_seed(5)
    loader = [(torch.rand(4, 1, 6, 32, 32, generator=g), torch.tensor([0, 1, 0, 1]))]           # class 2 never occurs
    with pytest.raises(ValueError):
        engine_finetune.evaluate_report(loader, model, torch.device(DEV), str(tmp_path), 0, "val", 3, task_mode="multi_cls")


# ---------------------------------------------------------------------------------------------- the half build
def half_build_cases():
    """What tests/f16_worker.py runs on the half-operand build."""
    for case in COUNT_CASES:
        check_counts(*case)
    return {"passed": [list(c) for c in COUNT_CASES]}


def start_children():
    """tests/conftest.py calls this once the collection holds a test of this module, before this process has touched the GPU;
    tests/children.py releases the worker when the GPU has room for it."""
    if os.path.exists(LIB_F16):
        children.spawn_f16_worker("metrics_f16", "tests.test_gpu_metrics:half_build_cases")


def test_half_build_runs_the_same_rank_count_kernel():
    """The entry point has no 16-bit operand: liboctmae_f16.so must give the same counts on every count case."""
    assert os.path.exists(LIB_F16), "make -C octcubem_amd/csrc both"
    start_children()
    res = children.f16_worker_result("metrics_f16")
    assert res["lib"] == "liboctmae_f16.so" and res["lp_is_f16"] is True
    assert res["passed"] == [list(c) for c in COUNT_CASES], res
