"""CPU tests of the validation loops for the dict-batch recipes (octcubem_amd/coem.py: evaluate_3modalities, evaluate_multimodal) and of
the ``pair_ranks=`` path of the metric functions.

The loops run on the CPU -- the ranks from the numpy restatement (tests/pair_ranks_ref.py) through ``pair_ranks=`` -- on one small seeded
problem and must reproduce what the REFERENCE's own ``evaluate`` functions returned on it (tests/golden/eval3mod_small.npz, written by
tools/gen_golden_eval3mod.py): train_retclip_3modalities.evaluate for 'oct_faf_ir', train_retclip.evaluate for 'oct_ir'.  The problem:
N = 41 in batches of 16, 16 and 9, D = 8, presence weights with zeros, the last batch without any FAF (the zero branch of the loss);
recorded with ``correct_label`` 0 and 1, and for 1 two IR rows of the first batch are bit copies (so the same-feature targets are not
the identity).  The two copies are absent IR samples (w1 = 0), which is what makes them copies in a real loader -- an absent modality is
one placeholder image -- and what keeps the reference's unstable argsort out of the fixture: no REPORTED rank has a tie.  The tool
asserts the row-gap condition of tools/gen_golden_retrieval.py (MIN_GAP of tests/test_cpu_retrieval.py) on all three products and their
transposes, with the second copy left out of the IR products.

Limits.  Rank metrics: equal (float64 means of at most 41 integers, the reference's own expressions).  ``val_loss``:
1e-6 * max(1, |want|) -- the same float32 arithmetic on the same CPU, the limit tests/test_gpu_retrieval.py::test_evaluate_end_to_end uses."""
import functools
import os
import re
import types
import zlib

import numpy as np
import pytest
import torch

from tests import eval3mod_ref as E
from tests import pair_ranks_ref as PR
from tests import retrieval_ref as R
from tests import test_cpu_retrieval as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval3mod_small.npz")
BATCHES = (16, 16, 9)
N, D = sum(BATCHES), 8
SEED = 10                # the first seed whose problem passes the assertions of tools/gen_golden_eval3mod.py
COPY = (3, 7)            # correct_label = 1: IR row 7 is a bit copy of IR row 3 (both in the first batch, both absent: w1 = 0)
SCALES = (np.float32(1 / 0.07), np.float32(20.0), np.float32(5.5))


@functools.lru_cache(maxsize=None)
def problem(correct_label):
    rng = np.random.default_rng([SEED, 3, 41])
    img = G._normalize(rng.standard_normal((N, D)))
    ir = G._normalize(0.6 * img + 0.5 * rng.standard_normal((N, D)))
    faf = G._normalize(0.4 * img + 0.6 * rng.standard_normal((N, D)))
    w1 = (rng.random(N) < 0.7).astype(np.float32)
    w2 = (rng.random(N) < 0.6).astype(np.float32)
    w2[sum(BATCHES[:2]):] = 0                                             # the last batch has no FAF at all
    w1[[0, 20, 35]], w2[[0, 20]] = 1, 1                                   # every batch reports something
    if correct_label:
        ir[COPY[1]] = ir[COPY[0]]
        w1[list(COPY)] = 0
        w2[list(COPY)] = 1                                                # ... and the image / FAF terms see the doubled targets
    p = {"image": img, "ir": ir, "faf": faf, "w1": w1, "w2": w2}
    for v in p.values():
        v.setflags(write=False)
    return p


def crc(p):
    c = 0
    for key in sorted(p):
        c = zlib.crc32(np.ascontiguousarray(p[key]).tobytes(), c)
    return c


class Echo(torch.nn.Module):
    """The stub model of the fixture: the 'inputs' are the seeded, normalised features themselves."""

    def forward(self, image, text1, text2=None):
        s = [torch.tensor(float(v), dtype=torch.float32) for v in SCALES]
        return (image, text1, s[0]) if text2 is None else (image, text1, text2, s[0], s[1], s[2])


class Loader(list):
    pass


def loader(p):
    items, i = Loader(), 0
    for bsz in BATCHES:
        sl = slice(i, i + bsz)
        x = {"oct": torch.from_numpy(p["image"][sl].copy()), "ir": torch.from_numpy(p["ir"][sl].copy()),
             "f2_faf": torch.from_numpy(p["faf"][sl].copy())}
        flags = [torch.ones(bsz, dtype=torch.int64), torch.from_numpy(p["w1"][sl].astype(np.int64)), torch.from_numpy(p["w2"][sl].astype(np.int64))]
        items.append((x, ([f"s{k}" for k in range(i, i + bsz)], [0] * bsz, flags, None)))
        i += bsz
    items.num_samples = N
    return items


def eval_args(mm, correct_label, **kw):
    base = dict(device="cpu", val_frequency=1, epochs=4, save_logs=False, save_retrieval_results=False, multimodal_type=mm,
                return_metainfo=False, correct_label=correct_label, precision="amp", wandb=False, rank=0)
    base.update(kw)
    return types.SimpleNamespace(**base)


def golden():
    return np.load(GOLDEN)


def expected(g, prefix):
    return {key.split("/", 1)[1]: float(g[key]) for key in g.files if key.startswith(prefix + "/")}


def assert_equals_the_reference(got, want):
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    for key, v in want.items():
        if key == "val_loss":
            print(f"val_loss {got[key]!r} / {v!r}")
            assert abs(got[key] - v) <= 1e-6 * max(1.0, abs(v)), (got[key], v)
        else:
            assert got[key] == v, (key, got[key], v)


@pytest.mark.parametrize("cl", (0, 1))
def test_inputs_are_the_recorded_ones(cl):
    assert int(golden()[f"crc_{cl}"]) == crc(problem(cl))
    p = problem(cl)
    assert (p["w1"] == 0).any() and (p["w2"][:32] == 0).any() and not p["w2"][32:].any() and p["w1"][32:].any()
    assert np.array_equal(p["ir"][COPY[0]], p["ir"][COPY[1]]) == bool(cl)


@pytest.mark.parametrize("cl", (0, 1))
def test_three_modality_loop_equals_the_reference(cl):
    from octcubem_amd import coem
    model = Echo().train()
    got = coem.evaluate_3modalities(model, {"val": types.SimpleNamespace(dataloader=loader(problem(cl)))}, 2, eval_args("oct_faf_ir", cl),
                                    pair_ranks=PR.pair_ranks_from())
    want = expected(golden(), f"three{cl}")
    assert len(want) == 33 and want["epoch"] == 2 and want["num_samples"] == N and not model.training
    assert_equals_the_reference(got, want)


@pytest.mark.parametrize("cl", (0, 1))
def test_oct_ir_loop_equals_the_reference(cl):
    """the two-tower dict-batch loop, on the copy-free features (a copy would tie with the partner in an UNFILTERED ranking)"""
    from octcubem_amd import coem
    got = coem.evaluate_multimodal(Echo(), {"val": types.SimpleNamespace(dataloader=loader(problem(0)))}, 2, eval_args("oct_ir", cl),
                                   pair_ranks=PR.pair_ranks_from())
    want = expected(golden(), f"oct_ir{cl}")
    assert len(want) == 13
    assert_equals_the_reference(got, want)


def ref_batches(p):
    out, i = [], 0
    for bsz in BATCHES:
        sl = slice(i, i + bsz)
        out.append((p["image"][sl], p["ir"][sl], p["faf"][sl]) + SCALES + (p["w1"][sl], p["w2"][sl]))
        i += bsz
    return out


@pytest.mark.parametrize("cl", (0, 1))
def test_restatement_equals_the_reference(cl):
    p = problem(cl)
    want = expected(golden(), f"three{cl}")
    got = R.get_metrics_3modalities(p["image"], p["ir"], p["faf"], p["w1"], p["w2"])
    for key, v in got.items():
        assert v == want[key], (key, v, want[key])
    loss = E.val_loss(ref_batches(p), correct_label=bool(cl))
    print(f"val_loss float64 {loss!r} / reference float32 {want['val_loss']!r}")
    assert abs(loss - want["val_loss"]) <= 1e-6 * max(1.0, abs(want["val_loss"]))


@pytest.mark.parametrize("cl", (0, 1))
def test_the_text_pair_is_weighted_by_w1_alone(cl):
    """train_retclip_3modalities.py:451-463 weights the IR / FAF terms by w1, not by w1 * w2 as ThreeModalityClipLoss does: on the
    recorded problem the other choice gives another val_loss, far outside the limit, so the detail cannot be lost silently."""
    p = problem(cl)
    want = expected(golden(), f"three{cl}")["val_loss"]
    other = E.val_loss(ref_batches(p), correct_label=bool(cl), text_pair_weight="w1w2")
    assert abs(other - want) > 1e-3 * max(1.0, abs(want)), (other, want)
    assert (p["w1"] * p["w2"] != p["w1"]).any()


def test_zero_weight_sum_gives_zero_without_a_division():
    from octcubem_amd import coem
    p = problem(0)
    sl = slice(32, 41)
    f = [torch.from_numpy(p[k][sl].copy()) for k in ("image", "ir", "faf")]
    s = [torch.tensor(float(v)) for v in SCALES]
    w1, zero = torch.from_numpy(p["w1"][sl].copy()), torch.zeros(9)
    got = coem.three_way_val_loss(*f, *s, w1, zero)
    assert torch.isfinite(got) and abs(float(got) - E.batch_loss(*f, *SCALES, w1, zero)) <= 1e-6
    assert float(coem.three_way_val_loss(*f, *s, zero, zero)) == 0.0
    # weights that cancel: the reference tests the SUM, and so does the loop
    assert float(coem.three_way_val_loss(*f, *s, torch.tensor([1.0, -1.0] + [0.0] * 7), zero)) == 0.0


@pytest.mark.parametrize("k", (0, 1))
def test_pair_ranks_gives_the_metrics_of_ranks(k):
    from octcubem_amd import coem
    p, t = G.golden_problem(k), G.t
    if k == 0:
        args = (t(p["image"]), t(p["text"]), t(p["logit_scale"]))
        fn = coem.get_metrics
    else:
        args = (t(p["image"]), t(p["text1"]), t(p["text2"]), t(p["logit_scale"]), t(p["logit_scale1"]), t(p["logit_scale2"]), t(p["w1"]), t(p["w2"]))
        fn = coem.get_metrics_3modalities
    calls = []

    def spy(pairs):
        calls.append(len(pairs))
        return PR.pair_ranks_from()(pairs)
    got = fn(*args, pair_ranks=spy)
    assert got == fn(*args, ranks=R.ranks_from()) and calls == [(1, 3)[k]]            # one call for all directions
    G.assert_close(got, G.expected(G.golden(), k))
    with pytest.raises(ValueError, match="not both"):
        fn(*args, ranks=R.ranks_from(), pair_ranks=spy)
    with pytest.raises(ValueError, match="pair_ranks returned"):
        fn(*args, pair_ranks=lambda pairs: np.zeros((len(pairs), 2, 5, 2), dtype=np.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        coem._device_pair_ranks([(args[0], args[1])])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(*args)                                                                     # the default is untouched


def test_pair_counts_are_the_counts_of_the_matrix_and_of_its_transpose():
    rng = np.random.default_rng(4)
    s = rng.integers(-2, 3, size=(37, 37)).astype(np.float32)                        # ties in every row and column
    c = PR.pair_counts([s, s.T])
    assert c.shape == (2, 2, 37, 2) and np.array_equal(c[0, 0], c[1, 1]) and np.array_equal(c[0, 1], c[1, 0])
    assert np.array_equal(c[0, 0].sum(1), R.stable_preds(s)) and np.array_equal(c[0, 1].sum(1), R.stable_preds(s.T))
    assert (c[..., 1] > 0).any() and not np.array_equal(c[0, 0], c[0, 1])


def test_dispatch_table(monkeypatch):
    from octcubem_amd import coem
    seen = []
    monkeypatch.setattr(coem, "evaluate", lambda *a, **k: seen.append(("evaluate", a, k)) or {"who": "evaluate"})
    monkeypatch.setattr(coem, "evaluate_3modalities", lambda *a, **k: seen.append(("three", a, k)) or {"who": "three"})
    monkeypatch.setattr(coem, "_evaluate_dict_batches", lambda *a, **k: seen.append(("dict", a, k)) or {"who": "dict"})
    model, data, tb, pr = object(), {"val": None}, object(), object()
    for mm, who in ((None, "evaluate"), ("default", "evaluate"), ("oct_ir", "dict"), ("oct_faf_only", "dict"), ("oct_faf_ir", "three")):
        assert coem.evaluate_multimodal(model, data, 3, eval_args(mm, 0), tb, pr) == {"who": who}
    assert [s[0] for s in seen] == ["evaluate", "evaluate", "dict", "dict", "three"]
    assert seen[0][1][:3] == (model, data, 3) and seen[0][1][4] is tb and pr not in seen[0][1]     # evaluate: its own signature
    assert seen[2][1][1] == "oct_ir" and seen[3][1][1] == "oct_faf_only" and seen[2][1][-1] is pr and seen[4][1][-1] is pr
    for mm in ("oct_f2_faf_inplace", "something"):
        with pytest.raises(NotImplementedError, match=mm):
            coem.evaluate_multimodal(model, data, 3, eval_args(mm, 0))
    assert len(seen) == 5
    args = types.SimpleNamespace(device="cpu", val_frequency=1, epochs=4)              # no multimodal_type at all: 'default'
    assert coem.evaluate_multimodal(model, data, 3, args) == {"who": "evaluate"}


def test_oct_faf_only_asserts_that_every_faf_flag_is_set():
    from octcubem_amd import coem
    p = dict(problem(0))
    data = {"val": types.SimpleNamespace(dataloader=loader(p))}
    with pytest.raises(AssertionError, match="Only f2_faf"):
        coem.evaluate_multimodal(Echo(), data, 1, eval_args("oct_faf_only", 0), pair_ranks=PR.pair_ranks_from())
    p["w2"] = np.ones(N, dtype=np.float32)
    data = {"val": types.SimpleNamespace(dataloader=loader(p))}
    got = coem.evaluate_multimodal(Echo(), data, 1, eval_args("oct_faf_only", 0), pair_ranks=PR.pair_ranks_from())
    want = R.get_metrics(p["image"], p["faf"])
    assert {k: v for k, v in got.items() if k in want} == {k: float(v) for k, v in want.items()} and got["num_samples"] == N


def test_not_due_and_not_the_main_process_return_nothing(monkeypatch):
    from octcubem_amd import coem, misc
    data = {"val": types.SimpleNamespace(dataloader=loader(problem(0)))}
    for fn, mm in ((coem.evaluate_3modalities, "oct_faf_ir"), (coem.evaluate_multimodal, "oct_faf_ir"), (coem.evaluate_multimodal, "oct_ir")):
        assert fn(Echo(), data, 1, eval_args(mm, 0, val_frequency=2)) == {}            # not due at epoch 1 of 4, every 2
        assert fn(Echo(), data, 1, eval_args(mm, 0, val_frequency=0)) == {}
        assert fn(Echo(), {}, 2, eval_args(mm, 0)) == {}                               # no 'val'
        assert fn(Echo(), data, 4, eval_args(mm, 0, val_frequency=3), pair_ranks=PR.pair_ranks_from()) != {}     # the last epoch is due
    monkeypatch.setattr(misc, "is_main_process", lambda: False)
    for fn, mm in ((coem.evaluate_3modalities, "oct_faf_ir"), (coem.evaluate_multimodal, "oct_ir"), (coem.evaluate_multimodal, "bogus")):
        assert fn(Echo(), data, 2, eval_args(mm, 0)) == {}


def test_empty_loader_raises_and_files_are_written(tmp_path):
    import json
    from octcubem_amd import coem
    empty = Loader()
    empty.num_samples = 0
    with pytest.raises(ValueError, match="empty"):
        coem.evaluate_3modalities(Echo(), {"val": types.SimpleNamespace(dataloader=empty)}, 1, eval_args("oct_faf_ir", 0))
    p = problem(0)
    scalars = []
    tb = types.SimpleNamespace(add_scalar=lambda name, val, step: scalars.append((name, val, step)))
    args = eval_args("oct_faf_ir", 0, save_logs=True, save_retrieval_results=True, checkpoint_path=str(tmp_path))
    got = coem.evaluate_3modalities(Echo(), {"val": types.SimpleNamespace(dataloader=loader(p))}, 2, args, tb_writer=tb,
                                    pair_ranks=PR.pair_ranks_from())
    lines = open(os.path.join(str(tmp_path), "results.jsonl")).read().splitlines()
    assert len(lines) == 1 and json.loads(lines[0]) == got and len(got) == 33
    assert sorted(scalars) == sorted((f"val/{k}", v, 2) for k, v in got.items())
    z = np.load(os.path.join(str(tmp_path), "retrieval_results_2.npz"))
    assert set(z.files) == {"image_features", "text1_features", "text2_features", "t_weight1", "t_weight2", "logit_scale"}
    assert np.array_equal(z["image_features"], p["image"]) and np.array_equal(z["text1_features"], p["ir"])
    assert np.array_equal(z["text2_features"], p["faf"]) and np.array_equal(z["t_weight1"], p["w1"]) and np.array_equal(z["t_weight2"], p["w2"])
    assert z["logit_scale"].shape == (3, 3) and np.array_equal(z["logit_scale"], np.tile(np.asarray(SCALES, dtype=np.float32), (3, 1)))


def test_default_of_the_loops_is_a_module_constant():
    from octcubem_amd import coem
    assert isinstance(coem.PAIR_RANKS_DEFAULT, bool)
    fn = lambda pairs: None
    assert coem._pair_ranks_arg(fn) is fn and coem._pair_ranks_arg(False) is None and coem._pair_ranks_arg(True) is coem._device_pair_ranks
    assert coem._pair_ranks_arg(None) is (coem._device_pair_ranks if coem.PAIR_RANKS_DEFAULT else None)


def test_abi_declares_the_pair_entry_points():
    from octcubem_amd import _lib
    header = open(os.path.join(ROOT, "include", "octmae.h")).read()
    assert re.search(r"^int octmae_retrieval_pair_ranks\(", header, re.M)
    assert re.search(r"^long long int octmae_retrieval_pair_ws\(", header, re.M)
    decl = re.search(r"^int octmae_retrieval_pair_ranks\(([^;]*)\);", header, re.M | re.S)
    assert len(_lib.SIGNATURES["octmae_retrieval_pair_ranks"]) == decl.group(1).count(",") + 1 == 19
    assert len(_lib.SIGNATURES["octmae_retrieval_pair_ws"]) == 2 and _lib.RESTYPES["octmae_retrieval_pair_ws"] is _lib._ll
    assert _lib.expected_abi_version() >= 32 and re.search(r"^ \* 32: octmae_retrieval_pair_ranks", header, re.M)
    mk = open(os.path.join(ROOT, "octcubem_amd", "csrc", "Makefile")).read()
    assert "retrieval_pair.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1)
    src = open(os.path.join(ROOT, "octcubem_amd", "csrc", "retrieval_pair.hip")).read()
    assert '#include "simtile.hpp"' in src and "sim_split(" in src and "SIM_SCORE_TILE(" in src and "SIM_TARGET_CHAIN(" in src
