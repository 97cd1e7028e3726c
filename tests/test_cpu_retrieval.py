"""CPU tests of the COEM validation metrics (octcubem_amd/coem.py: get_metrics, get_metrics_3modalities, get_corrected_metrics).

The host finish is fed with counts from the numpy restatement (tests/retrieval_ref.py) through ``ranks=`` and must equal the values the
REFERENCE's own functions gave on the same seeded problems (tests/golden/retrieval_small.npz, written by tools/gen_golden_retrieval.py,
which asserts that no two scores of a row lie within 1e-5 of each other, and none within 1e-5 of 0 where the sign is used: the order is then the same in f32 and float64, scaled or
not, and ties play no part).  Tolerance 1e-12: the finish is a float64 mean of at most 41 integers, the reference's own expression."""
import functools
import re
import os
import zlib

import numpy as np
import pytest
import torch

from tests import retrieval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "retrieval_small.npz")
N_GOLDEN = 3
MIN_GAP = 1e-5
SEEDS = (5, 713, 0)      # the first seeds whose problems pass the gap assertions of tools/gen_golden_retrieval.py


def _normalize(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def row_gap(s):
    """the smallest distance between two scores of one row of s"""
    return float(np.diff(np.sort(s, axis=1), axis=1).min())


@functools.lru_cache(maxsize=None)
def golden_problem(k):
    """k = 0: get_metrics (N = 40, D = 8); 1: get_metrics_3modalities (N = 41, presence weights with zeros); 2: get_corrected_metrics
    (N = 40 images over 12 reports, string labels).  Seeded; tools/gen_golden_retrieval.py asserts the gaps."""
    rng = np.random.default_rng([SEEDS[k], k, 7])
    if k == 0:
        img = _normalize(rng.standard_normal((40, 8)))
        txt = _normalize(0.6 * img + 0.5 * rng.standard_normal((40, 8)))
        return {"image": img, "text": txt, "logit_scale": np.float32(1 / 0.07)}
    if k == 1:
        img = _normalize(rng.standard_normal((41, 8)))
        t1 = _normalize(0.6 * img + 0.5 * rng.standard_normal((41, 8)))
        t2 = _normalize(0.4 * img + 0.6 * rng.standard_normal((41, 8)))
        w1 = (rng.random(41) < 0.7).astype(np.float32)
        w2 = (rng.random(41) < 0.5).astype(np.float32)
        return {"image": img, "text1": t1, "text2": t2, "w1": w1, "w2": w2, "logit_scale": np.float32(1 / 0.07),
                "logit_scale1": np.float32(20.0), "logit_scale2": np.float32(5.5)}
    which = rng.integers(0, 12, size=40)
    which[:12] = np.arange(12)                      # every report occurs
    reports = _normalize(rng.standard_normal((12, 8)))
    img = _normalize(0.7 * reports[which] + 0.5 * rng.standard_normal((40, 8)))
    return {"image": img, "text": reports[which].copy(), "labels": tuple(f"report-{int(w):02d}" for w in which),
            "logit_scale": np.float32(1 / 0.07)}


def crc(p):
    c = 0
    for key in sorted(p):
        v = p[key]
        c = zlib.crc32("|".join(v).encode() if isinstance(v, tuple) else np.ascontiguousarray(v).tobytes(), c)
    return c


def golden():
    return np.load(GOLDEN)


def expected(g, k):
    return {key.split("/", 1)[1]: float(g[key]) for key in g.files if key.startswith(f"p{k}/")}


def t(x):
    return torch.from_numpy(np.asarray(x))


def run(k, ranks):
    from octcubem_amd import coem
    p = golden_problem(k)
    if k == 0:
        return coem.get_metrics(t(p["image"]), t(p["text"]), t(p["logit_scale"]), ranks=ranks)
    if k == 1:
        return coem.get_metrics_3modalities(t(p["image"]), t(p["text1"]), t(p["text2"]), t(p["logit_scale"]), t(p["logit_scale1"]),
                                            t(p["logit_scale2"]), t(p["w1"]), t(p["w2"]), ranks=ranks)
    return coem.get_corrected_metrics(t(p["image"]), t(p["text"]), t(p["logit_scale"]), list(p["labels"]), ranks=ranks)


def assert_close(got, want, tol=1e-12):
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    for key in want:
        assert abs(float(got[key]) - want[key]) <= tol, (key, got[key], want[key])


@pytest.mark.parametrize("k", range(N_GOLDEN))
def test_inputs_are_the_recorded_ones(k):
    assert int(golden()[f"crc_{k}"]) == crc(golden_problem(k))


@pytest.mark.parametrize("k", range(N_GOLDEN))
def test_host_finish_equals_the_reference(k):
    want = expected(golden(), k)
    assert len(want) == (10, 30, 7)[k]
    assert_close(run(k, R.ranks_from()), want)


@pytest.mark.parametrize("k", range(N_GOLDEN))
def test_restatement_equals_the_reference(k):
    """tests/retrieval_ref.py's own formulas (torch.argsort(stable=True) on the CPU) are pinned to the same fixture."""
    p = golden_problem(k)
    if k == 0:
        got = R.get_metrics(p["image"], p["text"])
    elif k == 1:
        got = R.get_metrics_3modalities(p["image"], p["text1"], p["text2"], p["w1"], p["w2"])
    else:
        got = R.get_corrected_metrics(p["image"], p["text"], p["labels"])
    assert_close(got, expected(golden(), k))


def test_counts_give_the_stable_sort_position_with_ties():
    rng = np.random.default_rng(3)
    s = rng.integers(-2, 3, size=(37, 23)).astype(np.float32)          # ties in every row
    target = rng.integers(0, 23, size=37)
    c = R.counts(s, target)
    assert np.array_equal(c[:, 0] + c[:, 1], R.stable_preds(s, target)) and (c[:, 1] > 0).any()


def test_t_weight_filter_and_empty_direction():
    from octcubem_amd import coem
    p = golden_problem(1)
    args = [t(p[key]) for key in ("image", "text1", "text2", "logit_scale", "logit_scale1", "logit_scale2")]
    ones = torch.ones(41)
    full = coem.get_metrics_3modalities(*args, ones, ones, ranks=R.ranks_from())
    pair = coem.get_metrics(t(p["image"]), t(p["text1"]), 1.0, ranks=R.ranks_from())
    for key, v in pair.items():                                         # all present: the two-modality metrics of each pair
        assert full[key.replace("text", "text1")] == v
    w1 = torch.zeros(41); w1[[3, 17]] = 2.5                               # any positive weight counts, as a flag
    got = coem.get_metrics_3modalities(*args, w1, ones, ranks=R.ranks_from())
    preds = R.stable_preds(R.f64_scores(p["image"], p["text1"]))[[3, 17]]
    assert got["image_to_text1_mean_rank"] == preds.mean() + 1 and got["image_to_text1_R@1"] == np.mean(preds < 1)
    assert got["image_to_text2_mean_rank"] == full["image_to_text2_mean_rank"]
    with pytest.raises(ValueError, match="text1"):
        coem.get_metrics_3modalities(*args, torch.zeros(41), ones, ranks=R.ranks_from())
    w2 = torch.ones(41); w2[[3, 17]] = 0                                  # each modality has samples, the pair has none
    with pytest.raises(ValueError, match="text1_to_text2"):
        coem.get_metrics_3modalities(*args, w1, w2, ranks=R.ranks_from())


def test_label_mapping():
    from octcubem_amd import coem
    ids, last = coem._label_ids(["b", "a", "b", ("c", 1), "a", "b"])
    assert ids.tolist() == [0, 1, 0, 2, 1, 0] and last.tolist() == [5, 4, 5, 3, 4, 5] and ids.dtype == np.int32 and last.dtype == np.int32
    ids, last = coem._label_ids(torch.tensor([7, 7, 3]))
    assert ids.tolist() == [0, 0, 1] and last.tolist() == [1, 1, 2]
    # the mapping is what the kernel is asked for: keep = the last occurrences, target = the sample's own
    seen = {}

    def spy(a, b, target=None, keep=None, row_group=None, col_group=None):
        seen.update(target=target.tolist(), keep=keep.tolist(), rg=row_group.tolist(), cg=col_group.tolist())
        return R.ranks_from()(a, b, target, keep, row_group, col_group)
    p = golden_problem(0)
    labels = ["x"] * 20 + [f"u{i}" for i in range(20)]
    coem.get_corrected_metrics(t(p["image"]), t(p["text"]), 2.0, labels, ranks=spy)
    assert seen["target"] == [19] * 20 + list(range(20, 40)) and seen["keep"] == [0] * 19 + [1] * 21
    assert seen["rg"] == seen["cg"] == [0] * 20 + list(range(1, 21))


def test_logit_scale_must_be_positive_and_finite():
    from octcubem_amd import coem
    p = golden_problem(0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="logit_scale"):
            coem.get_metrics(t(p["image"]), t(p["text"]), bad, ranks=R.ranks_from())
    a = coem.get_metrics(t(p["image"]), t(p["text"]), 0.5, ranks=R.ranks_from())
    assert a == coem.get_metrics(t(p["image"]), t(p["text"]), 100.0, ranks=R.ranks_from())


def test_cpu_features_without_a_ranks_function_raise():
    from octcubem_amd import coem
    p = golden_problem(0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        coem.get_metrics(t(p["image"]), t(p["text"]), 1.0)


def test_evaluate_refuses_other_multimodal_types_and_skips_when_not_due():
    import types
    from octcubem_amd import coem
    args = types.SimpleNamespace(multimodal_type="oct_faf_ir", val_frequency=1, epochs=2, device="cpu")
    with pytest.raises(NotImplementedError, match="oct_faf_ir"):
        coem.evaluate(torch.nn.Identity(), {}, 1, args)
    args.multimodal_type = "default"
    assert coem.evaluate(torch.nn.Identity(), {}, 1, args) == {}                                   # no 'val'
    args.val_frequency = 2
    assert coem.evaluate(torch.nn.Identity(), {"val": None}, 1, args) == {}                        # not due at epoch 1 of 2 .. every 2


def test_abi_declares_retrieval_ranks():
    from octcubem_amd import _lib
    header = open(os.path.join(ROOT, "include", "octmae.h")).read()
    assert re.search(r"^int octmae_retrieval_ranks\(", header, re.M)
    assert "octmae_retrieval_ranks" in _lib.SIGNATURES and len(_lib.SIGNATURES["octmae_retrieval_ranks"]) == 13
    assert _lib.expected_abi_version() >= 19                 # 18 before this entry point
    assert re.search(r"^ \* 19: octmae_retrieval_ranks", header, re.M)
    mk = open(os.path.join(ROOT, "octcubem_amd", "csrc", "Makefile")).read()
    assert "retrieval.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1)


def test_restated_plan_follows_the_kernel_constants_and_the_trip_shapes_lie_past_the_split():
    """Whoever changes a constant of the tile (csrc/simtile.hpp) or the cap that csrc/retrieval.hip hands its split rule is told here
    to move R.TRIP_SHAPES (tests/test_gpu_retrieval.py runs them)."""
    src = open(os.path.join(ROOT, "octcubem_amd", "csrc", "retrieval.hip")).read()
    tile = open(os.path.join(ROOT, "octcubem_amd", "csrc", "simtile.hpp")).read()
    const = lambda name: int(re.search(rf"^constexpr int {name} = (\d+);", tile, re.M).group(1))
    assert '#include "simtile.hpp"' in src and not re.search(r"^constexpr int RR_", src, re.M)     # the file has no tile of its own
    assert const("SIM_ROWS") == const("SIM_COLS") == R.TILE and const("SIM_TARGET_WGS") == R.TARGET_WGS
    # sim_split as written: ceil(target / row_blocks), then the two caps; this file's cap is the grid's y
    assert re.search(r"long long split = \(SIM_TARGET_WGS \+ row_blocks - 1\) / row_blocks;\s*if \(split > col_tiles\) split = col_tiles;\s*"
                     r"if \(split > cap\) split = cap;", tile)
    assert re.search(rf"const long long split = sim_split\(row_blocks, col_tiles, {R.MAX_GRID_Y}\);", src)
    assert R.plan(1, 1) == (1, 1, 1) and R.plan(131, 131) == (3, 3, 3) and R.plan(64, 70000) == (1, 1094, 1024)
    for (n, m, d), want in zip(R.TRIP_SHAPES, R.TRIP_PLANS):
        assert R.plan(n, m) == want, (n, m, R.plan(n, m))
        assert want[1] > want[2]                                   # more tiles than workgroups to walk them: a second trip
    assert R.TRIP_PLANS[2][2] == 1 and R.TRIP_PLANS[0][2] == R.TARGET_WGS
    # no other size of the GPU module leaves a workgroup more than one tile
    for n in (1, 2, 63, 64, 65, 131):
        for m in (1, 2, 63, 64, 65, 131):
            assert R.plan(n, m)[1] == R.plan(n, m)[2]
