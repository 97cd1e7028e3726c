"""tests/optim_ref.py on the CPU: the per-element bounds that tests/test_gpu_optim_kernels.py applies to csrc/optim.hip hold for the
kernel's arithmetic done correctly (emulate_step_f32: numpy float32 in the kernel's operation order, on the inputs the GPU tests
draw), and every planted mutant of that arithmetic breaks at least one bound or exact check -- the bounds are neither too tight nor
vacuous."""
import itertools

import numpy as np
import pytest

from tests import optim_ref as R

HP = dict(lr=R.LR, eps=1e-8)
GSCALES = [None, 0.37, 2.0 ** -16]
BETAS = [(0.9, 0.95), (0.9, 0.999)]
WDS = [0.0, 0.05]


def _violations(got, ref, g_raw, where):
    """bounds on p, m, v (per element) and on sumsq of one emulated step -> list of messages"""
    p1, m1, v1, sq = got
    bad = []
    try:
        R.check_step(p1, m1, v1, ref, where)
    except AssertionError as e:
        bad.append(str(e))
    sr = R.sumsq_ref(g_raw)
    if abs(sq - sr) > R.sumsq_factor(g_raw.size) * R.E * sr:
        bad.append(f"{where}sumsq {sq!r} vs {sr!r}: {abs(sq - sr) / (R.E * sr):.1f} e, bound {R.sumsq_factor(g_raw.size)} e")
    return bad


def _run(gs, betas, wd, lengths, mutant=None):
    """three steps; the state always advances with the CORRECT emulation (as the kernel's own state does on the GPU), the mutant is
    applied to each step from that state.  -> (violations, worst ratios)"""
    ps, gsteps = R.draw(lengths, 1, gs)
    ms = [np.zeros_like(p) for p in ps]
    vs = [np.zeros_like(p) for p in ps]
    bad, ratio = [], {"p": 0.0, "m": 0.0, "v": 0.0}
    for step in (1, 2, 3):
        for i, n in enumerate(lengths):
            args = (ps[i], gsteps[step - 1][i], ms[i], vs[i], gs, step, HP["lr"], betas[0], betas[1], HP["eps"], wd)
            ref = R.ref_step(*args)
            good = R.emulate_step_f32(*args)
            got = good if mutant is None else R.emulate_step_f32(*args, mutant=mutant)
            bad += _violations(got, ref, gsteps[step - 1][i], f"step {step} n {n}: ")
            for k, a in zip("pmv", got[:3]):
                ratio[k] = max(ratio[k], R.worst(a, ref[k], ref["b" + k])[0])
            ps[i], ms[i], vs[i] = good[:3]
    return bad, ratio


def test_sweep_table_covers_every_length_and_index():
    cases = R.sweep_cases()
    assert 36 <= len(cases) <= 44 and len(set(cases)) == len(cases)
    assert {n for n, _ in cases} == set(R.SWEEP_LENGTHS)
    assert all(0 <= i < n for n, i in cases)
    idx = {i for _, i in cases}
    assert {0, 3, 4, 65535, 65536, 65537} <= idx
    for kind in (lambda n: n - 1, lambda n: n - 2, lambda n: 4 * (n // 4) - 1, lambda n: 4 * (n // 4)):
        assert sum(1 for n, i in cases if i == kind(n)) >= 4
    assert all(a[0] != b[0] for a, b in zip(cases, cases[1:]))             # neighbours differ in length


@pytest.mark.parametrize("gs,betas,wd", list(itertools.product(GSCALES, BETAS, WDS)))
def test_bounds_hold_for_correct_arithmetic(gs, betas, wd):
    bad, ratio = _run(gs, betas, wd, R.RANDOM_LENGTHS)
    print(f"\nemulation, gscale {gs} betas {betas} wd {wd}: worst measured / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratio.items()))
    assert not bad, bad[:3]
    assert all(0.02 < v <= 1.0 for v in ratio.values()), ratio           # and it IS an fp32 computation, not the reference again


@pytest.mark.parametrize("nt", [1, 63, 64, 65, 200])
def test_finish_norm_bound_holds_for_fp32_summation(nt):
    s = (np.random.default_rng(nt).standard_normal(nt) ** 2).astype(np.float32) * 100
    lanes = np.zeros(64, dtype=np.float32)
    for i in range(nt):
        lanes[i % 64] = np.float32(lanes[i % 64] + s[i])
    norm = float(np.sqrt(R._tree(lanes)))
    for mx in (0.0, 1e9, None):
        ref_n, ref_c = R.finish_ref(s, 0.5 * norm if mx is None else mx)
        assert abs(norm - ref_n) <= R.norm_factor(nt) * R.E * ref_n
        if mx is not None:
            assert ref_c == 1.0
        else:
            c = float(np.float32(np.float32(0.5 * norm) / np.float32(np.float32(norm) + np.float32(1e-6))))
            assert abs(c - ref_c) <= R.norm_factor(nt) * R.E * ref_c and 0.49 < ref_c < 0.51


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_bounds_reject_planted_mutants(mutant):
    """one tensor with a chunk seam and an n & 3 tail, gradient scale and weight decay both in play"""
    bad, _ = _run(0.37, (0.9, 0.95), 0.05, [131072 + 1029], mutant)
    assert bad, f"no bound noticed the mutant {mutant}"
    good, _ = _run(0.37, (0.9, 0.95), 0.05, [131072 + 1029])
    assert not good


def _sweep(mutant=None):
    bad = []
    for t, (n, idx) in enumerate(R.sweep_cases()):
        p0, g = R.sweep_p0(n, t), R.sweep_grad(n, idx, t)
        z = np.zeros(n, dtype=np.float32)
        S = R.SWEEP
        p, m, v, sq = R.emulate_step_f32(p0, g, z, z, S["gs"], S["step"], S["lr"], S["b1"], S["b2"], S["eps"], S["wd"], mutant=mutant)
        bad += R.one_hot_violations(t, n, idx, p0, p, m, v, sq)
    return bad


def test_one_hot_checks_pass_on_correct_arithmetic():
    assert not _sweep()


@pytest.mark.parametrize("mutant", ["skip_tail", "skip_seam", "sumsq_of_scaled", "unscaled_update", "beta2_for_beta1", "bc2_for_bc2_sqrt"])
def test_one_hot_checks_reject_mutants(mutant):
    """the exact checks see the mutants the sweep is there for -- a skipped tail or seam element, the norm of the scaled gradient --
    and, through the reference at the one-hot element, gross arithmetic ones (the subtle ones need the random data above)"""
    assert _sweep(mutant), f"no exact check noticed the mutant {mutant}"
