"""Test helper, not a test: a numpy restatement of the six outputs of octmae_bootstrap_rank_metrics (csrc/bootstrap.hip) from
``(scores, labels, mult, unit, valid)``, sort-based, integers in int64 and floats in float64, independent of octcubem_amd.

``rank_metrics``   per resample r and class c, with w = valid ? mult[r][unit] : 0 along the stable descending order of the class's
                   scores, TP / ALL the cumulative weighted positives / samples at the END of every tie group g, posw_g / negw_g the
                   group's own weights, FP_g = ALL_g - TP_g:
                     P, N      the totals
                     U2        sum_g posw_g (2 (N - FP_g) + negw_g)              (twice the Mann-Whitney statistic, exact)
                     ap_sum    sum_g posw_g * (TP_g / ALL_g)
                     auprc     sum_g (posw_g / P) * (prec_g + prec_(g-1)) / 2,   prec = TP / ALL, 1 where ALL == 0 and before group 0
                     max_f1    max(0, max_g 2 p r / (p + r + 1e-8)),             p = prec_g, r = TP_g / P
                   With P == 0 the three floats are 0 (the caller reports the pair as undefined).  It has the signature of
                   ``ops.bootstrap_rank_metrics`` and serves as the ``kernel=`` of octcubem_amd.metrics.bootstrap_rank_metrics on the CPU.
                   ``fault=`` plants one of three mistakes of a chunked walk (``FAULTS``) so that a test can show the bounds catch it.
``brute_force``    the resample materialised with np.repeat and handed to the EXISTING path, metrics.binary_rank_metrics on the O(n^2)
                   comparison table of tests/metrics_ref.py: what a user gets today by resampling the rows.

The error bounds.  ``SUM_BOUND(terms) = (terms + 4) * 2^-51`` for ap_sum / P and auprc: each is a sum of at most ``terms`` non-negative
summands whose total is at most 1 (precisions weighted by recall steps that add up to 1).  A summand carries a constant number of
roundings, at most five (two quotients, their sum, the width posw / P, the product; halving is exact), each at most half an ulp =
2^-53 relative, and summing ``terms`` non-negative numbers in ANY order adds at most (terms - 1) 2^-53 relative to the total: one side
is off by at most (terms + 4) 2^-53, two sides that each obey this by (terms + 4) 2^-52, and the bound leaves another factor of two
for the one formulation that differs in kind: binary_rank_metrics forms the widths as differences of rounded recalls, 2^-52 absolute
per width instead of relative, at most terms 2^-52 more in all.  ``terms`` is n for the kernel against this file; against the brute
force it is max(n, size of the materialised resample), because that path sums one summand per positive ROW for the average precision.
``F1_BOUND = 2^-49``: the value is at most 1 and comes from six roundings (TP / ALL, TP / P, the product, two additions, the quotient;
doubling is exact) of positive terms, no cancellation: at most 6 x 2^-53 relative per side, 12 x 2^-53 < 2^-49 between two sides; the
maximum of values that agree pairwise within a bound agrees within it.  Derived, not measured."""
import numpy as np

F1_BOUND = 2.0 ** -49
FAULTS = ("drop_end", "lose_carry", "lead_precision_0")


def SUM_BOUND(terms: int) -> float:
    return (terms + 4) * 2.0 ** -51


def _np(a):
    return np.asarray(a.cpu() if hasattr(a, "cpu") else a)


def sorted_columns(scores, labels, unit=None, valid=None):
    """Per class: (unit id, label, valid, tie-group end) along the stable descending order -- the kernel's inputs, as bool / int64."""
    s = _np(scores).astype(np.float32)
    lab = _np(labels) != 0
    n, C = s.shape
    val = np.ones((n, C), dtype=bool) if valid is None else _np(valid) != 0
    uid = np.arange(n, dtype=np.int64) if unit is None else _np(unit).astype(np.int64)
    cols = []
    for c in range(C):
        order = np.argsort(-s[:, c].astype(np.float64), kind="stable")       # a NaN (legal only where invalid) sorts last
        v = s[order, c]
        end = np.r_[v[1:] != v[:-1], True]                                   # inf == inf, -0.0 == 0.0
        cols.append((uid[order], lab[order, c], val[order, c], end))
    return cols


def rank_metrics(scores, labels, mult, unit=None, valid=None, fault=None, fault_at=None):
    """dict of P, N, U2 (int64 [R, C]) and ap_sum, auprc, max_f1 (float64 [R, C]).  ``fault`` in FAULTS with ``fault_at``: the index of
    the tie-group end to drop ('drop_end'), or the position in front of which the running sums restart ('lose_carry')."""
    assert fault is None or fault in FAULTS
    m = _np(mult).astype(np.int64)
    R, C = m.shape[0], _np(scores).shape[1]
    out = {k: np.zeros((R, C), dtype=np.int64) for k in ("P", "N", "U2")}
    out.update({k: np.zeros((R, C), dtype=np.float64) for k in ("ap_sum", "auprc", "max_f1")})
    for c, (uid, lab, val, end) in enumerate(sorted_columns(scores, labels, unit, valid)):
        ends = np.nonzero(end)[0]
        if fault == "drop_end":
            ends = np.delete(ends, fault_at)
        for r in range(R):
            w = np.where(val, m[r, uid], 0)
            tp, al = np.cumsum(np.where(lab, w, 0)), np.cumsum(w)
            P, N = int(tp[-1]), int(al[-1] - tp[-1])
            if fault == "lose_carry":
                tp, al = tp.copy(), al.copy()
                tp[fault_at:] -= tp[fault_at - 1]
                al[fault_at:] -= al[fault_at - 1]
            TP, ALL = tp[ends], al[ends]
            pTP, pALL = np.r_[0, TP[:-1]], np.r_[0, ALL[:-1]]
            posw = TP - pTP
            negw = (ALL - pALL) - posw
            out["P"][r, c], out["N"][r, c] = P, N
            out["U2"][r, c] = int(np.sum(posw * (2 * (N - (ALL - TP)) + negw)))
            if P == 0:
                continue
            empty = 0.0 if fault == "lead_precision_0" else 1.0
            with np.errstate(invalid="ignore", divide="ignore"):
                prec = np.where(ALL > 0, TP / np.where(ALL > 0, ALL, 1), empty)
                pprec = np.where(pALL > 0, pTP / np.where(pALL > 0, pALL, 1), empty)
            rec = TP / P
            out["ap_sum"][r, c] = float(np.sum(posw * prec))
            out["auprc"][r, c] = float(np.sum((posw / P) * (prec + pprec) * 0.5))
            out["max_f1"][r, c] = max(0.0, float(np.max(2 * prec * rec / (prec + rec + 1e-8))))
    return out


def mismatches(got, want, terms: int):
    """Where two sets of the six outputs disagree: P, N, U2 must be equal; ap_sum / P, auprc and max_f1 must lie within SUM_BOUND(terms)
    and F1_BOUND wherever P > 0.  A list of (key, r, c, got, want), empty when they agree."""
    g = {k: _np(v) for k, v in got.items()}
    bad = []
    for k in ("P", "N", "U2"):
        assert g[k].dtype == np.int64 and g[k].shape == want[k].shape, (k, g[k].dtype, g[k].shape)
        bad += [(k, r, c, int(g[k][r, c]), int(want[k][r, c])) for r, c in zip(*np.nonzero(g[k] != want[k]))]
    P = np.maximum(want["P"], 1).astype(np.float64)
    for k, scale, bound in (("ap_sum", P, SUM_BOUND(terms)), ("auprc", 1.0, SUM_BOUND(terms)), ("max_f1", 1.0, F1_BOUND)):
        assert g[k].dtype == np.float64 and g[k].shape == want[k].shape, (k, g[k].dtype, g[k].shape)
        err = np.abs(g[k] / scale - want[k] / scale)
        bad += [(k, r, c, float(g[k][r, c]), float(want[k][r, c])) for r, c in zip(*np.nonzero(~(err <= bound)))]
    return bad


def kernel_constants():
    """BS_BLOCK, BS_CHUNK, BS_LDS_UNITS as csrc/bootstrap.hip defines them: the shapes of the tests follow the source."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "octcubem_amd", "csrc", "bootstrap.hip")).read()
    return tuple(int(re.search(rf"^constexpr int {name} = (\d+);", src, re.M).group(1)) for name in ("BS_BLOCK", "BS_CHUNK", "BS_LDS_UNITS"))


def stub_problem(multi_label: bool, n: int = 48, C: int = 3, batch: int = 10):
    """A loader and a stub model for engine_finetune.evaluate_report: ``(loader, model, targets)``.  n samples of C features, the model
    a fixed linear read-out, targets that follow the features loosely; every class holds n / C positives (at least 8 of each label
    value, so that a resample without one is out of reach: (1 - 1/C)^n per draw of n)."""
    import torch
    g = torch.Generator().manual_seed(31)
    cls = torch.arange(n) % C
    x = 0.9 * torch.nn.functional.one_hot(cls, C).float() + torch.rand(n, C, generator=g)
    x = torch.round(x * 16) / 16                                   # a grid of sixteenths: ties
    targets = torch.nn.functional.one_hot(cls, C).float() if multi_label else cls

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(2.0 * torch.eye(C) + 0.25)

        def forward(self, v):
            return v @ self.w

    return [(x[i:i + batch], targets[i:i + batch]) for i in range(0, n, batch)], Stub(), targets


def finish(raw):
    """The host's divisions: dict of roc_auc, AP, auprc, max_f1 float64 [R, C], NaN where P == 0 or N == 0."""
    P, N = raw["P"].astype(np.int64), raw["N"].astype(np.int64)
    ok = (P > 0) & (N > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        vals = {"roc_auc": raw["U2"].astype(np.float64) / (2.0 * P * N), "AP": raw["ap_sum"] / P, "auprc": raw["auprc"], "max_f1": raw["max_f1"]}
    return {k: np.where(ok, v, np.nan) for k, v in vals.items()}


def brute_force(scores, labels, mult_row, unit=None, valid=None, c=0):
    """One resample of one class through the existing path: (dict of the four metrics as floats, number of materialised rows).  The
    rows of the class's population are repeated ``mult_row[unit]`` times.  ValueError where that path raises (one label value)."""
    from octcubem_amd import metrics
    from tests import metrics_ref
    s, lab = _np(scores).astype(np.float32)[:, c], (_np(labels) != 0)[:, c]
    n = s.shape[0]
    uid = np.arange(n) if unit is None else _np(unit).astype(np.int64)
    w = _np(mult_row).astype(np.int64)[uid]
    if valid is not None:
        w = np.where((_np(valid) != 0)[:, c], w, 0)
    rs, rl = np.repeat(s, w)[:, None], np.repeat(lab, w).astype(np.uint8)[:, None]
    got = metrics.binary_rank_metrics(metrics_ref.rank_counts(rs, rl), rl)
    return {k: float(v[0]) for k, v in got.items()}, int(w.sum())
