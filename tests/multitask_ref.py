"""Test helper, not a test: numpy restatements for the multi-task fine-tune mode, independent of octcubem_amd.

``rank_counts_masked``   the counts of octmae_rank_counts_masked by what the reference does: per column, compress to the valid rows,
                         count there with the plain comparison table of tests/metrics_ref.py, scatter back; zeros elsewhere.
``rank_counts``          the stand-in that ``metrics.misc_measures_multi_task(rank_counts=...)`` takes: with a mask the function above,
                         without one tests/metrics_ref.py's.
``multi_task_loss``      OCTCube/engine_finetune.py:45-70 with the weighted label-smoothing criterion as a float64 loop over tasks
                         and rows: the value, its terms (one per valid row of a task), and per logit of a pair the gradient with
                         the sum of the magnitudes of ITS terms (softmax share and target share, which cancel where the model is
                         right), so that a test can compute the error bound of a float32 sum from them."""
import numpy as np

from tests import metrics_ref as R


def _np(a):
    return np.asarray(a.cpu() if hasattr(a, "cpu") else a)


def rank_counts_masked(scores, labels, valid) -> np.ndarray:
    s, lab, val = _np(scores).astype(np.float32), _np(labels) != 0, _np(valid) != 0
    n, C = s.shape
    out = np.zeros((n, C, 4), dtype=np.int32)
    for c in range(C):
        keep = val[:, c]
        if keep.any():
            out[keep, c] = R.rank_counts(s[keep, c:c + 1], lab[keep, c:c + 1])[:, 0]
    return out


def rank_counts(scores, labels, valid=None) -> np.ndarray:
    return R.rank_counts(scores, labels) if valid is None else rank_counts_masked(scores, labels, valid)


def pairs_of(output, T, multi_task_type):
    """[B, T, 2] logit pairs of the two layouts."""
    o = np.asarray(output, dtype=np.float64)
    if multi_task_type == "multi_task_default":
        return o.reshape(o.shape[0], T, 2)
    return np.stack([np.repeat(o[:, :1], T, axis=1), o[:, 1:]], axis=2)


def multi_task_loss(output, target, smoothing=0.1, multi_task_type="multi_task_default"):
    """(value, terms [k], grad [B, T, 2], grad_abs [B, T, 2]) in float64.  ``terms`` are the summands of the value, one per valid
    (row, task); ``grad[b, t]`` is the derivative of that summand with respect to the task's logit pair, (softmax - smoothed one-hot)
    * scale, and ``grad_abs`` the sum of the magnitudes of its two terms (zeros for an invalid row)."""
    tgt = np.asarray(target)
    B, T = tgt.shape[0], tgt.shape[1] - 1
    pairs = pairs_of(output, T, multi_task_type)
    weight_sum = 0.0
    for b in range(B):
        for t in range(T):
            weight_sum += float(tgt[b, 0]) + float(tgt[b, t + 1])
    denom = weight_sum + 1e-8
    terms, grad, grad_abs = [], np.zeros((B, T, 2), dtype=np.float64), np.zeros((B, T, 2), dtype=np.float64)
    for t in range(T):
        rows = [b for b in range(B) if float(tgt[b, 0]) + float(tgt[b, t + 1]) != 0]
        for b in rows:
            z = pairs[b, t]
            logp = z - z.max() - np.log(np.sum(np.exp(z - z.max())))
            k = 0 if tgt[b, 0] >= tgt[b, t + 1] else 1             # argmax of (normal, task), the first on a tie
            row = -(1.0 - smoothing) * logp[k] - smoothing * logp.mean()
            scale = 1.0 / (len(rows) * denom)
            terms.append(row * scale)
            want = np.full(2, smoothing / 2)
            want[k] += 1.0 - smoothing
            grad[b, t] = (np.exp(logp) - want) * scale
            grad_abs[b, t] = (np.exp(logp) + want) * scale
    return float(np.sum(terms)), np.array(terms, dtype=np.float64), grad, grad_abs


def grad_of_layout(grad, grad_abs, multi_task_type):
    """(gradient, sum of the magnitudes of its terms, number of terms) per element of the ``output`` of that layout: two terms per
    logit of a pair, and the shared column 0 collects those of all T tasks."""
    B, T, _ = grad.shape
    if multi_task_type == "multi_task_default":
        return grad.reshape(B, 2 * T), grad_abs.reshape(B, 2 * T), np.full((B, 2 * T), 2.0)
    g = np.concatenate([grad[:, :, 0].sum(1, keepdims=True), grad[:, :, 1]], axis=1)
    a = np.concatenate([grad_abs[:, :, 0].sum(1, keepdims=True), grad_abs[:, :, 1]], axis=1)
    k = np.concatenate([np.full((B, 1), 2.0 * T), np.full((B, T), 2.0)], axis=1)
    return g, a, k
