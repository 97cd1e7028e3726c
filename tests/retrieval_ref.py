"""numpy / torch-CPU restatements for the retrieval tests (tests/test_cpu_retrieval.py, tests/test_gpu_retrieval.py).

``counts``          the four integers of octmae_retrieval_ranks per row, from a GIVEN score matrix [n, m] (any float dtype)
``ranks_from``      a function with the signature of ops.retrieval_ranks built on ``counts`` and a score function (float64 matmul by default)
``chain_scores``    the f32 k-ordered fmaf chain, exact for inputs whose partial sums are exact in f32 (the dyadic family)
``stable_preds``    the partner's place by torch.argsort(descending=True, stable=True) on the CPU: the cross-check of counts[:, 0] + counts[:, 1]
``rank_metrics`` / ``get_metrics`` / ``get_metrics_3modalities`` / ``get_corrected_metrics``   the reference's formulas from ``preds``"""
import numpy as np
import torch


def counts(scores, target=None, keep=None, row_group=None, col_group=None) -> np.ndarray:
    s = np.asarray(scores)
    n, m = s.shape
    target = np.arange(n) if target is None else np.asarray(target).astype(np.int64)
    kept = np.ones(m, dtype=bool) if keep is None else np.asarray(keep) != 0
    assert target.shape == (n,) and kept.shape == (m,) and kept[target].all()
    j = np.arange(m)[None, :]
    t = s[np.arange(n), target][:, None]
    out = np.zeros((n, 4), dtype=np.int64)
    out[:, 0] = (kept[None, :] & (j != target[:, None]) & (s > t)).sum(1)
    out[:, 1] = (kept[None, :] & (j < target[:, None]) & (s == t)).sum(1)
    if row_group is not None:
        same = np.asarray(col_group)[None, :] == np.asarray(row_group)[:, None]
        out[:, 2] = (same & (s >= 0)).sum(1)
        out[:, 3] = same.sum(1)
    return out


# ---- the launch plan of octmae_retrieval_ranks, restated
TILE = 64               # SIM_ROWS == SIM_COLS (csrc/simtile.hpp)
TARGET_WGS = 1024       # SIM_TARGET_WGS
MAX_GRID_Y = 65535
# (n, m, d) at which a workgroup of retrieval_ranks_kernel walks more than one column tile, with (row blocks, column tiles, split):
# tests/test_cpu_retrieval.py compares the constants with csrc/retrieval.hip and the plans with this table; tests/test_gpu_retrieval.py
# runs the shapes
TRIP_SHAPES = ((3, 65600, 2), (3001, 3001, 3), (65473, 131, 2))
TRIP_PLANS = ((1, 1025, 1024),          # one workgroup of 1024 makes a second trip, onto a whole last tile
              (47, 47, 22),             # two or three trips everywhere, a 57-column last tile
              (1024, 3, 1))             # split 1: every workgroup walks all three tiles, the last of 3 columns


def plan(n, m):
    """(row blocks, column tiles, split): the grid is row blocks x split, workgroup y walks tiles y, y + split, ..."""
    row_blocks, col_tiles = -(-n // TILE), -(-m // TILE)
    return row_blocks, col_tiles, max(1, min(-(-TARGET_WGS // row_blocks), col_tiles, MAX_GRID_Y))


def _np(x):
    return None if x is None else (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x))


def f64_scores(a, b):
    return _np(a).astype(np.float64) @ _np(b).astype(np.float64).T


def ranks_from(score_fn=f64_scores):
    def ranks(a, b, target=None, keep=None, row_group=None, col_group=None):
        return counts(score_fn(a, b), _np(target), _np(keep), _np(row_group), _np(col_group))
    return ranks


def chain_scores(a, b) -> np.ndarray:
    """acc = fmaf(a[i][k], b[j][k], acc) over k in float32.  Evaluated as a float32 multiply and add per k: equal to the fused chain
    whenever every product and partial sum is exactly representable (multiples of 1/16 below 2^20: the dyadic family)."""
    a, b = _np(a).astype(np.float32), _np(b).astype(np.float32)
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=np.float32)
    for k in range(a.shape[1]):
        acc = (a[:, k:k + 1] * b[None, :, k] + acc).astype(np.float32)
    return acc


def stable_preds(scores, target=None) -> np.ndarray:
    s = torch.as_tensor(np.asarray(scores))
    target = torch.arange(s.shape[0]) if target is None else torch.as_tensor(np.asarray(target)).long()
    ranking = torch.argsort(s, dim=1, descending=True, stable=True)
    return torch.where(ranking == target.view(-1, 1))[1].numpy()


def rank_metrics(name, preds) -> dict:
    preds = np.asarray(preds)
    m = {f"{name}_mean_rank": preds.mean() + 1, f"{name}_median_rank": np.floor(np.median(preds)) + 1}
    for k in (1, 5, 10):
        m[f"{name}_R@{k}"] = np.mean(preds < k)
    return m


def get_metrics(image, text) -> dict:
    s = f64_scores(image, text)
    return {**rank_metrics("image_to_text", stable_preds(s)), **rank_metrics("text_to_image", stable_preds(s.T))}


def get_metrics_3modalities(image, text1, text2, w1, w2) -> dict:
    w1, w2 = _np(w1), _np(w2)
    out = {}
    for name, a, b, w in (("image_to_text1", image, text1, w1), ("text1_to_image", text1, image, w1), ("image_to_text2", image, text2, w2),
                          ("text2_to_image", text2, image, w2), ("text1_to_text2", text1, text2, w1 * w2),
                          ("text2_to_text1", text2, text1, w1 * w2)):
        out.update(rank_metrics(name, stable_preds(f64_scores(a, b))[w > 0]))
    return out


def get_corrected_metrics(image, text, labels) -> dict:
    labels = list(labels)
    s = f64_scores(image, text)
    last = {l: i for i, l in enumerate(labels)}
    cols = sorted(set(last.values()))
    reduced = s[:, cols]
    tgt = np.asarray([cols.index(last[l]) for l in labels])
    out = rank_metrics("corrected_image_to_text", stable_preds(reduced, tgt))
    same = np.asarray([[li == lj for lj in labels] for li in labels])
    hit = same & (s >= 0)
    out["corrected_text_to_image_micro_recall"] = hit.sum() / same.sum()
    out["corrected_text_to_image_macro_recall"] = np.mean(hit.sum(1) / same.sum(1))
    return out
