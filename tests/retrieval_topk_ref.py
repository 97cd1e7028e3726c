"""numpy restatements for the top-k retrieval tests (tests/test_cpu_retrieval_topk.py, tests/test_gpu_retrieval_topk.py).

``topk_from``       the lists of octmae_retrieval_topk from a GIVEN score matrix [n, m]: candidates filtered, a stable descending argsort,
                    padded with -1 / -inf
``topk_fn``         a function with the signature of ops.retrieval_topk built on ``topk_from`` and a score function (float64 matmul by
                    default): the drop-in for coem's ``topk=``
``plan`` / ``ws_bytes``   the launch plan of octmae_retrieval_topk and its workspace, restated
``script_accuracy`` the reference script's tensor expressions for the micro / macro match accuracy (full lists), in float64
The scores (``chain_scores``, ``f64_scores``) and the shapes past the split (``TRIP_SHAPES``) are tests/retrieval_ref.py's."""
import numpy as np
import torch

from tests.retrieval_ref import TRIP_SHAPES, chain_scores, f64_scores, _np  # noqa: F401

# ---- the launch plan of octmae_retrieval_topk, restated (the walk of the ranks kernel plus the lists)
TILE = 64               # SIM_ROWS == SIM_COLS (csrc/simtile.hpp)
TARGET_WGS = 1024       # SIM_TARGET_WGS
MAX_GRID_Y = 65535
K_MAX = 32              # RT_KMAX
PAIR_BYTES = 8          # sizeof(RtPair): f32 score, int32 index
TRIP_PLANS = ((1, 1025, 1024), (47, 47, 22), (1024, 3, 1))          # (row blocks, column tiles, split) at TRIP_SHAPES


def plan(n, m):
    """(row blocks, column tiles, split): the grid is row blocks x split, workgroup y walks tiles y, y + split, ..."""
    row_blocks, col_tiles = -(-n // TILE), -(-m // TILE)
    return row_blocks, col_tiles, max(1, min(-(-TARGET_WGS // row_blocks), col_tiles, MAX_GRID_Y))


def ws_bytes(n, m, k):
    """the partial lists [split][n][k] of 8-byte pairs; nothing where the columns are not split"""
    split = plan(n, m)[2]
    return split * n * k * PAIR_BYTES if split > 1 else 0


def candidates(scores, keep=None, row_group=None, col_group=None) -> np.ndarray:
    """bool [n, m]: column j may be returned for row i"""
    s = np.asarray(scores)
    n, m = s.shape
    cand = ~np.isnan(s)
    if keep is not None:
        cand &= (np.asarray(keep) != 0)[None, :]
    if row_group is not None:
        cand &= np.asarray(col_group)[None, :] != np.asarray(row_group)[:, None]
    return cand


def topk_from(scores, k, keep=None, row_group=None, col_group=None):
    """(idx int64 [n, k], score [n, k] in the dtype of ``scores``): higher score first, equal scores by ascending column."""
    s = np.asarray(scores)
    n, m = s.shape
    cand = candidates(s, keep, row_group, col_group)
    order = np.argsort(-s, axis=1, kind="stable")                         # -s: descending; stable: ties by ascending column (NaN last)
    first = np.argsort(~np.take_along_axis(cand, order, axis=1), axis=1, kind="stable")      # the candidates in front, order kept
    order = np.take_along_axis(order, first, axis=1)[:, :k]
    filled = np.arange(order.shape[1])[None, :] < cand.sum(axis=1)[:, None]
    idx = np.full((n, k), -1, dtype=np.int64)
    out = np.full((n, k), -np.inf, dtype=s.dtype)
    idx[:, :order.shape[1]] = np.where(filled, order, -1)
    out[:, :order.shape[1]] = np.where(filled, np.take_along_axis(s, order, axis=1), -np.inf)
    return idx, out


def topk_fn(score_fn=f64_scores):
    def topk(a, b, k, keep=None, row_group=None, col_group=None):
        idx, score = topk_from(score_fn(a, b), k, _np(keep), _np(row_group), _np(col_group))
        return idx.astype(np.int32), score.astype(np.float32)
    return topk


def script_accuracy(topk_indices, attribute_binary):
    """evaluate_results_..._laterality.py:221-226 on a FULL index matrix, with the two divisions in float64:
    (matched count, micro, macro)"""
    topk_indices = torch.as_tensor(np.asarray(topk_indices)).long()
    attribute_binary = torch.as_tensor(np.asarray(attribute_binary))
    topk_attr = torch.tensor([attribute_binary[i] for i in topk_indices.flatten()]).reshape(topk_indices.shape)
    matched = torch.zeros_like(topk_attr)
    matched[topk_attr == attribute_binary.unsqueeze(1)] = 1
    micro = torch.sum(matched).double() / (topk_attr.shape[0] * topk_attr.shape[1])
    macro = torch.mean(torch.sum(matched, dim=1).double() / topk_attr.shape[1])
    return int(matched.sum()), micro.item(), macro.item()
