"""numpy restatement of ops.retrieval_pair_ranks (csrc/retrieval_pair.hip) for tests/test_cpu_eval3mod.py, tests/test_gpu_pair_ranks.py
and tests/test_gpu_eval3mod.py: ``counts`` of tests/retrieval_ref.py on a score matrix (the rows) and on its transpose (the columns).

``pair_counts``      int64 [P, 2, N, 2] from P GIVEN square score matrices
``pair_ranks_from``  a function with the signature of ops.retrieval_pair_ranks built on a score function (float64 matmul by default)"""
import numpy as np

from tests import retrieval_ref as R


def pair_counts(score_matrices) -> np.ndarray:
    out = []
    for s in score_matrices:
        s = np.asarray(s)
        assert s.ndim == 2 and s.shape[0] == s.shape[1], s.shape
        out.append(np.stack([R.counts(s)[:, :2], R.counts(s.T)[:, :2]]))
    return np.stack(out).astype(np.int64)


def pair_ranks_from(score_fn=R.f64_scores):
    def pair_ranks(pairs):
        return pair_counts([score_fn(a, b) for a, b in pairs])
    return pair_ranks
