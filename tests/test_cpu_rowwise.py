"""tests/rowwise.py::row_err sees one-row faults that the whole-tensor L2 bounds of tests/test_gpu_kernels.py let through -- shown
on the CPU, with the attention part of oracle/bf16_points.py (float64 + the kernels' 16-bit roundings) standing in for a correct
kernel and plain float64 autograd on the same operands as the reference.  The bound is the one tests/test_gpu_attention_rows.py
applies on the GPU: 2 x the model's own worst-row error, per tensor."""
import pytest
import torch

from tests import rowwise as RW

FACTOR = 2.0                       # tests/test_gpu_attention_rows.py: the kernel may be 2 x as far from float64 as the model is
L2_FWD, L2_BWD = 4e-3, 1.5e-2      # the whole-tensor bounds of tests/test_gpu_kernels.py
CASES = [(1, 2, 1281, 64), (1, 2, 1537, 32), (2, 3, 300, 64)]
_CACHE = {}


def _case(B, H, N, HD, plain=False):
    key = (B, H, N, HD, plain)
    if key not in _CACHE:
        qkv, do = RW.draw_inputs(B, H, N, HD, seed=N + HD, plain=plain)
        ref = RW.reference(qkv, do, B, N, H, HD)
        m = RW.model(qkv, do, B, N, H, HD)
        _CACHE[key] = (ref, {"o": m["o"], "dq": m["dq_fused"], "dk": m["dk"], "dv": m["dv"]}, m)
    return _CACHE[key]


def _mutations(t):
    """name -> mutated copy of t [B, H, N, hd]: the one-row faults of a kernel with a wrong edge."""
    B, H, N, _ = t.shape
    out = {}
    for name, n in (("zero_first", 0), ("zero_last", N - 1), ("zero_middle", N // 2)):
        m = t.clone(); m[B - 1, H - 1, n] = 0
        out[name] = m
    m = t.clone(); m[0, 0, N // 3] *= 1.1
    out["scale_1.1"] = m
    m = t.clone(); m[0, 1, [N - 2, N - 1]] = t[0, 1, [N - 1, N - 2]]
    out["swap_neighbours"] = m
    m = t.clone(); m[0, 0, N - 1] = t[0, 1, 0]               # the last row of a slice holds what belongs to the next head
    out["next_heads_row"] = m
    return out


@pytest.mark.parametrize("B,H,N,HD", CASES)
def test_row_err_passes_the_model_and_fails_every_one_row_fault(B, H, N, HD):
    ref, mod, raw = _case(B, H, N, HD)
    for name in RW.NAMES:
        own = RW.row_err(mod[name], ref[name])
        bound = FACTOR * own
        # the model's worst row is what 16-bit operands cost: 8 mantissa bits, 2^-9 per rounding, a few roundings deep
        assert 2.0 ** -10 < own <= 1.2e-2, (name, own)
        assert RW.row_err(mod[name], ref[name]) <= bound
        for mut, t in _mutations(mod[name]).items():
            e, idx = RW.row_err(t, ref[name], with_index=True)
            assert e > bound, (name, mut, e, bound)
            if mut.startswith("zero"):
                n = {"zero_first": 0, "zero_last": N - 1, "zero_middle": N // 2}[mut]
                assert idx == (B - 1, H - 1, n), (name, mut, idx)   # and the worst row IS the faulty row
    # a correct kernel that rounds at another place (the two-kernel backward's dQ: Q pre-scaled instead of K) is inside the bound
    # taken from the fused form's model, and the other way round
    pair, fused = RW.row_err(raw["dq_pair"], ref["dq"]), RW.row_err(raw["dq_fused"], ref["dq"])
    assert pair <= FACTOR * fused and fused <= FACTOR * pair, (pair, fused)
    # lse: an fp32 value whose score carries one 16-bit rounding of q * scale * log2e
    assert RW.lse_err(raw["lse"], ref["lse"]) <= 4e-3


def test_whole_tensor_l2_bounds_let_one_row_faults_through():
    """Why the row metric exists: at N = 1281 a zeroed row and a row scaled by 1.1 both PASS the L2 bounds of
    tests/test_gpu_kernels.py (4e-3 forward, 1.5e-2 backward) and FAIL the row bound.  On that suite's own inputs (randn rows of
    equal expected size): whether a zeroed row passes L2 depends on its share of the tensor, 1 / sqrt(B H N) = 1.1e-2 here."""
    B, H, N, HD = 2, 3, 1281, 64           # test_attention_fwd_bwd's largest case
    ref, mod, _ = _case(B, H, N, HD, plain=True)
    for name in RW.NAMES:
        l2_bound = L2_FWD if name == "o" else L2_BWD
        bound = FACTOR * RW.row_err(mod[name], ref[name])
        assert RW.rel_l2(mod[name], ref[name]) < l2_bound
        muts = _mutations(mod[name])
        picks = ["scale_1.1"] if name == "o" else ["scale_1.1", "zero_first", "zero_last", "zero_middle"]
        for mut in picks:      # a zeroed row of o is 1 / sqrt(B H N) = 1.1e-2 of the tensor: above the 4e-3 forward bound already
            assert RW.rel_l2(muts[mut], ref[name]) < l2_bound, (name, mut, RW.rel_l2(muts[mut], ref[name]))
            assert RW.row_err(muts[mut], ref[name]) > bound, (name, mut)


def test_row_err_floor_and_index():
    """The floor: a reference row of (almost) zero norm is measured against the slice's RMS row norm, not against itself."""
    ref = torch.ones(1, 2, 4, 8, dtype=torch.float64)
    ref[0, 1, 2] = 1e-9
    got = ref.clone()
    got[0, 1, 2] += 1e-6                                   # 1000 x the row's own size, 1e-6 of its neighbours'
    e, idx = RW.row_err(got, ref, with_index=True)
    assert idx == (0, 1, 2) and e == pytest.approx(1e-6 * 8 ** 0.5 / (0.75 * 8) ** 0.5, rel=1e-6)
    got = ref.clone()
    got[0, 0, 3, 0] = float("nan")
    e, idx = RW.row_err(got, ref, with_index=True)
    assert e == float("inf") and idx == (0, 0, 3)
    lse = torch.zeros(2, 3, 5, dtype=torch.float64); lse[1, 2, 4] = 9.0
    got = lse.clone(); got[1, 0, 1] = 0.5
    assert RW.lse_err(got, lse, with_index=True) == (0.05, (1, 0, 1))
