"""The attention kernels, every form, checked ROW BY ROW -- `pytest -m gpu` on an MI355X.

The whole-tensor relative L2 bounds of tests/test_gpu_kernels.py (4e-3 forward, 1.5e-2 backward) cannot see a fault confined to
one row -- the last query of a partial tile, the single key past the last full key block, the first row of the next head or
sample: tests/test_cpu_rowwise.py shows a dropped dK row and a 10 % wrong row of o passing them.  Here every row of o, dQ, dK, dV
is measured on its own (tests/rowwise.py::row_err) against float64 softmax-attention autograd on the same 16-bit operands, and
every row of lse relative to 1 + max |lse|.

The bound is not a fixed number: the rounding model of the kernels (the attention part of oracle/bf16_points.py, float64 with a
rounding to the library's operand type where the kernels round, evaluated on the CPU on the same inputs) has a worst-row error of
its own against float64, and the kernel may have 2 x that, per tensor -- the margin tests/test_gpu_rounding_model.py uses for its
self-sensitivity bounds.  The model is 5e-3 ... 1e-2 on bfloat16 operands, a one-row fault of 10 % is 8e-2 or more.  dQ is bounded
by the model variant of the form under test (K pre-scaled in the fused kernels, Q in the dQ kernel of the pair).

"The same inputs" means, for a backward kernel, qkv, dO AND the o and lse it is handed -- those of the forward kernel, not of the model's
forward.  The two differ by rounding flips of o (on the half build, whose forward is the online-max kernel and rounds exp2(s - max)
where the model rounds exp2(s), in half of all elements: one unit of o each way), and delta = rowsum(dO * o) carries a flip into
every dS of its row.  Measured on MI355X, half build, N = 65, head_dim 64: the fused dQ's worst row (0, 1, 20) is 1.124e-3 from
float64, the model fed the kernel's o and lse is 1.124e-3 at the same row (11 of 8320 elements differ), the model fed its own o is
5.449e-4 -- the backward kernel is exact, the difference is its input.  So the backward model starts from the forward kernel's o and
lse; o and lse themselves are bounded by the model's own forward.

Inputs are position dependent (tests/rowwise.py::draw_inputs).  Every measured value and its bound go to the parity ledger."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import ops
from tests import rowwise as RW
from tests.conftest import parity

DEV = "cuda"
FACTOR = 2.0
LENGTHS = {32: [5121, 1536, 1025, 513, 512, 545, 64, 31], 64: [5121, 2561, 1281, 257, 256, 300, 193, 65]}
SHAPES = [(1, 2, N, HD) for HD in (32, 64) for N in LENGTHS[HD]]
# boundaries between (b, h) slices: the row after the last row of a slice belongs to the next head or sample; H = 20 takes two
# passes of the row-constant kernel
SLICE_SHAPES = [(2, 3, 257, 64), (2, 3, 513, 32), (2, 20, 257, 64)]


class _Case:
    """Inputs, float64 reference, model and the per-tensor bounds of one shape; collects what fails instead of stopping at the first."""

    def __init__(self, B, H, N, HD, seed):
        self.dims = (B, N, H, HD)
        self.tag = f"attn_rows/{str(ops.BF16).split('.')[-1]}/hd{HD}/N{N}/B{B}H{H}"
        qkv, do = RW.draw_inputs(B, H, N, HD, seed, dtype=ops.BF16)
        self.qkv, self.do = qkv.to(DEV), do.to(DEV)
        self.ref = RW.reference(self.qkv, self.do, B, N, H, HD)
        self.mod = RW.model(qkv, do, B, N, H, HD, dtype=ops.BF16)
        self.own = {"o": RW.row_err(self.mod["o"], self.ref["o"]), "lse": RW.lse_err(self.mod["lse"], self.ref["lse"])}
        self.fed = None
        self.fails = []

    def backward_model(self, o, lse, do):
        """The model's backward on what the backward kernel is handed: qkv, dO and the o and lse of the forward KERNEL (see the module
        docstring); one evaluation serves every backward form of the case."""
        if self.fed is None or self.fed[0] is not o:
            B, N, H, HD = self.dims
            m = RW.model(self.qkv, do, B, N, H, HD, dtype=ops.BF16, o=o, lse=lse)
            for n in ("dq_fused", "dq_pair", "dk", "dv"):
                self.own[n] = RW.row_err(m[n], self.ref["dq" if n.startswith("dq") else n])
            self.fed = (o, lse)

    def check(self, form, name, got, model_name=None):
        """got [B, H, N, hd] (lse: [B, H, N]) against float64; bound = FACTOR x the model's own error on this tensor."""
        bound = FACTOR * self.own[model_name or name]
        e, idx = (RW.lse_err if name == "lse" else RW.row_err)(got, self.ref[name], with_index=True)
        print(f"{self.tag}/{form}/{name}: worst row {e:.3e} at (b, h, n) = {idx}, model {self.own[model_name or name]:.3e}, bound {bound:.3e}")
        try:
            parity(f"{self.tag}/{form}/{name}", e, bound)
        except AssertionError as err:
            self.fails.append(f"{err}; worst row (b, h, n) = {idx}")

    def forward(self, optimistic):
        B, N, H, HD = self.dims
        o, lse = ops.attn_fwd(self.qkv, B, N, H, HD, HD ** -0.5, optimistic=optimistic)
        form = {True: "fwd_optimistic", False: "fwd_online_max", None: "fwd_default"}[optimistic]
        self.check(form, "o", RW.heads(o, B, N, H, HD))
        self.check(form, "lse", lse)
        return o, lse

    def backward(self, form, o, lse, fused, delta=None, do=None):
        B, N, H, HD = self.dims
        do = self.do if do is None else do
        self.backward_model(o, lse, do)
        d = ops.attn_bwd(self.qkv, o, do, lse, B, N, H, HD, HD ** -0.5, fused=fused, delta=delta)
        dq, dk, dv = RW.split_heads(d, B, N, H, HD)
        self.check(form, "dq", dq, "dq_fused" if fused else "dq_pair")
        self.check(form, "dk", dk)
        self.check(form, "dv", dv)

    def every_form(self):
        """Both forwards; the backward as the two-kernel pair, fused in both main-kernel forms, and fused with the key past the last
        full key block in a launch of its own."""
        B, N, H, HD = self.dims
        self.forward(True)
        self.forward(False)
        o, lse = ops.attn_fwd(self.qkv, B, N, H, HD, HD ** -0.5)          # the default forward's: what every backward form is handed
        self.backward("bwd_pair", o, lse, fused=False)
        key = f"attn_bwd_hd{HD}_form"                                     # attn_bwd_hd32_form / attn_bwd_hd64_form
        prev = ops.set_option(key, 1)
        prev_t = ops.set_option("attn_bwd_tail_fused", 1)
        try:
            self.backward("bwd_fused_form1", o, lse, fused=True)
            ops.set_option(key, 0)
            self.backward("bwd_fused_form0", o, lse, fused=True)
            ops.set_option(key, 1)
            ops.set_option("attn_bwd_tail_fused", 0)
            self.backward("bwd_fused_tail_unfused", o, lse, fused=True)
        finally:
            ops.set_option(key, prev)
            ops.set_option("attn_bwd_tail_fused", prev_t)

    def finish(self):
        assert not self.fails, f"{len(self.fails)} row-wise checks failed:\n" + "\n".join(self.fails)


@pytest.mark.parametrize("B,H,N,HD", SHAPES)
def test_attention_rows_every_form(B, H, N, HD):
    """Lengths that are whole key blocks of the fused backward (512 / 256 keys), leave a multi-group tail, leave exactly one key, or
    are shorter than one tile, up to the production length 5121; both forwards and every backward form at each."""
    c = _Case(B, H, N, HD, seed=7 * N + HD)
    c.every_form()
    c.finish()


@pytest.mark.parametrize("B,H,N,HD", SLICE_SHAPES)
def test_attention_rows_across_slice_boundaries(B, H, N, HD):
    """Several samples and heads with one key past the last full key block: a kernel that reads or writes one row past its (b, h)
    slice lands in the next head's or sample's rows, which hold other values."""
    c = _Case(B, H, N, HD, seed=11 * N + H)
    c.every_form()
    c.finish()


@pytest.mark.parametrize("B,H,N,HD", [(1, 4, 300, 64), (2, 8, 513, 32)])
def test_attention_rows_fused_backward_with_the_proj_dgrad_delta(B, H, N, HD):
    """The production backward: delta comes out of the proj dgrad's epilogue (ops.linear_dgrad_delta), the fused kernel skips its
    pass over O and dO.  The dgrad's weight is the identity, so dO is the position-dependent draw itself, bit for bit."""
    c = _Case(B, H, N, HD, seed=13 * N + HD)
    C = H * HD
    o, lse = c.forward(None)
    w = torch.eye(C, dtype=ops.BF16, device=DEV)
    do, delta = ops.linear_dgrad_delta(c.do, w, o, H, HD)
    assert delta is not None, "the fused dgrad + delta GEMM must take this shape (M >= 256, C >= 256)"
    assert torch.equal(do, c.do)
    c.backward("bwd_fused_delta", o, lse, fused=True, delta=delta, do=do)
    c.finish()
