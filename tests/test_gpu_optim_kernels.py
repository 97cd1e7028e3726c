"""The multi-tensor optimizer kernels of csrc/optim.hip -- mt_sumsq, mt_finish_norm and the four mt_adamw_kernel<LP, SQ> -- against the
float64 reference and the per-element bounds of tests/optim_ref.py (derived there by counting fp32 roundings, validated on the CPU by
tests/test_cpu_optim_model.py), and the host-side tables of octcubem_amd/optim.py.

Every tensor a kernel test hands to a kernel is a VIEW inside a larger sentinel-filled buffer (Guarded): after every launch every
byte outside the views must be unchanged, and the gradients bit-unchanged.  That is how an over-run is seen; nothing here reads or
writes outside a live allocation (the host-side regressions keep even what the UNFIXED tables would touch inside one).

Measured / bound of the worst element goes to the parity ledger (tests/conftest.py::parity) under optim/...
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from octcubem_amd import misc, ops, optim as foptim
    from octcubem_amd._lib import call
    from octcubem_amd.optim import _MultiTensorTable
    LPT = ops.BF16
else:
    LPT = torch.bfloat16
from tests import optim_ref as R
from tests.conftest import parity

DEV = "cuda"
GUARD = 64                       # elements of sentinel before, between and after the views
SENT = {torch.float32: -7777.25, torch.bfloat16: 7.0, torch.float16: 7.0}
VARIANTS = {"plain": (False, False), "lp": (True, False), "sq": (False, True), "lp_sq": (True, True)}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ints(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


class Guarded:
    """Tensors of one role as views inside ONE sentinel-filled buffer.  Every view starts 256 bytes aligned (fp32; 128 bytes for the
    16-bit copy) plus ``offs`` elements, with at least GUARD elements of sentinel on either side."""

    def __init__(self, lengths, dtype=torch.float32, offs=0, fill=None, sentinel=None):
        offs = [offs] * len(lengths) if isinstance(offs, int) else list(offs)
        sentinel = SENT[dtype] if sentinel is None else sentinel          # (tests/test_gpu_nonfinite.py surrounds the inputs with NaN)
        self.starts, pos = [], GUARD
        for n, o in zip(lengths, offs):
            self.starts.append(pos + o)
            pos = (pos + o + n + 63) // 64 * 64 + GUARD
        self.buf = torch.full((pos,), sentinel, dtype=dtype, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.views = [self.buf[s:s + n] for s, n in zip(self.starts, lengths)]
        inside = torch.zeros(pos, dtype=torch.bool, device=DEV)
        for v, s in zip(self.views, self.starts):
            inside[s:s + v.numel()] = True
            if fill is not None:
                v.fill_(fill)
        self.outside = ~inside
        self.snap = None

    def load(self, arrays):
        for v, a in zip(self.views, arrays):
            v.copy_(torch.from_numpy(np.ascontiguousarray(a)))

    def ptrs(self):
        return [v.data_ptr() for v in self.views]

    def numpy(self):
        return [v.cpu().numpy().copy() for v in self.views]

    def snapshot(self):
        self.snap = self.buf.clone()

    def assert_outside_unchanged(self, what, also_view=None):
        changed = _ints(self.buf) != _ints(self.snap)
        mask = self.outside.clone()
        if also_view is not None:
            s = self.starts[also_view]
            mask[s:s + self.views[also_view].numel()] = True
        bad = (changed & mask).nonzero().flatten()
        assert bad.numel() == 0, f"{what}: {bad.numel()} elements outside the tensors were written, first at buffer offsets " \
                                 f"{bad[:8].tolist()} (views start at {self.starts})"

    def assert_unchanged(self, what):
        bad = (_ints(self.buf) != _ints(self.snap)).nonzero().flatten()
        assert bad.numel() == 0, f"{what} was written: {bad.numel()} elements, first at buffer offsets {bad[:8].tolist()}"


class World:
    """p, g, m, v, the 16-bit copy and sumsq of one table, each role in a Guarded buffer of its own"""

    def __init__(self, lengths, offs=None, lp_null=(), sentinel=None):
        """sentinel: what surrounds p, g, m, v in place of SENT (the 16-bit copy and sumsq are outputs and keep theirs)"""
        offs = offs or {}
        self.lengths = list(lengths)
        self.P, self.G, self.M, self.V = (Guarded(lengths, offs=offs.get(r, 0), fill=0.0, sentinel=sentinel) for r in "pgmv")
        self.LP = Guarded(lengths, dtype=LPT, offs=offs.get("lp", 0))
        self.SQ = Guarded([len(lengths)], fill=0.0)
        self.lp_null = set(lp_null)
        self.roles = {"p": self.P, "g": self.G, "m": self.M, "v": self.V, "lp": self.LP, "sumsq": self.SQ}

    def table(self, with_state=True, lp=False):
        none = [None] * len(self.lengths)
        lps = [0 if i in self.lp_null else a for i, a in enumerate(self.LP.ptrs())] if lp else None
        return _MultiTensorTable(self.P.views, self.G.views, self.M.views if with_state else none,
                                 self.V.views if with_state else none, lps)

    def adamw(self, variant, gs, step, lr, b1, b2, eps, wd):
        """one launch of mt_adamw_kernel<LP, SQ> through the C entry point, then: nothing outside the views was written, g and
        whatever this variant does not own were not written at all"""
        lp, sq = VARIANTS[variant]
        tab = self.table(lp=lp)
        assert (tab.lp_table is not None) == lp
        # gs: a number, or a one-element device tensor the caller placed (its data pointer is what the kernel is handed)
        gs_t = gs if gs is None or isinstance(gs, torch.Tensor) else torch.tensor([gs], dtype=torch.float32, device=DEV)
        self.SQ.views[0].zero_()
        for b in self.roles.values():
            b.snapshot()
        call("octmae_mt_adamw_fused", tab.table.data_ptr(), tab.chunk_tensor.data_ptr(), tab.chunk_off.data_ptr(), tab.n_chunks,
             gs_t.data_ptr() if gs_t is not None else None, tab.lp_table.data_ptr() if lp else None,
             self.SQ.views[0].data_ptr() if sq else None, lr, b1, b2, eps, wd, step, _stream())
        torch.cuda.synchronize()
        what = f"mt_adamw_kernel<{int(lp)},{int(sq)}>"
        for r in "pmv":
            self.roles[r].assert_outside_unchanged(f"{what}, {r}")
        self.G.assert_unchanged(f"{what}: the gradient")
        if lp:
            for i in (self.lp_null or [None]):
                self.LP.assert_outside_unchanged(f"{what}, 16-bit copy", also_view=i)
        else:
            self.LP.assert_unchanged(f"{what}: the 16-bit copy")
        (self.SQ.assert_outside_unchanged if sq else self.SQ.assert_unchanged)(f"{what}: sumsq")

    def sumsq(self):
        """one launch of mt_sumsq_kernel; writes nothing but sumsq"""
        tab = self.table(with_state=False)
        self.SQ.views[0].zero_()
        for b in self.roles.values():
            b.snapshot()
        call("octmae_mt_sumsq", tab.table.data_ptr(), tab.chunk_tensor.data_ptr(), tab.chunk_off.data_ptr(), tab.n_chunks,
             self.SQ.views[0].data_ptr(), _stream())
        torch.cuda.synchronize()
        for r in ("p", "g", "m", "v", "lp"):
            self.roles[r].assert_unchanged(f"mt_sumsq_kernel: {r}")
        self.SQ.assert_outside_unchanged("mt_sumsq_kernel: sumsq")
        return self.SQ.views[0].cpu().numpy().copy()

    def assert_lp_is_cast_of_p(self, what):
        for i, (p, lp) in enumerate(zip(self.P.views, self.LP.views)):
            if i in self.lp_null:
                continue
            bad = (_ints(lp) != _ints(p.to(LPT))).nonzero().flatten()
            assert bad.numel() == 0, f"{what}: 16-bit copy of tensor {i} (n {p.numel()}) differs from the cast of p at {bad[:8].tolist()}"


def _check_sumsq(got, gsteps_raw, lengths, where):
    worst = 0.0
    for t, (n, g) in enumerate(zip(lengths, gsteps_raw)):
        ref = R.sumsq_ref(g)
        r = abs(float(got[t]) - ref) / (R.sumsq_factor(n) * R.E * ref)
        assert r <= 1.0, f"{where}: sumsq[{t}] (n {n}) = {float(got[t])!r}, reference {ref!r}: {r:.2f} x its bound of {R.sumsq_factor(n)} e"
        worst = max(worst, r)
    return worst


# ------------------------------------------------------------------------------------------------ exact one-hot sweep
@pytest.mark.parametrize("variant", ["sumsq"] + list(VARIANTS))
def test_one_hot_sweep_is_exact(variant):
    """~40 tensors in one table, g = t + 1 at one index and zero elsewhere: the index walks the vector loop's first and last quad, the
    n & 3 tail and both sides of the 65536 chunk seams.  sumsq[t] == (t + 1)^2 exactly (the RAW gradient: the scale is 0.5), m and v
    nonzero at that index only, every other p == p0 (1 - lr wd) bit for bit, the 16-bit copy == the cast of p bit for bit."""
    cases = R.sweep_cases()
    lengths = [n for n, _ in cases]
    w = World(lengths)
    p0 = [R.sweep_p0(n, t) for t, (n, _) in enumerate(cases)]
    w.P.load(p0)
    w.G.load([R.sweep_grad(n, i, t) for t, (n, i) in enumerate(cases)])
    S = R.SWEEP
    if variant == "sumsq":
        sq = w.sumsq()
        exp = np.array([(t + 1) ** 2 for t in range(len(cases))], dtype=np.float32)
        assert np.array_equal(sq, exp), f"sumsq differs at tensors {np.flatnonzero(sq != exp)[:8].tolist()}: {sq[sq != exp][:8]}"
        return
    w.adamw(variant, S["gs"], S["step"], S["lr"], S["b1"], S["b2"], S["eps"], S["wd"])
    sq = w.SQ.views[0].cpu().numpy().copy() if VARIANTS[variant][1] else None
    p, m, v = w.P.numpy(), w.M.numpy(), w.V.numpy()
    bad = []
    for t, (n, i) in enumerate(cases):
        bad += R.one_hot_violations(t, n, i, p0[t], p[t], m[t], v[t], None if sq is None else sq[t])
    assert not bad, f"{len(bad)} violations: " + "; ".join(bad[:4])
    if VARIANTS[variant][0]:
        w.assert_lp_is_cast_of_p(variant)


# ------------------------------------------------------------------------------------------------ random data against ref_step
_DRAWS = {}


def _draw(gs):
    if gs not in _DRAWS:
        _DRAWS[gs] = R.draw(R.RANDOM_LENGTHS, 1, gs)
    return _DRAWS[gs]


@pytest.mark.parametrize("wd", [0.0, 0.05])
@pytest.mark.parametrize("betas", [(0.9, 0.95), (0.9, 0.999)], ids=["b95", "b999"])
@pytest.mark.parametrize("gs", [None, 0.37, 2.0 ** -16], ids=["noscale", "gs0.37", "gs2^-16"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_three_steps_within_per_element_bounds(variant, gs, betas, wd):
    """every (LP, SQ) variant x gradient scale x betas x weight decay, three steps: p, m and v of every element inside its bound from
    the float64 step taken from the kernel's own state before the step; sumsq of the RAW gradient inside its bound"""
    lengths = R.RANDOM_LENGTHS
    p0, gsteps = _draw(gs)
    w = World(lengths)
    w.P.load(p0)
    ratio = {"p": 0.0, "m": 0.0, "v": 0.0, "sumsq": 0.0}
    for step in (1, 2, 3):
        w.G.load(gsteps[step - 1])
        before = (w.P.numpy(), w.M.numpy(), w.V.numpy())
        w.adamw(variant, gs, step, R.LR, betas[0], betas[1], 1e-8, wd)
        after = (w.P.numpy(), w.M.numpy(), w.V.numpy())
        for t, n in enumerate(lengths):
            ref = R.ref_step(before[0][t], gsteps[step - 1][t], before[1][t], before[2][t], gs, step, R.LR, betas[0], betas[1], 1e-8, wd)
            got = R.check_step(after[0][t], after[1][t], after[2][t], ref, f"{variant} step {step} tensor {t} (n {n}): ")
            for k in "pmv":
                ratio[k] = max(ratio[k], got[k])
        if VARIANTS[variant][1]:
            ratio["sumsq"] = max(ratio["sumsq"], _check_sumsq(w.SQ.views[0].cpu().numpy(), gsteps[step - 1], lengths, f"{variant} step {step}"))
        if VARIANTS[variant][0]:
            w.assert_lp_is_cast_of_p(f"{variant} step {step}")
    tag = f"optim/adamw_{variant}/{'noscale' if gs is None else gs}/b2_{betas[1]}/wd{wd}"
    for k in ("p", "m", "v") + (("sumsq",) if VARIANTS[variant][1] else ()):
        parity(f"{tag}/{k}", ratio[k], 1.0)


# ------------------------------------------------------------------------------------------------ alignment matrix
ALIGN_HP = dict(gs=0.37, lr=R.LR, b1=0.9, b2=0.95, eps=1e-8, wd=0.05)


def _aligned_run(offs=None, lp_null=()):
    """two steps of <LP, SQ> on the random draw -> per step (p, m, v, lp as integers, sumsq), and mt_sumsq's own sums"""
    p0, gsteps = _draw(ALIGN_HP["gs"])
    w = World(R.RANDOM_LENGTHS, offs=offs, lp_null=lp_null)
    w.P.load(p0)
    out = []
    for step in (1, 2):
        w.G.load(gsteps[step - 1])
        H = ALIGN_HP
        w.adamw("lp_sq", H["gs"], step, H["lr"], H["b1"], H["b2"], H["eps"], H["wd"])
        out.append(dict(p=[_ints(x).cpu() for x in w.P.views], m=[_ints(x).cpu() for x in w.M.views], v=[_ints(x).cpu() for x in w.V.views],
                        lp=[_ints(x).cpu() for x in w.LP.views], sumsq=w.SQ.views[0].cpu().numpy().copy()))
    out.append(w.sumsq())
    return out


@pytest.fixture(scope="module")
def aligned():
    return _aligned_run()


ALIGN_CASES = [(r, o) for r in ("p", "g", "m", "v", "lp") for o in (1, 2, 3)] + [("lp_null", 0)]


@pytest.mark.parametrize("role,off", ALIGN_CASES, ids=[f"{r}+{o}" for r, o in ALIGN_CASES])
def test_alignment_matrix_equals_the_aligned_run_bit_for_bit(aligned, role, off):
    """Exactly one of p / g / m / v starts 1, 2 or 3 elements past a 16-byte boundary (the kernel takes its scalar loop), or the
    16-bit copy 1, 2 or 3 elements past an 8-byte one, or lp_table holds a zero between non-zero entries: the same arithmetic per
    element, so p, m, v and the copy equal the all-aligned run bit for bit; sumsq is summed in another order and stays in its bound."""
    null = (2, 4) if role == "lp_null" else ()
    got = _aligned_run(offs={role: off} if role != "lp_null" else None, lp_null=null)
    _, gsteps = _draw(ALIGN_HP["gs"])
    worst = 0.0
    for step in (1, 2):
        a, b = aligned[step - 1], got[step - 1]
        for k in ("p", "m", "v", "lp"):
            for t, (x, y) in enumerate(zip(a[k], b[k])):
                if k == "lp" and t in null:
                    assert bool((y == _ints(torch.full((1,), SENT[LPT], dtype=LPT))).all()), f"the copy of tensor {t} has no lp_table entry and was written"
                    continue
                bad = (x != y).nonzero().flatten()
                assert bad.numel() == 0, f"step {step}: {k} of tensor {t} (n {x.numel()}) differs from the aligned run at {bad[:8].tolist()}"
        worst = max(worst, _check_sumsq(b["sumsq"], gsteps[step - 1], R.RANDOM_LENGTHS, f"{role}+{off} step {step}"))
    worst = max(worst, _check_sumsq(got[2], gsteps[1], R.RANDOM_LENGTHS, f"mt_sumsq {role}+{off}"))
    parity(f"optim/align/{role}+{off}/sumsq", worst, 1.0)


# ------------------------------------------------------------------------------------------------ mt_finish_norm
@pytest.mark.parametrize("kind", ["none", "huge", "half"])
@pytest.mark.parametrize("nt", [1, 63, 64, 65, 200])
def test_finish_norm(nt, kind):
    s = (np.random.default_rng(nt).standard_normal(nt) ** 2 * 100).astype(np.float32)
    ref_norm = math.sqrt(float(s.astype(np.float64).sum()))
    max_norm = {"none": 0.0, "huge": 1e9, "half": 0.5 * ref_norm}[kind]
    S, O = Guarded([nt]), Guarded([2])
    S.load([s])
    S.snapshot(); O.snapshot()
    call("octmae_mt_finish_norm", S.views[0].data_ptr(), nt, max_norm, O.views[0].data_ptr(), O.views[0].data_ptr() + 4, _stream())
    torch.cuda.synchronize()
    S.assert_unchanged("mt_finish_norm: sumsq")
    O.assert_outside_unchanged("mt_finish_norm: outputs")
    norm, coef = (float(x) for x in O.views[0].cpu())
    ref_n, ref_c = R.finish_ref(s, max_norm)
    rn = abs(norm - ref_n) / (R.norm_factor(nt) * R.E * ref_n)
    rc = abs(coef - ref_c) / (R.norm_factor(nt) * R.E * ref_c)
    print(f"\nfinish_norm nt {nt} {kind}: norm {rn:.3f}, coef {rc:.3f} of the bound ({R.norm_factor(nt)} e)")
    if kind != "half":
        assert coef == 1.0
    else:
        assert 0.49 < ref_c < 0.51
    parity(f"optim/finish_norm/nt{nt}/{kind}/norm", rn, 1.0)
    parity(f"optim/finish_norm/nt{nt}/{kind}/coef", rc, 1.0)


# ------------------------------------------------------------------------------------------------ FusedAdamW.step(want_norm=True)
def _params(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=g).to(DEV)) for n in lengths]


def test_step_with_norm_equals_step_without_and_the_fp64_norm():
    """two groups of different tensor counts plus a group without gradients: the norm the AdamW kernels accumulate is the fp64 norm of
    the raw gradients within (max_t sumsq bound) / 2 + the finish bound over the whole (groups x widest group) sumsq array, and
    parameters and state equal a twin stepped without want_norm, bit for bit"""
    la, lb, lc = [5, 1027, 65539], [65536, 70000], [33]

    def make():
        a, b, c = _params(la, 1), _params(lb, 2), _params(lc, 3)
        opt = foptim.FusedAdamW([{"params": a, "weight_decay": 0.0}, {"params": b, "weight_decay": 0.05}, {"params": c}], lr=1e-3, betas=(0.9, 0.95))
        return a + b, c, opt

    (ps, idle, opt), (qs, idle2, twin) = make(), make()
    g = torch.Generator().manual_seed(4)
    factor = max(R.sumsq_factor(n) for n in la + lb) / 2 + R.norm_factor(3 * 3)
    for step in (1, 2):
        grads = [torch.randn(p.shape, generator=g) for p in ps]
        for p, q, gr in zip(ps, qs, grads):
            p.grad = gr.to(DEV); q.grad = gr.to(DEV)
        _, norm = opt.step(want_norm=True)
        twin.step()
        ref = math.sqrt(sum(float((gr.double() ** 2).sum()) for gr in grads))
        parity(f"optim/step_want_norm/step{step}", abs(float(norm) - ref) / (factor * R.E * ref), 1.0)
        for i, (p, q) in enumerate(zip(ps, qs)):
            assert torch.equal(p.detach(), q.detach()), f"parameter {i}"
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(opt.state[p][k], twin.state[q][k]), f"{k} of parameter {i}"
                assert bool((opt.state[p][k] != 0).any())
            assert torch.equal(p.grad, grads[i].to(DEV))
    assert not opt.state[idle[0]] and idle[0].grad is None


# ------------------------------------------------------------------------------------------------ host-side tables
def _norm64(t):
    return math.sqrt(float((t.double() ** 2).sum()))


def test_norm_table_is_rebuilt_for_the_same_pointers_at_another_size():
    """views of one buffer: the same data_ptr()s, 1000 then 500 elements, through the process-wide table cache of get_grad_norm_"""
    g = torch.Generator().manual_seed(21)
    buf, gbuf = torch.randn(1000, generator=g).to(DEV), torch.randn(1000, generator=g).to(DEV)
    for n in (1000, 500, 1000):
        p = torch.nn.Parameter(buf[:n])
        p.grad = gbuf[:n]
        assert p.data_ptr() == buf.data_ptr() and p.grad.data_ptr() == gbuf.data_ptr()
        got, ref = float(misc.get_grad_norm_([p])), _norm64(gbuf[:n])
        assert abs(got - ref) <= (R.sumsq_factor(n) / 2 + R.norm_factor(1)) * R.E * ref, f"norm of {n} elements: {got!r}, reference {ref!r}"


def test_adamw_table_is_rebuilt_for_the_same_pointers_at_another_size():
    """FusedAdamW: p.data, p.grad and a fresh state become shorter views of the same buffers; the step must update 500 elements and
    leave the other 500 of every buffer alone (all four buffers stay 1000 long: a stale table writes inside them, and is seen)"""
    g = torch.Generator().manual_seed(22)
    buf, gbuf = torch.randn(1000, generator=g).to(DEV), torch.randn(1000, generator=g).to(DEV)
    mbuf, vbuf = torch.zeros(1000, device=DEV), torch.zeros(1000, device=DEV)
    p = torch.nn.Parameter(buf[:1000])
    opt = foptim.FusedAdamW([p], lr=1e-3, betas=(0.9, 0.95), weight_decay=0.0)
    for n in (1000, 500):
        p.data = buf[:n]
        p.grad = gbuf[:n]
        mbuf.zero_(); vbuf.zero_()
        opt.state[p] = {"step": 0, "exp_avg": mbuf[:n], "exp_avg_sq": vbuf[:n]}
        opt.param_groups[0].pop("_step", None)
        before = buf.clone()
        opt.step()
        torch.cuda.synchronize()
        assert bool((buf[:n] != before[:n]).all()), "the step did not update the parameter"
        assert torch.equal(buf[n:], before[n:]), f"{int((buf[n:] != before[n:]).sum())} elements past the {n}-element parameter were updated"
        assert int(torch.count_nonzero(mbuf[n:])) == 0 and int(torch.count_nonzero(vbuf[n:])) == 0
        assert int(torch.count_nonzero(mbuf[:n])) == n


def test_zero_element_parameters():
    """only empty parameters: norm 0, the step is a no-op without error (as torch.optim.AdamW and the reference's get_grad_norm_);
    a mixed set ignores them"""
    empties = [torch.nn.Parameter(torch.empty(0, device=DEV)), torch.nn.Parameter(torch.empty(0, 3, device=DEV))]
    for p in empties:
        p.grad = torch.zeros_like(p)
    assert float(misc.get_grad_norm_(empties)) == 0.0
    norm, coef = foptim.grad_norm_and_coef(empties, 1.0, {})
    assert float(norm) == 0.0 and float(coef) == 1.0
    opt = foptim.FusedAdamW(empties, lr=1e-3)
    opt.step()
    _, n = opt.step(want_norm=True)
    assert float(n) == 0.0
    # mixed: the empty ones change nothing, in the norm or in the update of their neighbours
    real, twin = _params([1027, 5], 5), _params([1027, 5], 5)
    g = torch.Generator().manual_seed(6)
    for p, q in zip(real, twin):
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
        q.grad = p.grad.clone()
    mixed = [empties[0], real[0], empties[1], real[1]]
    ref = math.sqrt(sum(_norm64(p.grad) ** 2 for p in real))
    got = float(misc.get_grad_norm_(mixed))
    assert abs(got - ref) <= (R.sumsq_factor(1027) / 2 + R.norm_factor(4)) * R.E * ref
    o1, o2 = foptim.FusedAdamW(mixed, lr=1e-3), foptim.FusedAdamW(twin, lr=1e-3)
    _, n1 = o1.step(want_norm=True)
    o2.step()
    assert abs(float(n1) - ref) <= (R.sumsq_factor(1027) / 2 + R.norm_factor(4)) * R.E * ref
    for p, q in zip(real, twin):
        assert torch.equal(p.detach(), q.detach()) and torch.equal(o1.state[p]["exp_avg_sq"], o2.state[q]["exp_avg_sq"])


def _layout_case(kind):
    """(parameter, gradient) of logical shape (8, 16); whatever flat memory a table WITHOUT a layout check would read lies inside a
    live allocation (the expanded gradient is a view of a 1024-element buffer)"""
    g = torch.Generator().manual_seed(31)
    w0, g0 = torch.randn(8, 16, generator=g), torch.randn(8, 16, generator=g)
    if kind == "transposed_param":
        p = torch.nn.Parameter(w0.t().contiguous().to(DEV).t())                 # logical (8, 16), strides (1, 8)
        grad = g0.to(DEV)
    elif kind == "transposed_grad":
        p = torch.nn.Parameter(w0.to(DEV))
        grad = g0.t().contiguous().to(DEV).t()
    else:
        big = torch.randn(1024, generator=g)
        g0 = big[:16].expand(8, 16)
        p = torch.nn.Parameter(w0.to(DEV))
        grad = big.to(DEV)[:16].expand(8, 16)
    assert not (p.is_contiguous() and grad.is_contiguous()) and torch.equal(p.detach().cpu(), w0) and torch.equal(grad.cpu(), g0)
    return p, grad, w0, g0


@pytest.mark.parametrize("kind", ["transposed_param", "transposed_grad", "expanded_grad"])
def test_non_contiguous_tensors_raise_or_match_torch_adamw(kind):
    """never silently different: a clear ValueError that leaves parameter and step count alone, or torch.optim.AdamW's result per
    LOGICAL element, exp_avg and exp_avg_sq of state_dict() included; the same for the norm of an expanded gradient"""
    p, grad, w0, g0 = _layout_case(kind)
    kw = dict(lr=1e-2, betas=(0.9, 0.95), weight_decay=0.05)
    q = torch.nn.Parameter(w0.clone().double())
    q.grad = g0.clone().double()
    ref = torch.optim.AdamW([q], **kw)
    ref.step()
    p.grad = grad
    opt = foptim.FusedAdamW([p], **kw)
    try:
        opt.step()
    except ValueError as e:
        assert "contiguous" in str(e)
        assert torch.equal(p.detach().cpu(), w0) and "_step" not in opt.param_groups[0]
    else:
        sd, rd = opt.state_dict()["state"][0], ref.state_dict()["state"][0]
        for got, exp in ((p.detach(), q.detach()), (sd["exp_avg"], rd["exp_avg"]), (sd["exp_avg_sq"], rd["exp_avg_sq"])):
            assert got.shape == exp.shape
            err = (got.cpu().double() - exp).abs().max() / exp.abs().max()
            assert float(err) < 1e-6, f"{kind}: differs from torch.optim.AdamW per logical element ({float(err):.2e})"
    try:
        n = float(misc.get_grad_norm_([p]))
    except ValueError as e:
        assert "contiguous" in str(e)
    else:
        assert abs(n - _norm64(g0)) <= 1e-6 * _norm64(g0)
