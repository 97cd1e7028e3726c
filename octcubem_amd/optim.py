"""Fused multi-tensor AdamW + gradient-norm kernels behind the torch.optim.Optimizer interface.

Replaces ``torch.optim._multi_tensor.AdamW(param_groups, lr, betas=(0.9, 0.95))`` as built by the reference
driver (main_pretrain_oph_joint_2d512_flash_attn.py:441-455): same param_groups / lr / lr_scale contract, so
``lr_sched.adjust_learning_rate`` and ``misc.add_weight_decay`` work unchanged.  One kernel launch per group
(16 B read + 12 B written per parameter), gradient clip / unscale folded in as a device-side scale.
"""
from __future__ import annotations

import os
import struct
from typing import List, Optional

import torch

from ._lib import call
from .ops import _stream, is_deterministic


def _entry_key(p, g, m=None, v=None):
    """What a table holds of one tensor, plus what it relies on: the kernels read p, g, m and v as flat memory of p.numel() elements.
    The element count is part of it (views of one buffer, or an allocator block handed to another model, share pointers and not
    sizes), and so is the layout (a gradient replaced by a transposed view of itself keeps its pointer)."""
    return (p.data_ptr(), g.data_ptr() if g is not None else 0, m.data_ptr() if m is not None else 0,
            v.data_ptr() if v is not None else 0, p.numel(), p.is_contiguous() and (g is None or g.is_contiguous()))


class _MultiTensorTable:
    """Device-side tables for a list of (p, g, m, v) tensors: octmae_mt_* calling convention.  ``lps``: per tensor the device
    address of the 16-bit operand copy of p (0: none) -- the optional table octmae_mt_adamw_fused writes through.
    Every tensor must be contiguous and of p's element count: the kernels pair element i of p with element i of g, m and v in
    memory order, so a transposed or expanded gradient, or a parameter in a permuted layout, would be silently mis-paired
    (ValueError instead; arena tensors are always contiguous).  Zero-element tensors take part and have no chunks; a table whose
    tensors are all empty has n_chunks == 0 and must not be launched (the entry points reject an empty grid)."""

    def __init__(self, ps: List[torch.Tensor], gs, ms, vs, lps=None):
        from ._lib import load
        chunk = load().octmae_mt_chunk_elems()
        dev = ps[0].device
        raw = bytearray()
        ct, co = [], []
        for i, (p, g, m, v) in enumerate(zip(ps, gs, ms, vs)):
            n = p.numel()
            for name, t in (("parameter", p), ("gradient", g), ("exp_avg", m), ("exp_avg_sq", v)):
                if t is None:
                    continue
                if t.numel() != n or not t.is_contiguous():
                    raise ValueError(f"multi-tensor optimizer kernels need contiguous tensors of the parameter's size: {name} {i} has "
                                     f"shape {tuple(t.shape)}, strides {tuple(t.stride())} (parameter: shape {tuple(p.shape)}); "
                                     "make it contiguous (e.g. p.grad = p.grad.contiguous())")
            raw += struct.pack("<QQQQq", p.data_ptr(), g.data_ptr() if g is not None else 0,
                               m.data_ptr() if m is not None else 0, v.data_ptr() if v is not None else 0, n)
            for off in range(0, n, chunk):
                ct.append(i); co.append(off)
        self.n_tensors = len(ps)
        self.n_chunks = len(ct)
        self.table = torch.frombuffer(raw, dtype=torch.uint8).clone().to(dev)
        self.chunk_tensor = torch.tensor(ct, dtype=torch.int32, device=dev)
        self.chunk_off = torch.tensor(co, dtype=torch.int64, device=dev)
        self._partial = None
        self.lp_table = None
        if lps is not None and any(lps):
            self.lp_table = torch.tensor([int(a) for a in lps], dtype=torch.int64, device=dev)
        # every pointer the table holds is part of its identity: a loaded optimizer state replaces exp_avg / exp_avg_sq
        self.key = tuple(_entry_key(p, g, m, v) for p, g, m, v in zip(ps, gs, ms, vs))

    def partial_ws(self) -> torch.Tensor:
        """Deterministic mode: the fp32 [n_chunks] workspace the sum-of-squares kernels leave one partial per chunk in."""
        if self._partial is None:
            self._partial = torch.empty(max(self.n_chunks, 1), dtype=torch.float32, device=self.table.device)
        return self._partial


def grad_norm_and_coef(params, max_norm: Optional[float], cache: dict):
    """get_grad_norm_ (misc.py:356-373) / clip_grad_norm_ statistics in two launches.
    Returns (total_norm, clip_coef) as 0-dim device tensors; clip_coef == 1 when max_norm is None."""
    ps = [p for p in params if p.grad is not None]
    if not ps:
        return torch.tensor(0.0), None
    key = tuple(_entry_key(p, p.grad) for p in ps)
    tab = cache.get("norm")
    if tab is None or tab.key != key:
        tab = _MultiTensorTable([p.data for p in ps], [p.grad for p in ps], [None] * len(ps), [None] * len(ps))
        cache["norm"] = tab
    dev = ps[0].device
    sumsq = torch.zeros(tab.n_tensors, dtype=torch.float32, device=dev)
    out = torch.empty(2, dtype=torch.float32, device=dev)
    if tab.n_chunks:                                       # every gradient empty: the norm of nothing is 0
        if is_deterministic():
            call("octmae_mt_sumsq_ws", tab.table.data_ptr(), tab.chunk_tensor.data_ptr(), tab.chunk_off.data_ptr(), tab.n_chunks,
                 sumsq.data_ptr(), tab.partial_ws().data_ptr(), _stream())
        else:
            call("octmae_mt_sumsq", tab.table.data_ptr(), tab.chunk_tensor.data_ptr(), tab.chunk_off.data_ptr(), tab.n_chunks,
                 sumsq.data_ptr(), _stream())
    call("octmae_mt_finish_norm", sumsq.data_ptr(), tab.n_tensors, float(max_norm) if max_norm is not None else 0.0,
         out.data_ptr(), out.data_ptr() + 4, _stream())
    return out[0], out[1]


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._tables = {}
        self._grad_scale: Optional[torch.Tensor] = None   # device scalar multiplied into every gradient
        # write_mirror: the AdamW kernel also writes the 16-bit operand copy (arena.ParamArena.lp) of every parameter it updates, so
        # the next forward needs no cast pass over the arena (OCTMAE_ADAMW_MIRROR=0: same-box A/B; the arena then re-casts)
        self.write_mirror = os.environ.get("OCTMAE_ADAMW_MIRROR", "1") != "0"

    def load_state_dict(self, state_dict):
        """The moment buffers are replaced: drop the device pointer tables (they are rebuilt on the next step)."""
        super().load_state_dict(state_dict)
        self._tables = {}

    def set_grad_scale(self, scale: Optional[torch.Tensor]):
        self._grad_scale = scale

    def zero_grad(self, set_to_none: bool = False):
        """Gradients are views of one arena: they are zeroed in place, never detached -- and when the gradients of this
        optimizer are views of ONE flat buffer (the model's gradient arena), with one fill per contiguous RUN of them instead
        of one launch per parameter (~500 per step for ViT-L; a single run when this optimizer holds every trainable
        parameter).  Only bytes this optimizer owns are touched: two gradients join a run only when the second starts where
        the first ends or at the next arena alignment boundary, so a slice that belongs to a parameter of another optimizer
        (or to one that is accumulating for a later step) is never inside a fill."""
        grads = [p.grad for group in self.param_groups for p in group["params"] if p.grad is not None]
        if not grads:
            return
        base = grads[0]._base
        if base is None or base.dim() != 1 or not all(g._base is base and g.is_contiguous() for g in grads):
            for g in grads:
                g.zero_()
            return
        from .arena import ALIGN
        spans = sorted((g.storage_offset() - base.storage_offset(), g.numel()) for g in grads)
        start, end = spans[0][0], spans[0][0] + spans[0][1]
        for o, n in spans[1:]:
            if o == end or o == (end + ALIGN - 1) // ALIGN * ALIGN:
                end = o + n
            else:
                base[start:end].zero_()
                start, end = o, o + n
        base[start:end].zero_()

    def grads_key(self):
        """Identity of the set of gradients a step() will consume (misc.NativeScalerWithGradNormCount compares it with the set it is
        asked to take the norm of before it lets the optimizer produce that norm itself)."""
        return frozenset(id(p) for g in self.param_groups for p in g["params"] if p.grad is not None)

    @torch.no_grad()
    def step(self, closure=None, want_norm: bool = False):
        """want_norm: also return the 2-norm of the (raw, un-scaled) gradients this step consumed, accumulated by the AdamW kernels
        themselves (one read of the gradients for norm and update) -> (loss, norm) instead of loss."""
        from . import arena as _arena
        loss = closure() if closure is not None else None
        sumsq = None
        # first the tables of every group (a tensor the kernels cannot take raises here, before any group has been stepped) ...
        work = []
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            for p in ps:
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            key = tuple(_entry_key(p, p.grad, self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"]) for p in ps)
            tab = self._tables.get(gi)
            if tab is None or tab.key != key or tab.mirror != self.write_mirror:
                owners = [_arena.arena_of(p) for p in ps]
                lps = [(a.lp_ptr(p) if (a is not None and self.write_mirror) else 0) for a, p in zip(owners, ps)]
                tab = _MultiTensorTable([p.data for p in ps], [p.grad for p in ps], [self.state[p]["exp_avg"] for p in ps],
                                        [self.state[p]["exp_avg_sq"] for p in ps], lps)
                tab.mirror = self.write_mirror
                # arenas whose parameters this group updates WITHOUT writing their operand copy: they must re-cast
                tab.stale_arenas = [a for a in {id(a): a for a, lp in zip(owners, lps) if a is not None and lp == 0}.values()]
                self._tables[gi] = tab
            work.append((gi, group, ps, tab))
        # ... then the steps
        for gi, group, ps, tab in work:
            if "_step" not in group:
                # a state loaded from torch.optim.AdamW carries the count per parameter ("step", int or tensor), not per
                # group: continue from it so that the bias correction does not restart
                steps = [self.state[p].get("step", 0) for p in ps]
                group["_step"] = int(max(float(s_) for s_ in steps)) if steps else 0
            group["_step"] += 1
            for p in ps:
                self.state[p]["step"] = group["_step"]
            for a in tab.stale_arenas:
                a.invalidate_lp()
            if want_norm and sumsq is None:
                n_max = max(len(w[2]) for w in work)
                sumsq = torch.zeros((len(self.param_groups), n_max), dtype=torch.float32, device=ps[0].device)
            if not tab.n_chunks:                           # only zero-element parameters: nothing to update
                continue
            b1, b2 = group["betas"]
            gs = self._grad_scale
            head = (tab.table.data_ptr(), tab.chunk_tensor.data_ptr(), tab.chunk_off.data_ptr(), tab.n_chunks,
                    gs.data_ptr() if gs is not None else None, tab.lp_table.data_ptr() if tab.lp_table is not None else None,
                    sumsq[gi].data_ptr() if sumsq is not None else None)
            tail = (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]), int(group["_step"]), _stream())
            if sumsq is not None and is_deterministic():      # the by-product through per-chunk partials, added in chunk order
                call("octmae_mt_adamw_fused_ws", *head, tab.partial_ws().data_ptr(), *tail)
            else:
                call("octmae_mt_adamw_fused", *head, *tail)
        if not want_norm:
            return loss
        if sumsq is None:
            return loss, torch.tensor(0.0)
        out = torch.empty(2, dtype=torch.float32, device=sumsq.device)
        call("octmae_mt_finish_norm", sumsq.data_ptr(), sumsq.numel(), 0.0, out.data_ptr(), out.data_ptr() + 4, _stream())
        return loss, out[0]
