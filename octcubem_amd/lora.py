"""Low-rank adapters (LoRA) on the four Linears of the fused Block: parameter-efficient fine-tuning.

``attach(model)`` freezes every parameter of the Blocks it adapts and registers ``blk.lora`` with the parameters ``<target>_A [r, I]``
and ``<target>_B [O, r]`` (targets ``qkv``, ``proj``, ``fc1``, ``fc2``).  An adapted Linear computes with ``W + (alpha / r) B A``:
the Block's GEMMs run unchanged on a MERGED 16-bit operand that ``ops.lora_merge`` writes into a buffer the Block owns (the model's
operand arena stays the cast of the master weights), and the backward takes the adapter gradients from skinny products over the
activations and output gradients the weight-gradient GEMMs would have read (``ops.lora_wgrad``, csrc/lora.hip).  No gradient of a base
parameter of an adapted Block is produced, no gradient-arena slice of one is written.

The arithmetic is that of a full fine-tune whose fp32 master weights ``W + s B A`` are rounded once to the operand type;
``merge_and_unload`` folds exactly those fp32 values into the master weights, so the folded model's outputs are bit-identical.

The merged operands are rebuilt on every forward of a Block in training mode (``FusedAdamW`` writes parameters through raw pointers
that no version counter sees) and, in eval mode, when something changed: ``train()`` / ``eval()``, the loaders of this module, a
refresh of the operand arena (any write PyTorch's version counters see), a new arena."""
from __future__ import annotations

import math
from typing import Dict, Iterable, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import ops
from .arena import bind_arena
from .video_vit import Attention, Block, FlashMixer, TimmAttention

TARGETS = ("qkv", "proj", "fc1", "fc2")
_LP_SLOT = {"qkv": 0, "proj": 2, "fc1": 4, "fc2": 6}      # where a target's weight sits in BlockFn's operand tuple


class LoraBundle:
    """What ops.BlockFn needs of an adapted Block for one forward + backward: ``lp`` -- the Block's operand tuple with the merged
    weights in place of the adapted ones --, ``params`` -- the adapter parameters (inputs of the autograd node, notified when their
    gradients are complete) --, and ``wgrad(target, x, dy)``, which adds the adapter gradients of one Linear (nothing for a target
    without an adapter)."""

    def __init__(self, lp, params, layers):
        self.lp, self.params, self._layers = lp, params, layers

    def has(self, target: str) -> bool:
        return target in self._layers

    def wgrad(self, target: str, x: torch.Tensor, dy: torch.Tensor):
        ent = self._layers.get(target)
        if ent is None:
            return
        A, B, A_lp, B_lp, s, r = ent
        gA = ops.grad_buf(A) if A.requires_grad else None
        gB = ops.grad_buf(B) if B.requires_grad else None
        if gA is None and gB is None:
            return
        ops.lora_wgrad(x.view(-1, x.shape[-1]), dy.view(-1, dy.shape[-1]), A_lp, B_lp, s, r, gA, gB)


def _base_weights(blk: Block, arena) -> Dict[str, torch.Tensor]:
    """fp32 [O, I] views of the four master weights of a fused Block, in the arena (the q | k | v weights as one [3 D, D] view)"""
    a, m = blk.attn, blk.mlp
    if isinstance(a, Attention):
        D = a.q.weight.shape[0]
        qkv, proj = arena.f32_view(a.q.weight, a.v.weight, (3 * D, D)), arena.f32_view(a.proj.weight)
    elif isinstance(a, TimmAttention):
        qkv, proj = arena.f32_view(a.qkv.weight), arena.f32_view(a.proj.weight)
    else:
        qkv, proj = arena.f32_view(a.Wqkv.weight), arena.f32_view(a.out_proj.weight)
    return {"qkv": qkv, "proj": proj, "fc1": arena.f32_view(m.fc1.weight), "fc2": arena.f32_view(m.fc2.weight)}


def _layer_shapes(blk: Block) -> Dict[str, Tuple[int, int]]:
    a, m = blk.attn, blk.mlp
    if isinstance(a, Attention):
        D = a.q.weight.shape[0]
        qkv, proj = (3 * D, D), tuple(a.proj.weight.shape)
    elif isinstance(a, TimmAttention):
        qkv, proj = tuple(a.qkv.weight.shape), tuple(a.proj.weight.shape)
    else:
        qkv, proj = tuple(a.Wqkv.weight.shape), tuple(a.out_proj.weight.shape)
    return {"qkv": qkv, "proj": proj, "fc1": tuple(m.fc1.weight.shape), "fc2": tuple(m.fc2.weight.shape)}


def _is_fused(blk: Block) -> bool:
    return isinstance(blk.attn, (Attention, TimmAttention, FlashMixer)) and isinstance(blk.norm1, nn.LayerNorm) and \
        isinstance(blk.norm2, nn.LayerNorm)


class LoraAdapters(nn.Module):
    """The adapters of one Block: parameters ``<target>_A`` / ``<target>_B``; the merged operands and the padded 16-bit copies of the
    adapters are plain attributes (no state-dict keys)."""

    def __init__(self, shapes: Dict[str, Tuple[int, int]], rank: int, alpha: float, targets: Sequence[str], frozen_before: Dict[str, bool]):
        super().__init__()
        self.rank, self.alpha, self.targets = int(rank), float(alpha), tuple(targets)
        self.scale = self.alpha / self.rank
        self.frozen_before = frozen_before                    # name inside the Block -> requires_grad before attach
        for t in self.targets:
            O, I = shapes[t]
            A = torch.empty(self.rank, I)
            nn.init.kaiming_uniform_(A, a=math.sqrt(5))
            self.register_parameter(f"{t}_A", nn.Parameter(A))
            self.register_parameter(f"{t}_B", nn.Parameter(torch.zeros(O, self.rank)))
        self._gen = 0
        self._state = None
        self._bundle: Optional[LoraBundle] = None
        self._bufs: Dict[str, tuple] = {}

    def train(self, mode: bool = True):
        self._gen += 1                                        # train() / eval(): the next forward merges again
        return super().train(mode)

    def invalidate(self):
        self._gen += 1

    def _buffers_for(self, t: str, O: int, I: int, dev):
        b = self._bufs.get(t)
        if b is None or b[0].device != dev:
            rp = ops.lora_rp(self.rank)
            b = self._bufs[t] = (torch.empty((O, I), dtype=ops.BF16, device=dev), torch.empty((rp, I), dtype=ops.BF16, device=dev),
                                 torch.empty((O, rp), dtype=ops.BF16, device=dev))
        return b

    def bundle(self, blk: Block) -> LoraBundle:
        arena, lp, _, _ = blk._v()
        state = (id(arena), arena._lp_state, self._gen, blk.training)
        if self._bundle is not None and not blk.training and state == self._state:
            return self._bundle
        base = _base_weights(blk, arena)
        merged, layers, params = list(lp), {}, []
        for t in self.targets:
            A, B = getattr(self, f"{t}_A"), getattr(self, f"{t}_B")
            W = base[t]
            w_lp, A_lp, B_lp = self._buffers_for(t, W.shape[0], W.shape[1], W.device)
            ops.lora_merge(W, A.data, B.data, self.scale, w_lp, A_lp, B_lp)
            merged[_LP_SLOT[t]] = w_lp
            layers[t] = (A, B, A_lp, B_lp, self.scale, self.rank)
            params += [A, B]
        self._bundle = LoraBundle(tuple(merged), tuple(params), layers)
        self._state = state
        return self._bundle


def _blocks_of(model: nn.Module):
    return [(name, m) for name, m in model.named_modules() if isinstance(m, Block)]


def adapted_blocks(model: nn.Module):
    return [(name, m) for name, m in _blocks_of(model) if "lora" in m._modules]


def _rebind(model: nn.Module):
    """parameters were added or removed: the arena of the model (bound by its first forward) is built again around the new set"""
    arena = getattr(model, "_arena", None)
    if arena is None:
        return
    root = arena.root()
    bind_arena(root if root is not None else model)


def attach(model: nn.Module, rank: int = 8, alpha: float = 16, targets: Iterable[str] = TARGETS, blocks: Optional[Iterable[int]] = None,
           lora_dropout: float = 0.0):
    """Adapters of rank ``rank`` on the ``targets`` of every fused Block under ``model`` (``blocks``: only the Blocks at these positions
    of the list of Blocks, in module order).  ``A`` is kaiming-uniform (a = sqrt(5)), ``B`` zero: the adapted model starts as the base
    model.  Every other parameter of an adapted Block is frozen (``requires_grad = False``, ``grad = None``).  Returns the adapter
    parameters."""
    assert lora_dropout == 0.0, "adapter dropout is not built"
    targets = tuple(targets)
    if not targets or any(t not in TARGETS for t in targets):
        raise ValueError(f"attach: targets must be among {TARGETS}, got {targets}")
    rank = int(rank)
    if not 1 <= rank <= ops.LORA_MAX_RANK:
        raise ValueError(f"attach: rank {rank} outside 1 .. {ops.LORA_MAX_RANK}")
    found = _blocks_of(model)
    if blocks is not None:
        want = set(int(i) for i in blocks)
        if not want <= set(range(len(found))):
            raise ValueError(f"attach: blocks {sorted(want)} of a model with {len(found)} Blocks")
        found = [nb for i, nb in enumerate(found) if i in want]
    if not found:
        raise ValueError("attach: the model has no Block")
    for name, blk in found:
        if not _is_fused(blk):
            raise NotImplementedError(f"attach: {name or 'the module'} runs on the unfused path (adapters sit on the fused Block only)")
        if "lora" in blk._modules:
            raise RuntimeError(f"attach: {name or 'the module'} already has adapters")
    out = []
    for name, blk in found:
        frozen_before = {n: p.requires_grad for n, p in blk.named_parameters()}
        for p in blk.parameters():
            p.requires_grad = False
            p.grad = None
        ad = LoraAdapters(_layer_shapes(blk), rank, alpha, targets, frozen_before)
        ad.to(next(blk.parameters()).device)
        ad.train(blk.training)
        blk.lora = ad
        if hasattr(blk, "_views"):
            object.__setattr__(blk, "_views", None)
        out += list(ad.parameters())
    _rebind(model)
    return out


def mark_only_lora_trainable(model: nn.Module, also: Sequence[str] = ("head", "fc_norm", "norm")):
    """Freeze everything but the adapters and the parameters whose first name component is in ``also``; frozen parameters give up
    their gradient.  Returns the trainable parameters."""
    out = []
    for name, p in model.named_parameters():
        keep = ".lora." in f".{name}" or name.split(".")[0] in also
        p.requires_grad = keep
        if keep:
            out.append(p)
        else:
            p.grad = None
    return out


def _selected(name: str, also: Sequence[str]) -> bool:
    return ".lora." in f".{name}" or name.split(".")[0] in also


def lora_state_dict(model: nn.Module, also: Sequence[str] = ("head", "fc_norm", "norm")):
    """The per-task checkpoint: the adapters and the ``also`` modules, detached clones under the model's own keys"""
    return {k: v.detach().clone() for k, v in model.state_dict().items() if _selected(k, also)}


def load_lora_state_dict(model: nn.Module, sd, strict: bool = True):
    """Load what ``lora_state_dict`` saved.  ``strict``: every adapter key of the model must be present and no key may be unknown."""
    own = model.state_dict()
    unknown = [k for k in sd if k not in own]
    missing = [k for k in own if ".lora." in f".{k}" and k not in sd]
    if strict and (unknown or missing):
        raise RuntimeError(f"load_lora_state_dict: unexpected keys {unknown}, missing adapter keys {missing}")
    res = model.load_state_dict({k: v for k, v in sd.items() if k in own}, strict=False)
    for _, blk in adapted_blocks(model):
        blk.lora.invalidate()
    return res


@torch.no_grad()
def merge_and_unload(model: nn.Module):
    """Fold ``W + s B A`` -- the fp32 values the merged operands are the rounding of -- into the master weights and remove the
    adapters: the state-dict keys and the ``requires_grad`` pattern are the ones before ``attach``, the outputs bit-identical to the
    adapted model's.  Needs the model on the GPU."""
    touched = []
    for _, blk in adapted_blocks(model):
        ad = blk.lora
        arena, _, _, _ = blk._v()
        base = _base_weights(blk, arena)
        for t in ad.targets:
            W = base[t]
            v = torch.empty_like(W)
            ops.lora_merge(W, getattr(ad, f"{t}_A").data, getattr(ad, f"{t}_B").data, ad.scale, v)
            W.copy_(v)
        arena.invalidate_lp()                                  # written through the arena's own views: no version counter saw it
        touched.append(arena)
        del blk.lora
        for n, p in blk.named_parameters():
            p.requires_grad = ad.frozen_before.get(n, p.requires_grad)
        object.__setattr__(blk, "_views", None)
    _rebind(model)
    return model
