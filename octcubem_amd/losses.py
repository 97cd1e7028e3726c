"""Classification criteria the reference's fine-tune drivers pick from (OCTCube/main_finetune.py:305-312): timm's
``LabelSmoothingCrossEntropy`` / ``SoftTargetCrossEntropy`` (timm is not a dependency here) next to torch's own
``CrossEntropyLoss`` / ``BCEWithLogitsLoss``, and the reference's own ``WeightedLabelSmoothingCrossEntropy``
(OCTCube/util/WeightedLabelSmoothingCrossEntropy.py; picked at main_finetune_downstream_inhouse_singlefold.py:619 / :1145 for targets
with all-zero rows) and the multi-task split of multi-label targets that feeds it (OCTCube/engine_finetune.py:36-70).  They act on ``[B, num_classes]`` logits -- host-side torch ops, not a hot kernel."""
import torch
import torch.nn as nn
import torch.nn.functional as F
from ._autocast import autocast_invariant, no_autocast


@autocast_invariant
class LabelSmoothingCrossEntropy(nn.Module):
    """NLL loss with label smoothing: mean_i[(1 - s) * nll_i + s * mean_c(-log p_ic)]."""

    def __init__(self, smoothing=0.1):
        super().__init__()
        assert smoothing < 1.0
        self.smoothing = smoothing
        self.confidence = 1.0 - smoothing

    def forward(self, x, target):
        logprobs = F.log_softmax(x.float(), dim=-1)
        nll_loss = -logprobs.gather(dim=-1, index=target.unsqueeze(1)).squeeze(1)
        smooth_loss = -logprobs.mean(dim=-1)
        return (self.confidence * nll_loss + self.smoothing * smooth_loss).mean()


@autocast_invariant
class SoftTargetCrossEntropy(nn.Module):
    """Cross entropy against a probability vector (what mixup / cutmix produce)."""

    def forward(self, x, target):
        return torch.sum(-target * F.log_softmax(x.float(), dim=-1), dim=-1).mean()


@autocast_invariant
class WeightedLabelSmoothingCrossEntropy(nn.Module):
    """Label-smoothing NLL against one-hot rows, over the rows that carry a label: a target row that sums to 0 counts neither in the
    numerator nor in the denominator.  The class of a row is its argmax.  No valid row: ``x.mean() * 0`` -- a zero that still reaches
    every logit, so the gradient is zeros and not None."""

    def __init__(self, smoothing=0.1):
        super().__init__()
        assert smoothing < 1.0
        self.smoothing = smoothing
        self.confidence = 1.0 - smoothing

    def forward(self, x, target):
        x = x.float()
        valid = (target.sum(dim=-1) != 0).float()
        n_valid = valid.sum()
        if n_valid == 0:
            return x.mean() * 0
        logprobs = F.log_softmax(x, dim=-1)
        nll_loss = -logprobs.gather(dim=-1, index=target.argmax(dim=-1).unsqueeze(1)).squeeze(1)
        smooth_loss = -logprobs.mean(dim=-1)
        loss = (self.confidence * nll_loss + self.smoothing * smooth_loss) * valid
        return loss.sum() / n_valid


def multi_task_targets(target):
    """OCTCube/engine_finetune.py:36-43 (multi_label_target_to_multi_task_target): multi-label rows ``target`` [B, T + 1], column 0
    the shared "normal" label, as one two-class problem per task: ``target_mt`` [B, T, 2] = (target[:, 0], target[:, i + 1]) and
    ``weight`` [B, T] = their sum, 0 for a sample that belongs to neither side of task i.  Dtype and device of ``target``."""
    if target.dim() != 2 or target.shape[1] < 2:
        raise ValueError(f"multi_task_targets: expected target [B, T + 1], got {tuple(target.shape)}")
    B, T = target.shape[0], target.shape[1] - 1
    target_mt = torch.stack([target[:, :1].expand(B, T), target[:, 1:]], dim=2)
    return target_mt, target_mt.sum(dim=2)


@no_autocast          # what autocast_invariant puts around a class's forward
def multi_task_loss(output, target, criterion, multi_task_type="multi_task_default"):
    """OCTCube/engine_finetune.py:45-70: ``sum_i criterion(output_i, target_i) / (weight.sum() + 1e-8)`` over the T tasks of
    ``multi_task_targets(target)``.  ``output`` holds the logits: [B, 2T] read as [B, T, 2] for 'multi_task_default', [B, T + 1] for
    any other type, where task i uses columns (0, i + 1).  With ``WeightedLabelSmoothingCrossEntropy`` all tasks are computed in one
    batched pass; a task with no valid row contributes a zero that still reaches its logits, as the criterion's own ``x.mean() * 0``
    does.  Any other criterion is called once per task, as in the reference (``FocalLoss2d`` is not built: INTEGRATION.md, section 1f)."""
    target_mt, weight = multi_task_targets(target)
    B, T = weight.shape
    if output.dim() != 2 or output.shape[0] != B:
        raise ValueError(f"multi_task_loss: expected output [{B}, ...] for target {tuple(target.shape)}, got {tuple(output.shape)}")
    if multi_task_type == "multi_task_default":
        if output.shape[1] != 2 * T:
            raise ValueError(f"multi_task_loss: {T} tasks need output [B, {2 * T}] in the default layout, got {tuple(output.shape)}")
        pairs = output.reshape(B, T, 2)
    else:
        if output.shape[1] != T + 1:
            raise ValueError(f"multi_task_loss: {T} tasks need output [B, {T + 1}] in the shared-column layout, got {tuple(output.shape)}")
        pairs = torch.stack([output[:, :1].expand(B, T), output[:, 1:]], dim=2)
    denom = weight.sum() + 1e-8
    if isinstance(criterion, WeightedLabelSmoothingCrossEntropy):
        valid = (weight != 0).float()                                   # [B, T]
        logprobs = F.log_softmax(pairs.float(), dim=-1)
        nll = -logprobs.gather(dim=-1, index=target_mt.long().argmax(dim=-1, keepdim=True)).squeeze(-1)
        smooth = -logprobs.mean(dim=-1)
        per_row = (criterion.confidence * nll + criterion.smoothing * smooth) * valid
        # a task without a valid row: 0 / 1, a zero with a (zero) gradient to its logits
        per_task = per_row.sum(dim=0) / valid.sum(dim=0).clamp(min=1.0)
        return per_task.sum() / denom
    loss = 0
    for i in range(T):
        loss = loss + criterion(pairs[:, i], target_mt[:, i].long())
    return loss / denom
