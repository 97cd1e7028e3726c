"""Classification criteria the reference's fine-tune drivers pick from (OCTCube/main_finetune.py:305-312): timm's
``LabelSmoothingCrossEntropy`` / ``SoftTargetCrossEntropy`` (timm is not a dependency here) next to torch's own
``CrossEntropyLoss`` / ``BCEWithLogitsLoss``, and the reference's own ``WeightedLabelSmoothingCrossEntropy``
(OCTCube/util/WeightedLabelSmoothingCrossEntropy.py; picked at main_finetune_downstream_inhouse_singlefold.py:619 / :1145 for targets
with all-zero rows).  They act on ``[B, num_classes]`` logits -- host-side torch ops, not a hot kernel."""
import torch
import torch.nn as nn
import torch.nn.functional as F
from ._autocast import autocast_invariant


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
