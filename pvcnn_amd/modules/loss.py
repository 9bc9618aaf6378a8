"""KLLoss module (reference: modules/loss.py:6-9) and CrossEntropyLoss, nn.CrossEntropyLoss on the fused criterion."""
import torch
import torch.nn as nn

from . import functional as F
from .functional.loss import _cross_entropy

__all__ = ['KLLoss', 'CrossEntropyLoss']


class KLLoss(nn.Module):
    def forward(self, x, y):
        return F.kl_loss(x, y)


class CrossEntropyLoss(nn.CrossEntropyLoss):
    """nn.CrossEntropyLoss (same constructor, `weight` buffer and state_dict) whose forward is F.cross_entropy: on device logits
    (B, C, N) with int64 targets the loss and its gradient are three HIP launches, anything else is torch's.

    `bad_targets`: a 0-dim int64 tensor on the input's device (None until the first fused call), the running number of targets
    outside [0, C) that were not ignore_index.  Such points are treated as ignored instead of faulting; the kernels add to the
    counter, so reading it costs a synchronisation -- look at it between epochs, not inside the loop."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.bad_targets = None

    @classmethod
    def from_torch(cls, criterion):
        """The same criterion as an nn.CrossEntropyLoss instance: weight, ignore_index, reduction and label_smoothing are taken over."""
        if not isinstance(criterion, nn.CrossEntropyLoss):
            raise TypeError(f'from_torch expects an nn.CrossEntropyLoss, got {type(criterion).__name__}')
        return cls(weight=criterion.weight, ignore_index=criterion.ignore_index, reduction=criterion.reduction,
                   label_smoothing=criterion.label_smoothing)

    def forward(self, input, target):
        counter = None
        fused = F.cross_entropy_is_fused(input, target, self.weight, self.reduction)
        if fused:
            if self.bad_targets is None or self.bad_targets.device != input.device:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError('CrossEntropyLoss: call the criterion once before capturing it (its bad_targets counter is '
                                       'created on the first call; GraphedTrainStep\'s warm-up steps do that)')
                self.bad_targets = torch.zeros((), dtype=torch.int64, device=input.device)
            counter = self.bad_targets
        return _cross_entropy(input, target, self.weight, self.ignore_index, self.reduction, self.label_smoothing, counter, fused)
