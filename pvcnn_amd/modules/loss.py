"""KLLoss module (reference: modules/loss.py:6-9; fused through F.kl_loss), CrossEntropyLoss, nn.CrossEntropyLoss on the fused
criterion, DMLPairLoss, the two losses of a deep-mutual-learning step from one pass over both networks' logits, LovaszSoftmax, the
IoU surrogate of Berman et al. per cloud, and CrossEntropyLovasz, cross entropy + weight * Lovasz-Softmax on the same logits."""
import torch
import torch.nn as nn

from . import functional as F
from .functional.loss import _cross_entropy, _dml_pair_loss, _lovasz_softmax

__all__ = ['KLLoss', 'CrossEntropyLoss', 'DMLPairLoss', 'LovaszSoftmax', 'CrossEntropyLovasz']


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


class DMLPairLoss(nn.Module):
    """The criterion pair of a deep-mutual-learning step (reference: train_dml.py:125-137):
    forward(outputs, outputs_student, targets) -> (loss, loss_student) =
    (criterion(outputs, targets) + KLLoss()(outputs_student, outputs), criterion(outputs_student, targets) + KLLoss()(outputs, outputs_student)).

    `criterion`: an nn.CrossEntropyLoss or modules.CrossEntropyLoss (None: the default one); its weight, ignore_index, reduction
    and label_smoothing are taken over.  With reduction 'mean' and no smoothing, on device logits, the four terms are
    F.dml_pair_loss's two forward launches and one backward launch per network; the two losses are separate autograd nodes, so
    `loss.backward(); optimizer.step(); loss_student.backward()` and `(loss + loss_student).backward()` both work.  Anything else
    is composed of F.cross_entropy and F.kl_loss.

    `bad_targets`: as CrossEntropyLoss's -- created on the first call that runs a fused cross entropy, counted once per call."""

    def __init__(self, criterion=None):
        super().__init__()
        self.criterion = CrossEntropyLoss() if criterion is None else CrossEntropyLoss.from_torch(criterion)
        self.bad_targets = None

    def forward(self, outputs, outputs_student, targets):
        c = self.criterion
        fused = F.dml_pair_loss_is_fused(outputs, outputs_student, targets, c.weight, c.ignore_index, c.reduction, c.label_smoothing)
        counter = None
        if fused or F.cross_entropy_is_fused(outputs, targets, c.weight, c.reduction):
            if self.bad_targets is None or self.bad_targets.device != outputs.device:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError('DMLPairLoss: call the criterion once before capturing it (its bad_targets counter is '
                                       'created on the first call; GraphedTrainStep\'s warm-up steps do that)')
                self.bad_targets = torch.zeros((), dtype=torch.int64, device=outputs.device)
            counter = self.bad_targets
        return _dml_pair_loss(outputs, outputs_student, targets, c.weight, c.ignore_index, c.reduction, c.label_smoothing, counter, fused)


class LovaszSoftmax(nn.Module):
    """F.lovasz_softmax as a criterion: forward(input (B, C, N) logits, target (B, N)) -> loss.  On device tensors, one list per
    cloud of up to 16384 points, the loss and its gradient are four HIP launches; anything else is the torch composition.

    `bad_targets`: as CrossEntropyLoss's -- a 0-dim int64 tensor created on the first fused call, the running number of targets
    outside [0, C) that were not ignore_index (they are treated as ignored).  `count_bad_targets=False` keeps no counter (for a
    criterion that is added to one which counts the same targets already)."""

    def __init__(self, classes='present', per_cloud=True, ignore_index=-100, *, count_bad_targets=True):
        super().__init__()
        if classes not in ('present', 'all'):
            raise ValueError(f"LovaszSoftmax: classes must be 'present' or 'all', got {classes!r}")
        self.classes, self.per_cloud, self.ignore_index = classes, per_cloud, ignore_index
        self.count_bad_targets = count_bad_targets
        self.bad_targets = None

    def extra_repr(self):
        return f'classes={self.classes!r}, per_cloud={self.per_cloud}, ignore_index={self.ignore_index}'

    def forward(self, input, target):
        counter = None
        fused = F.lovasz_softmax_is_fused(input, target, self.per_cloud)
        if fused and self.count_bad_targets:
            if self.bad_targets is None or self.bad_targets.device != input.device:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError('LovaszSoftmax: call the criterion once before capturing it (its bad_targets counter is '
                                       'created on the first call; GraphedTrainStep\'s warm-up steps do that)')
                self.bad_targets = torch.zeros((), dtype=torch.int64, device=input.device)
            counter = self.bad_targets
        return _lovasz_softmax(input, target, self.classes, self.per_cloud, self.ignore_index, False, counter, fused)


class CrossEntropyLovasz(nn.Module):
    """The form people train segmentation with: CrossEntropyLoss(**cross-entropy arguments)(input, target) +
    lovasz_weight * LovaszSoftmax(classes, per_cloud, ignore_index)(input, target) on the same logits, composed of the two fused
    criteria (seven launches forward and backward on the device, capturable).  The cross-entropy arguments are nn.CrossEntropyLoss's
    (weight, ignore_index, reduction, label_smoothing); its ignore_index is the Lovasz term's too.

    `bad_targets`: the cross-entropy term's counter (both terms skip the same out-of-range targets; they are counted once)."""

    def __init__(self, lovasz_weight=1.0, classes='present', per_cloud=True, **cross_entropy_arguments):
        super().__init__()
        self.lovasz_weight = float(lovasz_weight)
        self.cross_entropy = CrossEntropyLoss(**cross_entropy_arguments)
        self.lovasz = LovaszSoftmax(classes, per_cloud, self.cross_entropy.ignore_index, count_bad_targets=False)

    @property
    def bad_targets(self):
        return self.cross_entropy.bad_targets

    def forward(self, input, target):
        return self.cross_entropy(input, target) + self.lovasz_weight * self.lovasz(input, target)
