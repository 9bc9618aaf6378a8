"""huber_loss (reference: modules/functional/loss.py:13-17; plain torch, tiny tensors) and the criteria of the segmentation recipes
on the device: cross_entropy (nn.CrossEntropyLoss on (B, classes, N) logits) on csrc/xent.hip, two launches forward and one backward
where torch takes five to six; kl_loss (reference: modules/functional/loss.py:7-10) and dml_pair_loss, the four terms of a
deep-mutual-learning step, on csrc/dml.hip; lovasz_softmax, the IoU surrogate of Berman et al. (CVPR 2018) per cloud, on csrc/lovasz.hip."""
import os

import torch
import torch.nn.functional as tf

__all__ = ['kl_loss', 'kl_loss_is_fused', 'huber_loss', 'cross_entropy', 'cross_entropy_is_fused', 'dml_pair_loss',
           'dml_pair_loss_is_fused', 'lovasz_softmax', 'lovasz_softmax_is_fused', 'lovasz_softmax_parts']

fused_enabled = os.environ.get('PVCNN_FUSED_XENT', '1') != '0'      # (debug / A-B switch: 0 = torch's cross_entropy everywhere)
dml_enabled = os.environ.get('PVCNN_FUSED_DML', '1') != '0'         # (0 = kl_loss as torch ops, dml_pair_loss composed of its terms)
lovasz_enabled = os.environ.get('PVCNN_FUSED_LOVASZ', '1') != '0'   # (0 = lovasz_softmax as its torch composition everywhere)

_FLOATS = (torch.float32, torch.float16, torch.bfloat16)


def kl_loss_is_fused(x, y):
    """True when kl_loss(x, y) runs on the HIP kernels: two device tensors of the same shape (B, C, d1, ...), each fp32 / fp16 / bf16,
    on the same device, not empty.  Everything else is the torch formulation, unchanged."""
    if not dml_enabled:
        return False
    if not getattr(x, 'is_cuda', False) or not getattr(y, 'is_cuda', False):
        return False
    if x.dtype not in _FLOATS or y.dtype not in _FLOATS or x.dim() < 3:
        return False
    return x.shape == y.shape and x.device == y.device and x.numel() > 0


def kl_loss(x, y):
    """KL(softmax(x).detach() || softmax(y)) averaged over all but the class dimension (dim 1).  Where kl_loss_is_fused says so the
    loss and its gradient (for y; x is a constant) are three launches of csrc/dml.hip, without a host synchronisation (capturable);
    half / bf16 logits are evaluated in fp32 and give an fp32 loss.

    One deliberate difference on the fused path: the reference computes p * (log(p) - log_softmax(y)) with p = softmax(x) in fp32,
    which is 0 * log 0 = NaN as soon as one class of one point lies about 104 below the maximum.  The kernels form log p as
    (x_c - max x) - log(sum exp) and stay finite: such a class adds 0."""
    if not kl_loss_is_fused(x, y):
        p = tf.softmax(x.detach(), dim=1)
        log_q = tf.log_softmax(y, dim=1)
        return (p * (p.log() - log_q)).sum(dim=1).mean()
    a, b = x.detach().flatten(2), y.flatten(2)
    with torch.autocast(b.device.type, enabled=False):
        return _KLLoss.apply(b if b.dtype == torch.float32 else b.float(), a if a.dtype == torch.float32 else a.float())


def huber_loss(error, delta):
    """Mean Huber loss: 0.5*e^2 for |e| <= delta, delta*(|e| - 0.5*delta) beyond."""
    mag = error.abs()
    inner = mag.clamp(max=delta)
    return (0.5 * inner * inner + delta * (mag - inner)).mean()


def cross_entropy_is_fused(input, target, weight=None, reduction='mean'):
    """True when cross_entropy(input, target, weight, reduction=reduction) runs on the HIP kernels: device logits (B, C, d1, ...) in
    fp32 / fp16 / bf16 with int64 class-index targets (B, d1, ...) on the same device, an fp32 weight (C,) there or none, reduction
    mean or sum.  Everything else is torch's cross_entropy, unchanged."""
    if not fused_enabled:
        return False
    if not getattr(input, 'is_cuda', False) or not hasattr(target, 'dtype'):
        return False
    if input.dtype not in _FLOATS or input.dim() < 3 or reduction not in ('mean', 'sum'):
        return False
    if target.dtype != torch.int64 or target.device != input.device:
        return False
    if target.dim() != input.dim() - 1 or target.shape[0] != input.shape[0] or target.shape[1:] != input.shape[2:]:
        return False
    if input.numel() == 0:
        return False
    if weight is not None and not (getattr(weight, 'device', None) == input.device and weight.dtype == torch.float32
                                   and weight.dim() == 1 and weight.shape[0] == input.shape[1]):
        return False
    return True


_NATIVE = None


def _native():
    """(library, backend._run, backend.batch_strided_ok), looked up once: the criterion runs every step and, issued eagerly, is
    bound by the host."""
    global _NATIVE
    if _NATIVE is None:
        from ... import _lib
        from .backend import _run, batch_strided_ok
        _NATIVE = (_lib.load(), _run, batch_strided_ok)
    return _NATIVE


def _rows(t, ok):
    """t as it is when the kernels can walk it (rows of a sample contiguous, samples possibly further apart), else a packed copy."""
    return t if ok(t) else t.contiguous()


def _target_rows_ok(t):
    b, s = t.shape
    return (s == 1 or t.stride(1) == 1) and (b == 1 or t.stride(0) >= s)


class _CrossEntropy(torch.autograd.Function):
    """(logits (B, C, S) fp32, targets (B, S) int64, weight (C,) or None, ...) -> loss (0-dim).  Forward leaves (max, sum of exp) per
    point and the denominator in the workspace; backward reads them, the logits and the incoming gradient ON THE DEVICE and writes
    the whole gradient in one launch."""

    @staticmethod
    def forward(ctx, x, target, weight, ignore_index, mean, eps, bad_targets):
        lib, _run, batch_strided_ok = _native()
        x, target = _rows(x, batch_strided_ok), _rows(target, _target_rows_ok)
        if weight is not None and not weight.is_contiguous():
            weight = weight.contiguous()                 # the kernels read weight[c] packed: a strided / expanded view is copied (C floats)
        B, C, S = x.shape
        xbs = x.stride(0) if B > 1 else C * S
        tbs = target.stride(0) if B > 1 else S
        nbytes = lib.pvcnn_xent_workspace_bytes(B, S)          # (memoised per (B, S) by _lib.load)
        if nbytes == 0:
            raise RuntimeError(f'cross_entropy: {B} x {S} points are more than the kernels index')
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        _run(lib.pvcnn_xent_partials, 'xent_partials', x, x, xbs, target, tbs, weight, B, C, S, ignore_index, int(eps > 0.0), ws)
        _run(lib.pvcnn_xent_finalize, 'xent_finalize', x, weight, B, C, S, eps, mean, ws, loss, bad_targets)
        ctx.save_for_backward(x, target, weight, ws)
        ctx.args = (xbs, tbs, B, C, S, ignore_index, eps, mean)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        lib, _run, _ = _native()
        x, target, weight, ws = ctx.saved_tensors
        xbs, tbs, B, C, S, ignore_index, eps, mean = ctx.args
        if g.dtype != torch.float32:
            g = g.float()
        grad = torch.empty((B, C, S), dtype=torch.float32, device=x.device)
        _run(lib.pvcnn_xent_bwd, 'xent_bwd', x, x, xbs, target, tbs, weight, g, B, C, S, ignore_index, eps, mean, ws, grad)
        return grad, None, None, None, None, None, None


def cross_entropy(input, target, weight=None, ignore_index=-100, reduction='mean', label_smoothing=0.0, *, bad_targets=None):
    """torch.nn.functional.cross_entropy with the same arguments.  Where cross_entropy_is_fused says so the loss and its gradient come
    from csrc/xent.hip (no host synchronisation, no host-to-device copy: it can be captured into a hipGraph); every other call IS
    torch's, results and exceptions alike.

    One deliberate difference on the fused path: a target outside [0, C) that is not ignore_index is treated as ignored (torch's GPU
    kernel answers it with a device-side assert).  `bad_targets`, a 0-dim int64 tensor on the input's device, is incremented by the
    number of such targets of the call (do not share one counter between calls that run concurrently on different streams)."""
    return _cross_entropy(input, target, weight, ignore_index, reduction, label_smoothing, bad_targets,
                          cross_entropy_is_fused(input, target, weight, reduction))


def _cross_entropy(input, target, weight, ignore_index, reduction, label_smoothing, bad_targets, fused):
    """cross_entropy for a caller that has asked cross_entropy_is_fused already (modules.CrossEntropyLoss: once per call, not twice)."""
    eps = float(label_smoothing) if isinstance(label_smoothing, (int, float)) else -1.0
    if not (fused and 0.0 <= eps <= 1.0 and isinstance(ignore_index, int)):
        return tf.cross_entropy(input, target, weight=weight, ignore_index=ignore_index, reduction=reduction,
                                label_smoothing=label_smoothing)
    if bad_targets is not None and not (bad_targets.dtype == torch.int64 and bad_targets.dim() == 0 and bad_targets.device == input.device):
        raise ValueError("bad_targets must be a 0-dim int64 tensor on the input's device")
    x = input.flatten(2)
    if x.dtype != torch.float32:
        x = x.float()                                    # half / bf16 logits: the criterion is evaluated in fp32
    with torch.autocast(x.device.type, enabled=False):
        return _CrossEntropy.apply(x, target.flatten(1), weight, ignore_index, int(reduction == 'mean'), eps, bad_targets)


def _bstride(t, inner):
    return t.stride(0) if t.shape[0] > 1 else inner


class _KLLoss(torch.autograd.Function):
    """(y (B, C, S) fp32, x likewise and detached) -> kl_loss(x, y) (0-dim).  Forward leaves (max, sum of exp) of both tensors per
    point in the workspace; backward writes y's whole gradient in one launch."""

    @staticmethod
    def forward(ctx, y, x):
        lib, _run, batch_strided_ok = _native()
        x, y = _rows(x, batch_strided_ok), _rows(y, batch_strided_ok)
        B, C, S = y.shape
        xbs, ybs = _bstride(x, C * S), _bstride(y, C * S)
        nbytes = lib.pvcnn_kl_workspace_bytes(B, S)
        if nbytes == 0:
            raise RuntimeError(f'kl_loss: {B} x {S} points are more than the kernels index')
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=y.device)
        loss = torch.empty((), dtype=torch.float32, device=y.device)
        _run(lib.pvcnn_kl_partials, 'kl_partials', y, x, xbs, y, ybs, B, C, S, ws)
        _run(lib.pvcnn_kl_finalize, 'kl_finalize', y, B, C, S, ws, loss)
        ctx.save_for_backward(x, y, ws)
        ctx.args = (xbs, ybs, B, C, S)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        lib, _run, _ = _native()
        x, y, ws = ctx.saved_tensors
        xbs, ybs, B, C, S = ctx.args
        if g.dtype != torch.float32:
            g = g.float()
        grad = torch.empty((B, C, S), dtype=torch.float32, device=y.device)
        _run(lib.pvcnn_kl_bwd, 'kl_bwd', y, x, xbs, y, ybs, g, B, C, S, ws, grad)
        return grad, None


class _PairForward:
    """What the two nodes of one dml_pair_loss call share: the forward's two launches, run once, and what they leave behind."""

    def __init__(self, a, b, target, weight, ignore_index, bad_targets):
        lib, _run, batch_strided_ok = _native()
        a, b, target = _rows(a, batch_strided_ok), _rows(b, batch_strided_ok), _rows(target, _target_rows_ok)
        if weight is not None and not weight.is_contiguous():
            weight = weight.contiguous()
        B, C, S = a.shape
        self.args = (_bstride(a, C * S), _bstride(b, C * S), _bstride(target, S), B, C, S, ignore_index)
        nbytes = lib.pvcnn_dml_pair_workspace_bytes(B, S)
        if nbytes == 0:
            raise RuntimeError(f'dml_pair_loss: {B} x {S} points are more than the kernels index')
        self.tensors = (a, b, target, weight, torch.empty((nbytes,), dtype=torch.uint8, device=a.device))
        self.losses = torch.empty((2,), dtype=torch.float32, device=a.device)
        abs_, bbs, tbs = self.args[:3]
        _run(lib.pvcnn_dml_pair_partials, 'dml_pair_partials', a, a, abs_, b, bbs, target, tbs, weight, B, C, S, ignore_index,
             self.tensors[4])
        _run(lib.pvcnn_dml_pair_finalize, 'dml_pair_finalize', a, B, C, S, self.tensors[4], self.losses, bad_targets)


class _DmlPairSide(torch.autograd.Function):
    """(one network's logits (B, C, S) fp32, the call's _PairForward, side) -> that network's loss (0-dim): cross entropy against the
    targets + KL from the other network's (constant) distribution.  One node per network, so that each loss can be sent backward
    on its own, in either order, or both summed; backward is one launch that writes this network's whole gradient."""

    @staticmethod
    def forward(ctx, x, shared, side):
        ctx.save_for_backward(*shared.tensors)
        ctx.args = shared.args + (side,)
        return shared.losses[side]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        lib, _run, _ = _native()
        a, b, target, weight, ws = ctx.saved_tensors
        abs_, bbs, tbs, B, C, S, ignore_index, side = ctx.args
        if g.dtype != torch.float32:
            g = g.float()
        grad = torch.empty((B, C, S), dtype=torch.float32, device=a.device)
        _run(lib.pvcnn_dml_pair_bwd, 'dml_pair_bwd', a, a, abs_, b, bbs, target, tbs, weight, g, B, C, S, ignore_index, side, ws, grad)
        return grad, None, None


def dml_pair_loss_is_fused(outputs, outputs_student, targets, weight=None, ignore_index=-100, reduction='mean', label_smoothing=0.0):
    """True when dml_pair_loss with these arguments runs on the pair kernels of csrc/dml.hip: both logit tensors served by
    cross_entropy_is_fused with these targets and this weight, of the same shape, reduction 'mean', no label smoothing, an int
    ignore_index, and neither PVCNN_FUSED_DML nor PVCNN_FUSED_XENT at 0.  Everything else is composed of cross_entropy and kl_loss."""
    if not (fused_enabled and dml_enabled):
        return False
    if reduction != 'mean' or not isinstance(ignore_index, int):
        return False
    if not isinstance(label_smoothing, (int, float)) or label_smoothing != 0:
        return False
    if not (cross_entropy_is_fused(outputs, targets, weight, reduction) and cross_entropy_is_fused(outputs_student, targets, weight, reduction)):
        return False
    return outputs.shape == outputs_student.shape


def dml_pair_loss(outputs, outputs_student, targets, weight=None, ignore_index=-100, reduction='mean', label_smoothing=0.0, *,
                  bad_targets=None):
    """The two losses of a deep-mutual-learning step (reference: train_dml.py:125-137), (loss, loss_student) =
    (cross_entropy(outputs, targets, ...) + kl_loss(outputs_student, outputs),
     cross_entropy(outputs_student, targets, ...) + kl_loss(outputs, outputs_student)).

    Where dml_pair_loss_is_fused says so, all four terms come from one pass over both logit tensors (two launches, no host
    synchronisation: capturable) and the two results are two separate autograd nodes, one per network, each with a one-launch
    backward: `loss.backward()`, an optimizer step, then `loss_student.backward()` works, and so does
    `(loss + loss_student).backward()`.  Every other call is exactly the composition above, each function fused or not by its own
    predicate.

    On the fused path a target outside [0, C) that is not ignore_index is treated as ignored by the cross-entropy terms and counted
    in `bad_targets` (see cross_entropy; once per call -- the composition passes the counter to its first cross_entropy only); the KL
    terms take every point, as the reference's do.  When every point is ignored both losses are NaN, as torch's mean gives, and the
    gradients hold the KL part alone.  The KL terms stay finite where the reference's fp32 formula is NaN (see kl_loss)."""
    return _dml_pair_loss(outputs, outputs_student, targets, weight, ignore_index, reduction, label_smoothing, bad_targets,
                          dml_pair_loss_is_fused(outputs, outputs_student, targets, weight, ignore_index, reduction, label_smoothing))


def _dml_pair_loss(outputs, outputs_student, targets, weight, ignore_index, reduction, label_smoothing, bad_targets, fused):
    """dml_pair_loss for a caller that has asked dml_pair_loss_is_fused already (modules.DMLPairLoss)."""
    if not fused:
        return (cross_entropy(outputs, targets, weight, ignore_index, reduction, label_smoothing, bad_targets=bad_targets)
                + kl_loss(outputs_student, outputs),
                cross_entropy(outputs_student, targets, weight, ignore_index, reduction, label_smoothing)
                + kl_loss(outputs, outputs_student))
    if bad_targets is not None and not (bad_targets.dtype == torch.int64 and bad_targets.dim() == 0 and bad_targets.device == outputs.device):
        raise ValueError("bad_targets must be a 0-dim int64 tensor on the input's device")
    a, b = outputs.flatten(2), outputs_student.flatten(2)
    if a.dtype != torch.float32:
        a = a.float()                                    # half / bf16 logits: the criterion is evaluated in fp32
    if b.dtype != torch.float32:
        b = b.float()
    with torch.autocast(a.device.type, enabled=False):
        with torch.no_grad():
            shared = _PairForward(a.detach(), b.detach(), targets.flatten(1), weight, ignore_index, bad_targets)
        return _DmlPairSide.apply(a, shared, 0), _DmlPairSide.apply(b, shared, 1)


# ---- Lovasz-Softmax (Berman et al., CVPR 2018).  The definition is stated once, in include/pvcnn_hip.h; tests/lovasz_truth.py
# restates it in numpy.

_LOVASZ_CLASSES = ('present', 'all')


def _lovasz_workspace_bytes(b, c, s):
    """pvcnn_lovasz_workspace_bytes: 0 for what the kernels refuse (a list longer than 16384 points, sizes they do not index)."""
    return _native()[0].pvcnn_lovasz_workspace_bytes(b, c, s)


def lovasz_softmax_is_fused(input, target, per_cloud=True):
    """True when lovasz_softmax(input, target, per_cloud=per_cloud) runs on the HIP kernels: device logits or probabilities
    (B, C, d1, ...) in fp32 / fp16 / bf16 with int64 class-index targets (B, d1, ...) on the same device, one list per cloud
    (per_cloud, or a single cloud) of at most 16384 points, and PVCNN_FUSED_LOVASZ not 0.  Everything else is the torch composition of
    the same definition."""
    if not lovasz_enabled:
        return False
    if not getattr(input, 'is_cuda', False) or not hasattr(target, 'dtype'):
        return False
    if input.dtype not in _FLOATS or input.dim() < 3:
        return False
    if target.dtype != torch.int64 or target.device != input.device:
        return False
    if target.dim() != input.dim() - 1 or target.shape[0] != input.shape[0] or target.shape[1:] != input.shape[2:]:
        return False
    if input.numel() == 0 or not (per_cloud or input.shape[0] == 1):
        return False
    b, c = input.shape[:2]
    return _lovasz_workspace_bytes(b, c, input.numel() // (b * c)) != 0


def _lovasz_composition(p, target, classes_all, ignore_index):
    """The definition as batched torch ops on probabilities p (B, C, S) and targets (B, S): one stable descending sort on detached
    keys (dead points keyed below every error), gathers, one cumulative sum, the closed-form steps in fp64.  Returns the loss in
    fp64; differentiable for p (the order and the steps are constants)."""
    b, c, s = p.shape
    live = (target != ignore_index) & (target >= 0) & (target < c)
    fg = (target.unsqueeze(1) == torch.arange(c, device=p.device).view(1, c, 1)) & live.unsqueeze(1)
    e = torch.where(fg, 1.0 - p, p)
    keys = torch.where(live.unsqueeze(1), e.detach(), torch.full_like(e, float('-inf')))
    order = torch.sort(keys, dim=2, descending=True, stable=True).indices
    e_sorted, fg_sorted = torch.gather(e, 2, order), torch.gather(fg, 2, order)
    n, big_g = live.sum(1).view(b, 1, 1), fg.sum(2).unsqueeze(2)
    cf = torch.cumsum(fg_sorted, 2)
    i = torch.arange(1, s + 1, device=p.device).view(1, 1, s)
    inter, union = (big_g - cf).double(), (big_g + i - cf).double()
    # (union == 1 at a background element: a list without foreground, its first element -- the step is 1, not 0 / 0)
    background = torch.where(union == 1.0, torch.ones_like(union), inter / (union * (union - 1.0)).clamp_min(1.0))
    step = torch.where(fg_sorted, 1.0 / union, background)
    step = torch.where(i <= n, step, torch.zeros_like(step))
    per_class = (e_sorted.double() * step).sum(2)
    counted = (n.view(b, 1) > 0).expand(b, c) if classes_all else big_g.view(b, c) > 0
    k = counted.sum(1)
    cloud = torch.where(k > 0, (per_class * counted).sum(1) / k.clamp_min(1), torch.zeros_like(per_class[:, 0]))
    return cloud.mean()


def _lovasz_launches(x, target, ignore_index, classes_all, probas, bad_targets):
    """The forward launches on (B, C, S) fp32 / (B, S) int64: (loss, p, grad_p, workspace, p's batch stride).  p: the probabilities
    (x itself under probas); grad_p: d loss(b, c) / d p, the signed steps; the workspace holds the per-cloud scales 1 / (k_b B)."""
    lib, _run, batch_strided_ok = _native()
    x, target = _rows(x, batch_strided_ok), _rows(target, _target_rows_ok)
    B, C, S = x.shape
    nbytes = lib.pvcnn_lovasz_workspace_bytes(B, C, S)
    if nbytes == 0:
        raise RuntimeError(f'lovasz_softmax: {B} x {C} lists of {S} points are more than the kernels serve')
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    grad_p = torch.empty((B, C, S), dtype=torch.float32, device=x.device)
    if probas:
        p, pbs = x, _bstride(x, C * S)
    else:
        p, pbs = torch.empty((B, C, S), dtype=torch.float32, device=x.device), C * S
        _run(lib.pvcnn_lovasz_probs, 'lovasz_probs', x, x, _bstride(x, C * S), B, C, S, p)
    _run(lib.pvcnn_lovasz_sort, 'lovasz_sort', x, p, pbs, target, _bstride(target, S), B, C, S, ignore_index, classes_all, ws, grad_p)
    _run(lib.pvcnn_lovasz_finalize, 'lovasz_finalize', x, B, C, S, classes_all, ws, loss, bad_targets)
    return loss, p, grad_p, ws, pbs


class _LovaszSoftmax(torch.autograd.Function):
    """(logits or probabilities (B, C, S) fp32, targets (B, S) int64, ...) -> loss (0-dim).  Forward keeps the probabilities, the
    signed steps and the per-cloud scales; backward reads them and the incoming gradient ON THE DEVICE and writes the whole gradient
    in one launch."""

    @staticmethod
    def forward(ctx, x, target, ignore_index, classes_all, probas, bad_targets):
        loss, p, grad_p, ws, pbs = _lovasz_launches(x, target, ignore_index, classes_all, probas, bad_targets)
        ctx.save_for_backward(p, grad_p, ws)
        ctx.args = (pbs,) + tuple(x.shape) + (probas,)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        lib, _run, _ = _native()
        p, grad_p, ws = ctx.saved_tensors
        pbs, B, C, S, probas = ctx.args
        if g.dtype != torch.float32:
            g = g.float()
        grad = torch.empty((B, C, S), dtype=torch.float32, device=p.device)
        _run(lib.pvcnn_lovasz_bwd, 'lovasz_bwd', p, p, pbs, grad_p, g, B, C, S, probas, ws, grad)
        return grad, None, None, None, None, None


def _lovasz_arguments(input, target, classes, ignore_index, bad_targets, fused):
    if classes not in _LOVASZ_CLASSES:
        raise ValueError(f"lovasz_softmax: classes must be 'present' or 'all', got {classes!r}")
    if not isinstance(ignore_index, int):
        raise TypeError('lovasz_softmax: ignore_index must be an int')
    if input.dim() < 3 or target.dim() != input.dim() - 1 or target.shape[0] != input.shape[0] or target.shape[1:] != input.shape[2:]:
        raise ValueError(f'lovasz_softmax: input (B, C, d1, ...) and target (B, d1, ...) expected, got {tuple(input.shape)} and '
                         f'{tuple(target.shape)}')
    if fused and bad_targets is not None and not (bad_targets.dtype == torch.int64 and bad_targets.dim() == 0
                                                  and bad_targets.device == input.device):
        raise ValueError("bad_targets must be a 0-dim int64 tensor on the input's device")


def _composition_inputs(input, target, per_cloud, probas):
    """(probabilities (B', C, S'), targets (B', S')) of the composition: fp32 (fp64 stays fp64), per_cloud=False as ONE list."""
    x = input.flatten(2)
    if x.dtype != torch.float64:
        x = x.float()
    p = x if probas else tf.softmax(x, dim=1)
    t = target.flatten(1)
    if not per_cloud and p.shape[0] > 1:
        p, t = p.permute(1, 0, 2).reshape(1, p.shape[1], -1), t.reshape(1, -1)
    return p, t


def lovasz_softmax(input, target, *, classes='present', per_cloud=True, ignore_index=-100, probas=False, bad_targets=None):
    """The Lovasz-Softmax loss of Berman et al. (CVPR 2018), the surrogate of the mean IoU the meters report, on logits (or, with
    `probas`, probabilities) (B, C, d1, ...) and int64 targets (B, d1, ...).  Per cloud and class the points' errors are ranked and
    weighted by the steps of the Jaccard index along the ranking; `classes`: 'present' averages over the classes a cloud holds, 'all'
    over all C; `per_cloud` (Berman's per_image): the mean over the clouds' losses, False: the whole batch as one list.

    Where lovasz_softmax_is_fused says so the loss and its gradient come from csrc/lovasz.hip: three launches forward, one backward,
    no host synchronisation (capturable), the same bits for the same inputs; half / bf16 inputs are evaluated in fp32.  Everything
    else (CPU tensors, per_cloud=False over several clouds, lists beyond 16384 points) is a batched torch composition of the same
    definition, differentiable through autograd.

    A target outside [0, C) that is not ignore_index is treated as ignored; on the fused path `bad_targets`, a 0-dim int64 tensor on
    the input's device, is incremented by their number (see cross_entropy)."""
    return _lovasz_softmax(input, target, classes, per_cloud, ignore_index, probas, bad_targets,
                           lovasz_softmax_is_fused(input, target, per_cloud))


def _lovasz_softmax(input, target, classes, per_cloud, ignore_index, probas, bad_targets, fused):
    """lovasz_softmax for a caller that has asked lovasz_softmax_is_fused already (modules.LovaszSoftmax)."""
    _lovasz_arguments(input, target, classes, ignore_index, bad_targets, fused)
    if not fused:
        p, t = _composition_inputs(input, target, per_cloud, probas)
        return _lovasz_composition(p, t, classes == 'all', ignore_index).to(p.dtype)
    x = input.flatten(2)
    if x.dtype != torch.float32:
        x = x.float()                                    # half / bf16: the criterion is evaluated in fp32
    with torch.autocast(x.device.type, enabled=False):
        return _LovaszSoftmax.apply(x, target.flatten(1), ignore_index, int(classes == 'all'), int(bool(probas)), bad_targets)


def lovasz_softmax_parts(input, target, *, classes='present', per_cloud=True, ignore_index=-100, probas=False):
    """A diagnostic seam for the tests: (loss, probabilities, grad_probabilities) of lovasz_softmax with these arguments, detached.
    On the fused path these are the device tensors the autograd node keeps for backward -- the fp32 loss, the (B, C, S) probabilities
    the lists were ranked on, and d loss / d probabilities = the kept signed steps times the kept per-cloud scale 1 / (k_b B), the
    product backward forms.  On the composition path: its fp64 loss before the cast, its probabilities ((1, C, B S) for
    per_cloud=False) and autograd's gradient for them."""
    fused = lovasz_softmax_is_fused(input, target, per_cloud)
    _lovasz_arguments(input, target, classes, ignore_index, None, fused)
    if not fused:
        p, t = _composition_inputs(input.detach(), target, per_cloud, probas)
        p = p.detach().requires_grad_()
        loss = _lovasz_composition(p, t, classes == 'all', ignore_index)
        grad, = torch.autograd.grad(loss, p)
        return loss.detach(), p.detach(), grad
    x = input.detach().flatten(2)
    if x.dtype != torch.float32:
        x = x.float()
    with torch.no_grad(), torch.autocast(x.device.type, enabled=False):
        loss, p, steps, ws, _ = _lovasz_launches(x, target.flatten(1), ignore_index, int(classes == 'all'), int(bool(probas)), None)
        scale = ws[:4 * x.shape[0]].view(torch.float32)
        return loss, p, steps * scale.view(-1, 1, 1)
