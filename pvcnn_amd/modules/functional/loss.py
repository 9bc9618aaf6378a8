"""huber_loss (reference: modules/functional/loss.py:13-17; plain torch, tiny tensors) and the criteria of the segmentation recipes
on the device: cross_entropy (nn.CrossEntropyLoss on (B, classes, N) logits) on csrc/xent.hip, two launches forward and one backward
where torch takes five to six; kl_loss (reference: modules/functional/loss.py:7-10) and dml_pair_loss, the four terms of a
deep-mutual-learning step, on csrc/dml.hip."""
import os

import torch
import torch.nn.functional as tf

__all__ = ['kl_loss', 'kl_loss_is_fused', 'huber_loss', 'cross_entropy', 'cross_entropy_is_fused', 'dml_pair_loss',
           'dml_pair_loss_is_fused']

fused_enabled = os.environ.get('PVCNN_FUSED_XENT', '1') != '0'      # (debug / A-B switch: 0 = torch's cross_entropy everywhere)
dml_enabled = os.environ.get('PVCNN_FUSED_DML', '1') != '0'         # (0 = kl_loss as torch ops, dml_pair_loss composed of its terms)

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
