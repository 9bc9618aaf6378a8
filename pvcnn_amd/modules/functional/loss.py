"""kl_loss / huber_loss (reference: modules/functional/loss.py:7-17) -- plain torch, tiny tensors -- and cross_entropy: the criterion
of the segmentation recipes (nn.CrossEntropyLoss on (B, classes, N) logits) on csrc/xent.hip, two launches forward and one
backward where torch takes five to six."""
import os

import torch
import torch.nn.functional as tf

__all__ = ['kl_loss', 'huber_loss', 'cross_entropy', 'cross_entropy_is_fused']

fused_enabled = os.environ.get('PVCNN_FUSED_XENT', '1') != '0'      # (debug / A-B switch: 0 = torch's cross_entropy everywhere)


def kl_loss(x, y):
    """KL(softmax(x).detach() || softmax(y)) averaged over all but the class dimension (dim 1)."""
    p = tf.softmax(x.detach(), dim=1)
    log_q = tf.log_softmax(y, dim=1)
    return (p * (p.log() - log_q)).sum(dim=1).mean()


def huber_loss(error, delta):
    """Mean Huber loss: 0.5*e^2 for |e| <= delta, delta*(|e| - 0.5*delta) beyond."""
    mag = error.abs()
    inner = mag.clamp(max=delta)
    return (0.5 * inner * inner + delta * (mag - inner)).mean()


_FLOATS = (torch.float32, torch.float16, torch.bfloat16)


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
