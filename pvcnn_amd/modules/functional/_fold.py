"""Folded inference: an eval-mode BatchNorm is a constant per-channel affine map, so it belongs in the weights of the convolution in
front of it.  `folded_parameters` is the arithmetic; a `FoldSnapshot` is what `pvcnn_amd.fold_batchnorm` leaves on a convolution (a
plain attribute: no parameter, no buffer, nothing in state_dict) and what `functional.bnact.run_layers` runs instead of the three
modules [conv, BatchNorm, ReLU | LeakyReLU] -- one product whose epilogue applies the activation and emits the result's amax table
(csrc/gemm_epilogue.h: the activation tail).

A snapshot is never stale: it records the version counter and the address of its six source tensors (weight, bias, gamma, beta,
running mean, running variance) and the weight bank's epoch (FlatAdam writes parameters behind torch's back and says so through
`weight_bank_invalidate`, the rule the weight bank itself follows).  Any mismatch -- or a BatchNorm in training mode, or gradients
enabled -- and `snapshot_for` answers None: the caller runs the modules as they are, and the stale snapshot is dropped."""
import torch

ATTR = '_pvcnn_fold'


def folded_parameters(conv, bn):
    """(weight, bias) of the convolution that computes bn(conv(x)) in eval mode, formed in fp64 and rounded ONCE to fp32:
        w' = w * (gamma * rsqrt(var + eps)) per output channel,  b' = (b - mean) * gamma * rsqrt(var + eps) + beta
    (no conv bias: b = 0; a BatchNorm without affine parameters: gamma = 1, beta = 0)."""
    w = conv.weight.detach().double()
    co = w.shape[0]
    one, zero = torch.ones(co, dtype=torch.float64, device=w.device), torch.zeros(co, dtype=torch.float64, device=w.device)
    gamma = bn.weight.detach().double() if bn.weight is not None else one
    beta = bn.bias.detach().double() if bn.bias is not None else zero
    b = conv.bias.detach().double() if conv.bias is not None else zero
    scale = gamma * torch.rsqrt(bn.running_var.detach().double() + bn.eps)
    weight = (w * scale.view(-1, *([1] * (w.dim() - 1)))).float()
    bias = ((b - bn.running_mean.detach().double()) * scale + beta).float()
    return weight.contiguous(), bias.contiguous()


def _sources(conv, bn):
    return (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)


def _stamp(t):
    return None if t is None else (t._version, t.data_ptr(), tuple(t.shape))


def _bank_epoch():
    """The weight bank's epoch of the active backend (0 where there is no bank)."""
    from ._autograd import native
    be = native()
    return be._bank().epoch if getattr(be, 'has_weight_bank', False) else 0


class FoldSnapshot:
    """w', b' of one (conv, BatchNorm) pair, the state of the sources they were formed from, and the weight images of w' the kernels
    take (made once, on the first folded forward of each arithmetic mode: a folded forward launches no weight split after that)."""

    def __init__(self, conv, bn):
        self.weight, self.bias = folded_parameters(conv, bn)
        self.stamps = tuple(_stamp(t) for t in _sources(conv, bn))
        self.eps = bn.eps
        self.epoch = _bank_epoch()
        self.images = {}

    def valid(self, conv, bn):
        return (self.stamps == tuple(_stamp(t) for t in _sources(conv, bn)) and self.eps == bn.eps and self.epoch == _bank_epoch())

    def image(self, nsplit, make):
        """The forward weight image of w' for arithmetic `nsplit`, made by make(w') on first use."""
        if nsplit not in self.images:
            self.images[nsplit] = make(self.weight)
        return self.images[nsplit]


def snapshot_for(conv, bn):
    """THE predicate of the folded path, on the modules' side: the valid snapshot of (conv, bn), or None -- no snapshot, a stale one
    (dropped here), a BatchNorm that is not in eval mode with running statistics, or gradients enabled."""
    snap = getattr(conv, ATTR, None)
    if snap is None:
        return None
    if not snap.valid(conv, bn):
        delattr(conv, ATTR)
        return None
    if bn.training or bn.running_mean is None or bn.running_var is None or torch.is_grad_enabled():
        return None
    return snap


def attach(conv, bn):
    setattr(conv, ATTR, FoldSnapshot(conv, bn))


def detach(module):
    if ATTR in module.__dict__:
        delattr(module, ATTR)
