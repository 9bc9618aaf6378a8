"""pointwise_conv: the kernel-size-1 Conv1d / Conv2d of SharedMLP (reference: modules/shared_mlp.py:9-25).

The reference calls nn.Conv1d / nn.Conv2d (cuDNN / cuBLAS).  On gfx950 the three GEMMs (forward, backward-data,
backward-weight + bias gradient) run directly on the channel-major (B, C, N) tensors in "f16x2" arithmetic on the fp16 matrix
cores (csrc/pointwise_bf16.hip, pointwise_wgrad_f16.hip: fp32 tensors, operands split into scaled fp16 hi + lo, fp32 accumulation)
-- forward / backward-data from `backend.pw_split_min_macs` (16.8 M) multiply-adds up, backward-weight from
`backend.pw_wgrad_f16_min_macs` (4.3 G) -- and on the fp32-MFMA kernels of csrc/pointwise.hip below those bars.

The node's body is shared with the voxel Conv3d: functional/_product.py (`PW` is this kind's descriptor: the (B, C, N) / (Co, Ci)
views, the 256-point amax tiles and the backward-weight bar)."""
import torch
from torch.autograd import Function

from . import _product
from ._autograd import native, amp_fwd, amp_bwd

__all__ = ['pointwise_conv', 'pw_nsplit']


def pw_nsplit(x, weight):
    """Arithmetic of one 1x1 convolution's forward / backward-data products, decided where it is CALLED (inside the autograd node
    autocast is already switched off): 2 = f16x2 / 3 = bf16x3 (fp32-class, csrc/pointwise_bf16.hip; `backend.pw_math`), 1 = plain bf16
    operands under torch.autocast(bfloat16), 0 = the fp32-MFMA kernels of csrc/pointwise.hip -- always for GEMMs below
    `backend.pw_split_min_macs` multiply-adds: they are launch-bound, and the split kernels' extra launches cost more than they save."""
    be = native()
    if not getattr(be, 'has_pwconv_split', False):
        return 0
    macs = weight.shape[0] * weight.shape[1] * x.shape[0] * (x.numel() // max(x.shape[0] * x.shape[1], 1))
    if macs < getattr(be, 'pw_split_min_macs', 0):
        return 0
    if torch.is_autocast_enabled() and torch.get_autocast_dtype('cuda') == torch.bfloat16:
        return 1
    return getattr(be, 'PW_NSPLIT', {}).get(getattr(be, 'pw_math', 'fp32'), 0)


class PointwiseConv(Function):
    @staticmethod
    @amp_fwd
    def forward(ctx, x, weight, bias, want_stats=False, split=None):
        # the split products on the 16-bit matrix cores (csrc/pointwise_bf16.hip): 2 = f16x2, 3 = bf16x3, 1 = bf16, 0 = fp32 MFMA
        nsplit = split if split is not None else pw_nsplit(x, weight)
        return _product.forward(_product.PW, native(), ctx, x, weight, bias, want_stats, nsplit)

    @staticmethod
    @amp_bwd
    def backward(ctx, grad_y, grad_part=None):
        return _product.backward(_product.PW, native(), ctx, grad_y)


pointwise_conv = PointwiseConv.apply
