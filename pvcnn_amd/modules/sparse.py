"""SparseConv3d: the submanifold sparse 3x3x3 convolution as a layer (functional/sparse.py, csrc/sparse.hip)."""
import torch.nn as nn

from . import functional as F

__all__ = ['SparseConv3d']


class SparseConv3d(nn.Conv3d):
    """An nn.Conv3d with kernel 3, stride 1, padding 1 -- the same parameters and state_dict keys, so a dense checkpoint loads --
    whose forward runs on the rows of the active voxels: forward(rows (cap, Ci), map) -> (cap, Co), equal to the dense layer on the
    zero-filled grid, read at the active voxels."""

    def __init__(self, in_channels, out_channels, bias=True):
        super().__init__(in_channels, out_channels, 3, stride=1, padding=1, bias=bias)

    def forward(self, rows, map):
        return F.sparse_conv3d(rows, self.weight, self.bias, map)
