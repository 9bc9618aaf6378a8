"""Sparse voxels: the submanifold sparse 3x3x3 convolution on the occupied voxels of a cloud (csrc/sparse.hip).

A dense Conv3d forms an output at every voxel of a grid of which a cloud occupies an eighth or less.  The convolution of SPVCNN is
defined on the ACTIVE voxels only (those that hold a point); the definition is in include/pvcnn_hip.h ("Sparse voxels") and restated
in torch fp64 by tests/sparse_conv_truth.py:

    sparse_map(cnt, resolution)         cnt (B, R^3) int32 (`VoxelPlan.cnt`, what voxelization already has) -> SparseMap
    sparse_gather(grid, map)            (B, C, R, R, R) -> rows (cap, C): a voxel's channels are contiguous
    sparse_conv3d(rows, w, bias, map)   rows (cap, Ci) -> (cap, Co), weight (Co, Ci, 3, 3, 3) as nn.Conv3d holds it
    sparse_scatter(rows, map)           rows (cap, C) -> (B, C, R, R, R), zero at the inactive voxels

The number of active voxels stays on the device (`map.count`, one int32 word): every launch is sized by the static capacity `cap`
and bounded by that word, rows >= count are zeros.  Nothing synchronises with the host, so the chain can be captured in a graph and
replayed on another occupancy.

Device tensors take the kernels (no switch, no fallback).  CPU tensors take a torch formulation of the same definition, stated once
as `sparse_conv3d_reference`: scatter to a dense grid, F.conv3d, gather.

Not here (the next step): BatchNorm / activation over the active rows and a composed sparse PVConv, strided and transposed sparse
convolutions, hashed maps for R > 128, the f16x2 / bf16x3 split arithmetic."""
import torch
import torch.nn.functional as TF
from torch.autograd import Function

from ._autograd import native, amp_fwd, amp_bwd

__all__ = ['SparseMap', 'sparse_map', 'sparse_gather', 'sparse_scatter', 'sparse_conv3d', 'sparse_conv3d_reference',
           'sparse_default_cap', 'SPARSE_ROW_TILE', 'SPARSE_MAX_R']

SPARSE_ROW_TILE = 64      # PVCNN_SPARSE_ROW_TILE: rows of a convolution tile
SPARSE_MAX_R = 128        # PVCNN_SPARSE_MAX_R


class SparseMap:
    """The active voxels of one (coordinates, R): voxel (cap,), index (B R^3,), offsets (B + 1,), nbr (cap, 27), overflow (1,), all
    int32 on one device (include/pvcnn_hip.h, "Sparse voxels").  `count` is the device word offsets[B]; `overflow` is 1 when `cap` was
    smaller than the number of active voxels (the map then keeps the first `cap`)."""

    def __init__(self, voxel, index, offsets, nbr, overflow, batch, resolution):
        self.voxel, self.index, self.offsets, self.nbr, self.overflow = voxel, index, offsets, nbr, overflow
        self.batch, self.resolution, self.cap = int(batch), int(resolution), int(voxel.shape[0])

    @property
    def count(self):
        return self.offsets[self.batch:]

    @property
    def device(self):
        return self.voxel.device

    def tensors(self):
        return self.voxel, self.index, self.offsets, self.nbr, self.overflow

    def __repr__(self):
        return f'SparseMap(batch={self.batch}, resolution={self.resolution}, cap={self.cap}, device={self.device})'


def sparse_default_cap(batch, resolution, num_points=None):
    """B min(N, R^3) rounded up to the row tile: no cloud of N points occupies more voxels."""
    per = int(resolution) ** 3 if num_points is None else min(int(num_points), int(resolution) ** 3)
    rows = max(int(batch) * per, 1)
    return (rows + SPARSE_ROW_TILE - 1) // SPARSE_ROW_TILE * SPARSE_ROW_TILE


def _check_sizes(batch, r, cap):
    if not (batch >= 1 and 1 <= r <= SPARSE_MAX_R and batch * r ** 3 < 2 ** 31 and 1 <= cap < 2 ** 31 // 27):
        raise RuntimeError('sparse_map: R <= 128, B R^3 < 2^31 and 1 <= cap < 2^31 / 27 expected')


def _map_torch(cnt, r, cap):
    """The map with tensor operations (any device): the CPU path, same tables as the kernels'."""
    b = cnt.shape[0]
    r3 = r ** 3
    dev = cnt.device
    active = torch.nonzero(cnt.reshape(-1) > 0).reshape(-1)                      # ascending
    total = active.numel()
    count = min(total, cap)
    kept = active[:count]
    voxel = torch.full((cap,), -1, dtype=torch.int64, device=dev)
    voxel[:count] = kept
    index = torch.full((b * r3,), -1, dtype=torch.int64, device=dev)
    index[kept] = torch.arange(count, device=dev)
    first = torch.searchsorted(active, torch.arange(b + 1, device=dev) * r3).clamp(max=cap)
    nbr = torch.full((cap, 27), -1, dtype=torch.int64, device=dev)
    z, y, x, cloud = kept % r, (kept // r) % r, (kept // (r * r)) % r, kept // r3
    for tap in range(27):
        nx, ny, nz = x + tap // 9 - 1, y + (tap // 3) % 3 - 1, z + tap % 3 - 1
        ok = (nx >= 0) & (nx < r) & (ny >= 0) & (ny < r) & (nz >= 0) & (nz < r)
        flat = ((cloud * r + nx.clamp(0, r - 1)) * r + ny.clamp(0, r - 1)) * r + nz.clamp(0, r - 1)
        nbr[:count, tap] = torch.where(ok, index[flat], torch.full_like(flat, -1))
    overflow = torch.tensor([1 if total > cap else 0], dtype=torch.int32, device=dev)
    i32 = torch.int32
    return voxel.to(i32), index.to(i32), first.to(i32), nbr.to(i32), overflow


def sparse_map(cnt, resolution, cap=None, num_points=None, out=None):
    """cnt (B, R^3) int32 -- points per voxel, `VoxelPlan.cnt` -- -> SparseMap.  `cap`: the static capacity in rows (default: B min(N,
    R^3) rounded up to the row tile, N = `num_points`, or R^3).  `out=`: the five tensors of a map, preallocated (device path)."""
    r = int(resolution)
    if cnt.dim() != 2 or cnt.shape[1] != r ** 3:
        raise RuntimeError(f'sparse_map: cnt (B, R^3) expected, got {tuple(cnt.shape)} at R = {r}')
    b = cnt.shape[0]
    cap = sparse_default_cap(b, r, num_points) if cap is None else int(cap)
    _check_sizes(b, r, cap)
    if cnt.is_cuda:
        tensors = native().sparse_map(cnt.int().contiguous(), r, cap, out=out)
    else:
        tensors = _map_torch(cnt, r, cap)
    return SparseMap(*tensors, b, r)


def _grid3(grid, m):
    if grid.dim() not in (3, 5) or grid.shape[0] != m.batch or grid[0, 0].numel() != m.resolution ** 3:
        raise RuntimeError(f'sparse_gather: a grid (B, C, R, R, R) of the map\'s B = {m.batch}, R = {m.resolution} expected')
    return grid.reshape(grid.shape[0], grid.shape[1], -1)


def _rows2(rows, m, who):
    if rows.dim() != 2 or rows.shape[0] != m.cap:
        raise RuntimeError(f'{who}: rows (cap = {m.cap}, C) expected, got {tuple(rows.shape)}')
    return rows


def _host_rows(m):
    count = int(m.count.item())
    v = m.voxel[:count].long()
    r3 = m.resolution ** 3
    return count, v // r3, v % r3


def _gather_torch(grid, m):
    count, cloud, cell = _host_rows(m)
    g = _grid3(grid, m)
    rows = g.new_zeros((m.cap, g.shape[1]))
    if count:
        rows = torch.cat([g[cloud, :, cell], rows[count:]], 0)
    return rows


def _scatter_torch(rows, m):
    count, cloud, cell = _host_rows(m)
    r = m.resolution
    g = rows.new_zeros((m.batch, r ** 3, rows.shape[1]))
    if count:
        g = g.index_put((cloud, cell), rows[:count])
    return g.permute(0, 2, 1).reshape(m.batch, rows.shape[1], r, r, r)


def sparse_conv3d_reference(rows, weight, bias, m):
    """THE formulation in torch (any device, any dtype, differentiable): rows scattered into a zero grid, F.conv3d(padding = 1), read at
    the active voxels; the bias only there."""
    _rows2(rows, m, 'sparse_conv3d')
    y = _gather_torch(TF.conv3d(_scatter_torch(rows, m), weight, None, padding=1), m)
    if bias is not None:
        live = (torch.arange(m.cap, device=rows.device) < m.count.to(rows.device)).to(y.dtype)
        y = y + live[:, None] * bias[None, :]
    return y


class SparseGather(Function):
    @staticmethod
    @amp_fwd
    def forward(ctx, grid, m):
        ctx.map, ctx.shape = m, grid.shape
        return native().sparse_gather(_grid3(grid, m).contiguous(), m.voxel, m.count)

    @staticmethod
    @amp_bwd
    def backward(ctx, grad_rows):
        m = ctx.map
        return native().sparse_scatter(grad_rows.contiguous(), m.index, m.count, m.batch, m.resolution).view(ctx.shape), None


class SparseScatter(Function):
    @staticmethod
    @amp_fwd
    def forward(ctx, rows, m):
        ctx.map = m
        r = m.resolution
        grid = native().sparse_scatter(_rows2(rows, m, 'sparse_scatter').contiguous(), m.index, m.count, m.batch, r)
        return grid.view(m.batch, rows.shape[1], r, r, r)

    @staticmethod
    @amp_bwd
    def backward(ctx, grad_grid):
        m = ctx.map
        return native().sparse_gather(_grid3(grad_grid, m).contiguous(), m.voxel, m.count), None


class SparseConv3dFunction(Function):
    @staticmethod
    @amp_fwd
    def forward(ctx, rows, weight, bias, m):
        be = native()
        rows = _rows2(rows, m, 'sparse_conv3d').contiguous()
        weight = weight.contiguous()
        ctx.map, ctx.has_bias = m, bias is not None
        ctx.save_for_backward(rows, weight)
        return be.sparse_conv3d_forward(rows, be.sparse_conv3d_weight_image(weight), bias.contiguous() if bias is not None else None,
                                        m.nbr, m.count)

    @staticmethod
    @amp_bwd
    def backward(ctx, grad_y):
        be, m = native(), ctx.map
        rows, weight = ctx.saved_tensors
        grad_y = grad_y.contiguous()
        grad_x = grad_w = grad_b = None
        if ctx.needs_input_grad[0]:
            grad_x = be.sparse_conv3d_forward(grad_y, be.sparse_conv3d_weight_image(weight, for_bwd_data=True), None, m.nbr, m.count)
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_b:
            grad_w, grad_b = be.sparse_conv3d_backward_weight(rows, grad_y, m.nbr, m.count, want_weight=ctx.needs_input_grad[1],
                                                              want_bias=want_b)
        return grad_x, grad_w, grad_b, None


def sparse_gather(grid, m):
    """grid (B, C, R, R, R) (or (B, C, R^3)) -> rows (cap, C), zeros at the rows >= count.  Its backward is sparse_scatter."""
    return SparseGather.apply(grid, m) if grid.is_cuda else _gather_torch(grid, m)


def sparse_scatter(rows, m):
    """rows (cap, C) -> (B, C, R, R, R), zero at every voxel without a row.  Its backward is sparse_gather."""
    return SparseScatter.apply(rows, m) if rows.is_cuda else _scatter_torch(_rows2(rows, m, 'sparse_scatter'), m)


def sparse_conv3d(rows, weight, bias, m):
    """y[j] = bias + sum_tap W[:, :, tap] x[nbr[j, tap]] at the rows j < count, zeros past them; = F.conv3d(padding = 1) of the
    zero-filled dense grid, read at the active voxels.  weight (Co, Ci, 3, 3, 3)."""
    if weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 3, 3) or rows.dim() != 2 or weight.shape[1] != rows.shape[1]:
        raise RuntimeError('sparse_conv3d: rows (cap, Ci) and weight (Co, Ci, 3, 3, 3) expected')
    if rows.is_cuda:
        return SparseConv3dFunction.apply(rows, weight, bias, m)
    return sparse_conv3d_reference(rows, weight, bias, m)
