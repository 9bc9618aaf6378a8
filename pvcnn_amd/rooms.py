"""S3DIS room preparation on the device: a raw scan -> windows, a `DeviceS3DIS` store, per-point labels (csrc/rooms.hip).

Reference: data/s3dis/prepare_data.py:119-282 -- numpy with one Python loop iteration per occupied grid cell of every block, written for
a numpy that still had `np.int`, and the only producer of `indices_split_to_full`, which the evaluation needs.  Here one pass (one block
offset) over a room is a fixed sequence of launches:

    extent -> block keys, counts, merge map -> per-block minimum, cell keys -> [sort by (block, cell)] -> cells, averages, output
    counts, prefix sums, window table -> resampling fill, shuffle keys -> [sort by (block, key)] -> per-block minima, packed rows

Every value the reference defines (block partition, merge, cell counts, averages, window sizes, the nine columns, labels, indices) is
computed by the kernels in the reference's fp64 arithmetic, one rounding per operation; the two orderings are torch.sort(stable=True).
What the reference leaves to `np.random.shuffle` (which avg of a cell's c * r copies survive; the order of a block's entries, hence
which window an entry lands in) is drawn from a Philox stream keyed by two int64 words from torch's generator: the same distributions,
other numbers than numpy's.  Same generator state, same output, bit for bit.

Host synchronisation: a pass makes exactly COPIES_PER_PASS = 2 device-to-host copies, each a few words, whatever the room's size:
the extent (6 fp64, to size the block table) and the status (cells, entries, windows, error bits, large cells: 5 int32, to size
the outputs).
Both go through `_read`, which counts them (`copies_made()`).

The product path needs device tensors (or numpy arrays, uploaded once) and the native library: there is no CPU implementation.
"""
import math

import numpy as np
import torch

from . import _lib
from .evaluate import SceneVotes, s3dis_file_votes
from .modules.functional.backend import _device_call as _call, fresh_seed

__all__ = ['RoomWindows', 'prepare_room', 'segment_room', 'copies_made', 'COPIES_PER_PASS']

COPIES_PER_PASS = 2
MAX_BLOCKS = 1 << 24
_copies = 0


def copies_made():
    """Device-to-host copies this module has made so far (every one goes through `_read`)."""
    return _copies


def _read(t):
    """The one place a pass reads device memory on the host."""
    global _copies
    _copies += 1
    return t.cpu().tolist()


def _device_points(xyzrgb):
    """(N, 6) float64 on the device: a device tensor as it is (float32 is widened), a numpy array uploaded once."""
    if isinstance(xyzrgb, torch.Tensor):
        if xyzrgb.device.type != 'cuda':
            raise RuntimeError('room preparation needs a CUDA (HIP) tensor or a numpy array -- there is no CPU implementation')
        x = xyzrgb
    else:
        if not torch.cuda.is_available():
            raise RuntimeError('room preparation needs a GPU and the native library -- there is no CPU implementation')
        x = torch.from_numpy(np.ascontiguousarray(xyzrgb)).to(torch.device('cuda', torch.cuda.current_device()))
    if x.dim() != 2 or x.shape[1] != 6 or x.shape[0] < 1:
        raise ValueError(f'xyzrgb (N, 6) with N >= 1 expected, got {tuple(x.shape)}')
    if x.dtype not in (torch.float64, torch.float32):
        raise ValueError('xyzrgb must be float64 or float32')
    return x.to(torch.float64).contiguous()


def _device_labels(labels, n, device):
    if labels is None:
        return None
    if isinstance(labels, torch.Tensor):
        if labels.device.type != 'cuda':
            raise RuntimeError('room preparation needs CUDA (HIP) tensors or numpy arrays -- there is no CPU implementation')
        lab = labels.to(device)
    else:
        lab = torch.from_numpy(np.ascontiguousarray(np.asarray(labels).reshape(-1).astype(np.int64))).to(device)
    lab = lab.reshape(-1)
    if lab.numel() != n:
        raise ValueError(f'{n} labels expected, got {lab.numel()}')
    return lab.to(torch.int32).contiguous()


class RoomWindows:
    """The windows of one pass over one room, packed like `data._Store`: window w owns rows offsets[w] .. offsets[w + 1].
    rows (R, 9) fp32, labels (R,) int32 or None, indices (R,) int32 (`indices_split_to_full`), offsets (W + 1,) int64,
    window_block (W,) int32 (the reference's block number)."""

    def __init__(self, rows, labels, indices, offsets, window_block, num_room_points, max_num_points, num_cells=None):
        self.num_cells = num_cells                     # occupied grid cells over all merged blocks (None if not known)
        self.rows, self.labels, self.indices, self.offsets, self.window_block = rows, labels, indices, offsets, window_block
        self.num_room_points, self.max_num_points = int(num_room_points), int(max_num_points)
        self.device = rows.device

    def __len__(self):
        return self.offsets.numel() - 1

    @property
    def data_num(self):
        """(W,) int32: the h5 file's `data_num`."""
        return (self.offsets[1:] - self.offsets[:-1]).to(torch.int32)

    def padded(self):
        """The reference's h5 layout on the device: (data (W, max_num_points, 9) fp32, data_num (W,) int32, label_seg (W, max_num_points)
        int32, indices_split_to_full (W, max_num_points) int32), zeros beyond data_num (the reference leaves stale rows of earlier
        windows there; nobody reads them)."""
        w, m, r = len(self), self.max_num_points, self.rows.shape[0]
        num = self.offsets[1:] - self.offsets[:-1]
        window = torch.repeat_interleave(torch.arange(w, device=self.device), num, output_size=r)
        slot = window * m + (torch.arange(r, device=self.device) - self.offsets[:-1][window])
        data = torch.zeros((w * m, 9), dtype=torch.float32, device=self.device)
        data[slot] = self.rows
        label_seg = torch.zeros((w * m,), dtype=torch.int32, device=self.device)
        if self.labels is not None:
            label_seg[slot] = self.labels
        indices = torch.zeros((w * m,), dtype=torch.int32, device=self.device)
        indices[slot] = self.indices
        return data.view(w, m, 9), num.to(torch.int32), label_seg.view(w, m), indices.view(w, m)


def prepare_room(xyzrgb, labels=None, *, max_num_points=8192, block_size=1.5, grid_size=0.03, offset=0.0, generator=None):
    """One pass of prepare_data.py over one room.  xyzrgb (N, 6): coordinates and colours 0..255, float64 (float32 is widened; parity with
    the reference is claimed for float64 input), finite; labels (N,) integers or None.  offset: 0.0 for the reference's `zero` pass,
    block_size / 2 for `half`.  generator: a torch.Generator (device or CPU) for the two Philox words, default torch's device generator.
    -> RoomWindows."""
    x = _device_points(xyzrgb)
    dev, n = x.device, x.shape[0]
    lab = _device_labels(labels, n, dev)
    max_num_points, block_size, grid_size, offset = int(max_num_points), float(block_size), float(grid_size), float(offset)
    if max_num_points < 1 or not block_size > 0 or not grid_size > 0 or offset < 0:
        raise ValueError('max_num_points >= 1, block_size > 0, grid_size > 0 and offset >= 0 expected')
    lib = _lib.load()
    i32 = dict(dtype=torch.int32, device=dev)
    i64 = dict(dtype=torch.int64, device=dev)

    # step 1: the extent, and from it the size of the dense block table (the expressions of the block-key kernel)
    ws = torch.empty((max(lib.pvcnn_room_workspace_bytes(n, 0), 16),), dtype=torch.uint8, device=dev)
    extent = torch.empty((6,), dtype=torch.float64, device=dev)
    _call('room_extent', x, x, n, extent, ws, ws.numel())
    ext = _read(extent)
    if not all(math.isfinite(v) for v in ext):
        raise ValueError('xyzrgb holds a coordinate that is not finite')
    gx = int(math.floor(((ext[3] - ext[0]) - (0.0 - offset)) / block_size)) + 1
    gy = int(math.floor(((ext[4] - ext[1]) - (0.0 - offset)) / block_size)) + 1
    g = gx * gy
    if g > MAX_BLOCKS:
        raise ValueError(f'{gx} x {gy} blocks: the block table holds at most 2^24')

    # steps 2-4a: block keys, counts, merge map, per-block minimum, cell keys
    ws = torch.empty((max(lib.pvcnn_room_workspace_bytes(n, g), 16),), dtype=torch.uint8, device=dev)
    point_block = torch.empty((n,), **i32)
    block_count, block_target, block_rank = (torch.empty((g,), **i32) for _ in range(3))
    status = torch.empty((5,), **i32)
    _call('room_blocks', x, x, n, extent, offset, block_size, gx, gy, max_num_points, point_block, block_count, block_target, block_rank,
          status, ws, ws.numel())
    block_min = torch.empty((g, 3), **i64)
    cell_key = torch.empty((n,), **i64)
    _call('room_cells', x, x, n, extent, grid_size, g, block_target, point_block, block_min, cell_key, status)

    # order the points by (merged block, cell key): two stable sorts
    sorted_key, by_key = torch.sort(cell_key, stable=True)
    sorted_block, by_block = torch.sort(point_block[by_key], stable=True)
    perm = by_key[by_block].to(torch.int32)
    sorted_key = sorted_key[by_block].contiguous()

    # steps 4b, 5: cells, averages, output counts, prefix sums, window table
    point_cell, cell_out, cell_out_start = (torch.empty((n,), **i32) for _ in range(3))
    cell_start = torch.empty((n + 1,), **i32)
    block_tables = torch.empty((5, g), **i32)
    _call('room_plan', x, sorted_block, sorted_key, n, g, max_num_points, point_cell, cell_start, cell_out, cell_out_start, block_tables,
          status, ws, ws.numel())
    num_cells, num_entries, num_windows, error, _ = _read(status)
    if error & 1:
        raise RuntimeError('a point fell outside the block table (non-finite coordinates?)')
    if error & 2:
        raise ValueError('a merged block spans more than 2^21 cells along one axis: grid_size is too small for this room')

    # step 4c: the resampling fill and the block shuffle's keys
    seed = fresh_seed(dev, generator)
    entry_point, entry_block = torch.empty((num_entries,), **i32), torch.empty((num_entries,), **i32)
    entry_key = torch.empty((num_entries,), **i64)
    _call('room_fill', x, perm, sorted_block, point_cell, cell_start, cell_out_start, block_tables, status, n, g, num_entries, seed,
          entry_point, entry_block, entry_key)

    # order the entries by (block, key): the entries are block-contiguous already, so the second sort only restores that
    _, by_key = torch.sort(entry_key, stable=True)
    _, by_block = torch.sort(entry_block[by_key], stable=True)
    entry_point = entry_point[by_key[by_block]].contiguous()

    # step 6: per-block minima over the resampled entries, rows, labels, indices, the window table
    rows = torch.empty((num_entries, 9), dtype=torch.float32, device=dev)
    labels_out = torch.empty((num_entries,), **i32) if lab is not None else None
    indices = torch.empty((num_entries,), **i32)
    offsets = torch.empty((num_windows + 1,), **i64)
    window_block = torch.empty((num_windows,), **i32)
    block_minxy = torch.empty((g, 2), **i64)
    _call('room_pack', x, x, lab, n, extent, block_size / 2, entry_point, entry_block, num_entries, g, max_num_points, num_windows,
          block_tables, block_rank, block_minxy, rows, labels_out, indices, offsets, window_block)
    return RoomWindows(rows, labels_out, indices, offsets, window_block, n, max_num_points, num_cells)


def segment_room(model, xyzrgb, *, num_points=4096, num_votes=1, batch_size=10, rng=np.random, generator=None, **prepare_options):
    """Per-point labels of a raw scan: the `zero` and `half` passes of `prepare_room`, then the reference's evaluation loop
    (`s3dis_file_votes`) over each, merged in one `SceneVotes`.  -> (predictions (N,) int64 on the device, the SceneVotes).  A point no
    window covers keeps prediction -1.  prepare_options: max_num_points, block_size, grid_size."""
    unknown = set(prepare_options) - {'max_num_points', 'block_size', 'grid_size'}
    if unknown:
        raise TypeError(f'unexpected options {sorted(unknown)}')
    x = _device_points(xyzrgb)
    votes = SceneVotes(x.shape[0], x.device)
    half = float(prepare_options.get('block_size', 1.5)) / 2
    for offset in (0.0, half):
        windows = prepare_room(x, None, offset=offset, generator=generator, **prepare_options)
        data, data_num, _, indices = windows.padded()
        s3dis_file_votes(model, data, data_num, indices, votes, num_points=num_points, num_votes=num_votes, batch_size=batch_size, rng=rng)
    return votes.predictions(), votes
