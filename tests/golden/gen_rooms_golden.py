#!/usr/bin/env python3
"""Generate tests/golden/rooms.pt from the REFERENCE's data/s3dis/prepare_data.py, run where the reference tree is mounted.

Producer of the expected values: the reference script itself, unmodified, executed with runpy.run_path(run_name='__main__') under
  * a stand-in `h5py` whose File.create_dataset keeps the arrays and an empty stand-in `plyfile` (neither is needed to compute);
  * `np.int = int` (an attribute of the running numpy that the script still spells the old way);
  * a wrapped np.random.shuffle that records (caller line, copy of the array, the caller's `offset_name`, `block_idx` and number of
    blocks) BEFORE shuffling: line 210 is a cell shuffle, line 229 receives a block's resampled index list, blocks in block order.
    Block numbers in the fixture are the script's own `block_idx`, read from its frame; nothing here recomputes the partition;
  * a temporary tree Area_1 .. Area_6 with one room (xyzrgb.npy, label.npy) and -m / -g / -b on sys.argv.
Nothing of pvcnn_amd takes part in producing the expected values.

Two rooms (see tests/test_gpu_rooms.py):
  A  draw-free: in every block each cell's count is at least the block's average or divides it, so every copy of the resampling
     survives and a block's resampled multiset depends on no draw.  PROVED here, not assumed: the reference runs under two seeds and
     the sorted line-229 lists must be equal block by block, else nothing is written.
  B  general: uniform fill, one dense slab, one sparse sliver; most cells draw.  Run under NUM_SEEDS seeds; stored per point: the
     block in whose line-229 list it appeared under any seed (-1: under none).
Stored per pass: the valid rows of the h5 arrays (`data` cast .astype(np.float32) as datasets/s3dis.py reads it, `label_seg`,
`indices_split_to_full`), `data_num`, and per window the block number; per block the resampled total.
Run:  python tests/golden/gen_rooms_golden.py [reference root]     (rewrites rooms.pt)
"""
import math
import os
import runpy
import sys
import tempfile
import time
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith('-') else '/root/reference'
SCRIPT = os.path.join(REF, 'data', 's3dis', 'prepare_data.py')
SEED = 1588147245
NUM_SEEDS = 8
CELL_SHUFFLE_LINE, BLOCK_SHUFFLE_LINE = 210, 229

H5 = {}                # basename -> {dataset name: array}


class _File:
    def __init__(self, name, mode='r'):
        self.sets = H5.setdefault(os.path.basename(name), {})

    def create_dataset(self, name, data=None):
        self.sets[name] = np.array(data)

    def close(self):
        pass


def run_reference(xyzrgb, labels, max_num_points, grid_size, block_size, seed):
    """-> ({'zero': h5 arrays, 'half': h5 arrays}, [(line, array before the shuffle, the caller's loop variables)], seconds)."""
    h5py, plyfile = types.ModuleType('h5py'), types.ModuleType('plyfile')
    h5py.File = _File
    saved_modules = {k: sys.modules.get(k) for k in ('h5py', 'plyfile')}
    sys.modules['h5py'], sys.modules['plyfile'] = h5py, plyfile
    had_int = hasattr(np, 'int')
    if not had_int:
        np.int = int
    real_shuffle, record = np.random.shuffle, []

    def shuffle(a):
        frame = sys._getframe(1)
        at = {k: frame.f_locals.get(k) for k in ('offset_name', 'block_idx')}          # the script's own loop variables
        at['num_blocks'] = frame.f_locals['blocks'].shape[0]
        record.append((frame.f_lineno, np.array(a, copy=True), at))
        real_shuffle(a)
    np.random.shuffle = shuffle
    saved_argv, saved_stdout = sys.argv, sys.stdout
    H5.clear()
    try:
        with tempfile.TemporaryDirectory() as tmp:
            raw, out = os.path.join(tmp, 'raw'), os.path.join(tmp, 'out')
            os.makedirs(raw)
            for area in range(1, 7):
                os.makedirs(os.path.join(out, f'Area_{area}'))
            room = os.path.join(out, 'Area_1', 'room_1')
            os.makedirs(room)
            np.save(os.path.join(room, 'xyzrgb.npy'), xyzrgb)
            np.save(os.path.join(room, 'label.npy'), labels.reshape(-1, 1).astype(np.float64))
            sys.argv = [SCRIPT, '-d', raw, '-f', out, '-m', str(max_num_points), '-g', repr(grid_size), '-b', repr(block_size)]
            sys.stdout = open(os.devnull, 'w')
            np.random.seed(seed)
            t0 = time.perf_counter()
            runpy.run_path(SCRIPT, run_name='__main__')
            seconds = time.perf_counter() - t0
    finally:
        sys.stdout.close() if sys.stdout is not saved_stdout else None
        sys.argv, sys.stdout = saved_argv, saved_stdout
        np.random.shuffle = real_shuffle
        if not had_int:
            del np.int
        for k, v in saved_modules.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    passes = {}
    for name in ('zero', 'half'):
        assert f'{name}_1.h5' not in H5, 'more than 2048 windows: shrink the room'
        passes[name] = {k: v.copy() for k, v in H5[f'{name}_0.h5'].items()}
    return passes, record, seconds


def block_lists(record, name=None):
    """The line-229 calls (of pass `name`), in call order: [(block_idx, list)], blocks in block order."""
    return [(at['block_idx'], a) for line, a, at in record if line == BLOCK_SHUFFLE_LINE and name in (None, at['offset_name'])]


def split_sizes(n, max_num_points):
    s = int(math.ceil(n * 1.0 / max_num_points))
    avg = int(math.ceil(n * 1.0 / s))
    return [avg] * (s - 1) + [n - avg * (s - 1)]


def pack_pass(h5, lists, max_num_points):
    """The stored form of one pass + the window -> block table from the recorded calls: a block's windows follow each other, their
    sizes follow step 5, and every index of a block's windows is in that block's list."""
    num = h5['data_num'].astype(np.int64)
    window_block, block_total, w = [], [], 0
    for block, lst in lists:
        sizes = split_sizes(len(lst), max_num_points)
        assert list(num[w:w + len(sizes)]) == sizes, 'window sizes do not follow the split rule'
        members = set(lst.tolist())
        for k in range(len(sizes)):
            assert set(h5['indices_split_to_full'][w + k, :num[w + k]].tolist()) <= members
        window_block += [block] * len(sizes)
        block_total.append((block, len(lst)))
        w += len(sizes)
    assert w == num.shape[0]
    valid = np.arange(h5['data'].shape[1])[None, :] < num[:, None]
    return {'data_num': torch.from_numpy(h5['data_num'].astype(np.int32)),
            'rows': torch.from_numpy(h5['data'].astype(np.float32)[valid]),
            'label_seg': torch.from_numpy(h5['label_seg'][valid].astype(np.int32)),
            'indices': torch.from_numpy(h5['indices_split_to_full'][valid].astype(np.int32)),
            'window_block': torch.tensor(window_block, dtype=torch.int32),
            'block_total': torch.tensor(block_total, dtype=torch.int64).reshape(-1, 2)}


def run_room(xyzrgb, labels, opts, seeds):
    runs = [run_reference(xyzrgb, labels, opts['max_num_points'], opts['grid_size'], opts['block_size'], s) for s in seeds]
    passes, record, _ = runs[0]
    room = {'xyzrgb': torch.from_numpy(xyzrgb), 'labels': torch.from_numpy(labels.astype(np.int64)), 'options': dict(opts),
            'cell_shuffles': sum(1 for line, _, _ in record if line == CELL_SHUFFLE_LINE), 'passes': {}}
    for name, offset in (('zero', 0.0), ('half', opts['block_size'] / 2)):
        room['passes'][name] = pack_pass(passes[name], block_lists(record, name), opts['max_num_points'])
        room['passes'][name]['offset'] = offset
        room['passes'][name]['num_blocks'] = next(at['num_blocks'] for line, _, at in record
                                                  if line == BLOCK_SHUFFLE_LINE and at['offset_name'] == name)
    return room, runs


# ------------------------------------------------------------------------------------------------------------------ room A
PATTERN = (1, 2, 4, 8, 8, 4, 2, 4)      # points per cell along z of one column: 33 points in 8 cells, average 4


def room_a(rng):
    """Columns of cells on a lattice of 0.25 (block 1.5 = 6 x 6 columns).  Every cell holds one point at its lattice corner (so a
    block's minimum is a lattice value and the cell index is exact) and the rest within 0.1 of it, on a 1/1024 raster."""
    g = 0.25
    cols = [(i, j, 8) for i in (0, 1) for j in (0, 1, 2)]               # a dense block (198 points) ...
    cols += [(i, j, 8) for i in (6, 7) for j in (0, 1, 2)]              # ... a second one beside it
    cols += [(12, 2, 2)]                                                # a sliver of two cells next to the second dense block
    cols += [(24, 1, 2)]                                                # two cells far from everything: small, no large neighbour
    pts = []
    for (i, j, cells) in cols:
        for k, c in enumerate(PATTERN[:cells]):
            corner = np.array([i * g + 0.125, j * g + 0.125, k * g + 0.125])
            jitter = rng.randint(0, 103, size=(c, 3)) / 1024.0
            jitter[0] = 0.0
            pts.append(corner + jitter)
    xyz = np.concatenate(pts) + np.array([3.0, -2.0, 0.5])              # the room does not start at the origin
    perm = rng.permutation(xyz.shape[0])
    xyz = xyz[perm]
    rgb = rng.randint(0, 256, size=xyz.shape).astype(np.float64)
    return np.concatenate([xyz, rgb], axis=1), rng.randint(0, 13, size=xyz.shape[0])


def room_b(rng):
    fill = rng.rand(900, 3) * [4.4, 2.9, 2.5]
    slab = rng.rand(250, 3) * [0.6, 0.5, 0.05] + [1.7, 1.1, 0.8]
    sliver = rng.rand(9, 3) * [0.1, 2.0, 2.0] + [4.52, 0.2, 0.1]
    xyz = np.concatenate([fill, slab, sliver]) + np.array([-1.25, 7.5, 0.1])
    xyz = xyz[rng.permutation(xyz.shape[0])]
    rgb = rng.randint(0, 256, size=xyz.shape).astype(np.float64)
    return np.concatenate([xyz, rgb], axis=1), rng.randint(0, 13, size=xyz.shape[0])


def timing(n_points):
    """The reference on a synthetic room of about n_points points at the default options, once (profiles/rooms_prepare.md)."""
    rng = np.random.RandomState(SEED)
    xyz = rng.rand(n_points, 3) * [6.0, 4.5, 3.0]
    xyzrgb = np.concatenate([xyz, rng.randint(0, 256, size=xyz.shape).astype(np.float64)], axis=1)
    labels = rng.randint(0, 13, size=n_points)
    passes, record, seconds = run_reference(xyzrgb, labels, 8192, 0.03, 1.5, SEED)
    print(f'reference prepare_data.py: {n_points} points, {seconds:.1f} s for both passes; windows '
          f'{passes["zero"]["data_num"].shape[0]} + {passes["half"]["data_num"].shape[0]}, entries '
          f'{int(passes["zero"]["data_num"].sum())} + {int(passes["half"]["data_num"].sum())}, '
          f'{sum(1 for l, _, _ in record if l == CELL_SHUFFLE_LINE)} cell shuffles; blocks (before the merge) '
          f'{[next(at["num_blocks"] for l, _, at in record if l == BLOCK_SHUFFLE_LINE and at["offset_name"] == n) for n in ("zero", "half")]}, '
          f'blocks after the merge {[len(block_lists(record, n)) for n in ("zero", "half")]}')


def main():
    if '--timing' in sys.argv:
        return timing(int(sys.argv[sys.argv.index('--timing') + 1]))
    rng = np.random.RandomState(SEED)
    golden = {}

    xyzrgb, labels = room_a(rng)
    opts = {'max_num_points': 100, 'grid_size': 0.25, 'block_size': 1.5}
    room, runs = run_room(xyzrgb, labels, opts, [SEED, SEED + 1])
    la, lb = block_lists(runs[0][1]), block_lists(runs[1][1])
    draw_free = len(la) == len(lb) and all(ba == bb and np.array_equal(np.sort(a), np.sort(b)) for (ba, a), (bb, b) in zip(la, lb))
    assert draw_free, 'room A is not draw-free: the resampled multisets of two seeds differ'
    zero = room['passes']['zero']
    assert zero['block_total'].shape[0] < zero['num_blocks'], 'room A needs a block that merges'
    assert int(torch.bincount(zero['window_block'].long()).max()) >= 3, 'room A needs a block of three or more windows'
    assert any(int(t) < opts['max_num_points'] / 10 for _, t in zero['block_total'].tolist()), 'room A needs a small block that stays'
    assert room['cell_shuffles'] > 0 and int(torch.bincount(room['passes']['half']['indices'].long()).min()) >= 1
    room['draw_free'] = bool(draw_free)
    golden['A'] = room

    xyzrgb, labels = room_b(rng)
    opts = {'max_num_points': 128, 'grid_size': 0.25, 'block_size': 1.5}
    seeds = [SEED + i for i in range(NUM_SEEDS)]
    room, runs = run_room(xyzrgb, labels, opts, seeds)
    for name in ('zero', 'half'):
        member = np.full(xyzrgb.shape[0], -1, dtype=np.int64)
        blocks = room['passes'][name]['block_total'][:, 0].tolist()
        for _, record, _ in runs:
            sub = block_lists(record, name)
            assert [b for b, _ in sub] == blocks        # the partition and the merge depend on no draw
            for block, lst in sub:
                assert np.all((member[lst] == -1) | (member[lst] == block))
                member[lst] = block
        room['passes'][name]['point_block'] = torch.from_numpy(member.astype(np.int32))
    room['num_seeds'] = NUM_SEEDS
    golden['B'] = room

    path = os.path.join(HERE, 'rooms.pt')
    torch.save(golden, path)
    for k, r in golden.items():
        print(k, r['xyzrgb'].shape[0], 'points;', {n: (int(p['data_num'].numel()), int(p['data_num'].sum())) for n, p in r['passes'].items()},
              r['cell_shuffles'], 'cell shuffles')
    print(f'wrote {path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
