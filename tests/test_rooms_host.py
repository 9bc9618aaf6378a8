"""Host side of the room preparation (no GPU): the fixture tests/golden/rooms.pt is self-consistent, the product path refuses CPU
tensors, and the new entry points are declared and bound."""
import os
import re

import pytest
import torch

from conftest import ROOT

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'rooms.pt')
ENTRY_POINTS = ['pvcnn_room_workspace_bytes', 'pvcnn_room_extent', 'pvcnn_room_blocks', 'pvcnn_room_cells', 'pvcnn_room_plan',
                'pvcnn_room_fill', 'pvcnn_room_pack']


@pytest.fixture(scope='module')
def golden():
    return torch.load(GOLDEN, weights_only=False)


def test_fixture_is_self_consistent(golden):
    assert os.path.getsize(GOLDEN) < 300 * 1024                  # the size class of the other goldens
    assert golden['A']['draw_free'] is True                      # the generator's two-seed equality of the resampled multisets
    assert golden['B']['num_seeds'] >= 8
    for room in golden.values():
        n, m = room['xyzrgb'].shape[0], room['options']['max_num_points']
        assert room['xyzrgb'].dtype == torch.float64 and room['xyzrgb'].shape == (n, 6) and room['labels'].shape == (n,)
        assert set(room['passes']) == {'zero', 'half'}
        assert room['passes']['zero']['offset'] == 0.0 and room['passes']['half']['offset'] == room['options']['block_size'] / 2
        for p in room['passes'].values():
            num, total = p['data_num'].long(), int(p['data_num'].sum())
            assert p['rows'].shape == (total, 9) and p['rows'].dtype == torch.float32
            assert p['label_seg'].shape == (total,) and p['indices'].shape == (total,) and p['window_block'].shape == num.shape
            assert int(p['indices'].min()) >= 0 and int(p['indices'].max()) < n
            assert torch.equal(p['label_seg'].long(), room['labels'][p['indices'].long()])
            # window sizes follow step 5 from the recorded block totals, blocks in block order
            sizes, blocks = [], []
            for b, t in p['block_total'].tolist():
                s = -(-t // m)
                avg = -(-t // s)
                sizes += [avg] * (s - 1) + [t - avg * (s - 1)]
                blocks += [b] * s
            assert num.tolist() == sizes and p['window_block'].tolist() == blocks
            assert blocks == sorted(blocks)
    a = golden['A']['passes']['zero']
    assert int(torch.bincount(a['window_block'].long()).max()) >= 3          # a block of three or more windows
    assert int(a['block_total'][:, 1].min()) < golden['A']['options']['max_num_points'] / 10   # a small block that stayed
    for p in golden['B']['passes'].values():
        member = p['point_block'].long()
        assert member.shape == (golden['B']['xyzrgb'].shape[0],) and float((member >= 0).float().mean()) > 0.9
        assert set(member[member >= 0].tolist()) <= set(p['block_total'][:, 0].tolist())


def test_prepare_room_refuses_cpu_tensors():
    from pvcnn_amd.rooms import prepare_room, segment_room
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        prepare_room(torch.zeros(8, 6, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        segment_room(torch.nn.Identity(), torch.zeros(8, 6, dtype=torch.float64))


def test_from_rooms_refuses_an_empty_list():
    """(rooms without labels are refused too: tests/test_gpu_rooms.py::test_from_rooms_equals_the_numpy_constructor)"""
    from pvcnn_amd.data import DeviceS3DIS
    with pytest.raises(ValueError):
        DeviceS3DIS.from_rooms([], 64)


def test_entry_points_are_declared_and_bound():
    from pvcnn_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'pvcnn_hip.h')).read()
    assert re.search(r'#define PVCNN_ABI_VERSION 17\b', header) and _lib.ABI_VERSION == 17
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r'PVCNN_API\s+\w+\s+' + name + r'\s*\(', header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert 'rooms.hip' in open(os.path.join(ROOT, 'pvcnn_amd', 'csrc', 'Makefile')).read()
    # the workspace query: two int arrays over the points, two over the blocks, the scan's tile sums
    assert lib.pvcnn_room_workspace_bytes(1000000, 400) >= (2 * 1000000 + 2 * 400) * 4
    assert lib.pvcnn_room_workspace_bytes(1, 0) >= 48
    assert lib.pvcnn_room_extent(None, 0, None, None, 0, None) != 0          # refused before anything is launched
    assert b'room' in lib.pvcnn_last_error_string()
