"""The KITTI frame stage on the host: tests/frames_truth.py (the numpy definition the kernels are held to) against closed forms, the
host scalars of pvcnn_amd.frames against the truth, the calib reader, the ABI additions.  No GPU: no kernel is launched here."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import frames_truth as ft
from pvcnn_amd import frames

F, CU, CV = 512.0, 620.0, 187.5
P = np.array([[F, 0, CU, 0], [0, F, CV, 0], [0, 0, 1, 0]], dtype=np.float64)
R0 = np.eye(3)
V2C = np.hstack([np.eye(3), np.zeros((3, 1))])
SIZE = (1242, 375)


def _lattice():
    """Dyadic points (x, y, z) with x > 2 and z a power of two: f * x / z is exact in fp64."""
    xs = np.arange(17) * 0.25 + 2.25
    ys = np.arange(-4, 5) * 0.125
    zs = np.array([1.0, 2.0, 4.0, 8.0, 16.0])
    g = np.stack(np.meshgrid(xs, ys, zs, indexing='ij'), axis=-1).reshape(-1, 3)
    return np.concatenate([g, np.full((len(g), 1), 0.5)], axis=1).astype(np.float32)


def test_projection_is_the_closed_form_on_a_dyadic_lattice():
    scan = _lattice()
    rows, uv, in_image = ft.project(scan, P, R0, V2C, SIZE)
    x, y, z = (scan[:, c].astype(np.float64) for c in range(3))
    assert np.array_equal(uv[:, 0], F * x / z + CU) and np.array_equal(uv[:, 1], F * y / z + CV)
    assert np.array_equal(rows, scan)                                   # identity extrinsics: the stored row is the scan row
    want = (uv[:, 0] >= 0) & (uv[:, 0] < 1242) & (uv[:, 1] >= 0) & (uv[:, 1] < 375)
    assert np.array_equal(in_image, want) and in_image.any() and not in_image.all()


def test_box_edges_clip_distance_and_zero_depth():
    # u = 512 x / z + 620, v = 512 y / z + 187.5 at z = 4: x = 2.5 -> u = 940, y = 0.25 -> v = 219.5
    scan = np.array([[2.5, 0.25, 4.0, 0], [2.5, 0.25, 4.0, 0], [2.0, 0.25, 4.0, 0], [3.0, 0.25, 0.0, 0], [3.0, 0.0, 0.0, 0],
                     [np.nan, 0.25, 4.0, 0]], dtype=np.float32)
    with np.errstate(all='raise'):                                      # nothing may raise, whatever numpy is told to do
        try:
            rows, uv, in_image = ft.project(scan, P, R0, V2C, SIZE)
        except FloatingPointError as e:                                 # pragma: no cover
            pytest.fail(f'the truth raised {e!r}')
    assert (uv[0, 0], uv[0, 1]) == (940.0, 219.5)
    assert in_image.tolist() == [True, True, False, False, False, False]    # x_velo == 2.0, img_2 == 0 (inf and nan), a NaN coordinate
    on_min = ft.in_box(uv, in_image, (940.0, 219.5, 1000.0, 300.0))
    on_max = ft.in_box(uv, in_image, (900.0, 200.0, 940.0, 300.0))
    on_vmax = ft.in_box(uv, in_image, (900.0, 200.0, 1000.0, 219.5))
    assert on_min[0] and not on_max[0] and not on_vmax[0]
    assert ft.in_box(uv, in_image, (900.0, 219.5, 1000.0, 220.0))[0]
    assert not ft.in_box(uv, in_image, (0.0, 0.0, 1242.0, 375.0))[2:].any()


def test_frustum_angle_of_a_centred_box_and_its_rotation():
    box = (CU - 50.0, 100.0, CU + 50.0, 200.0)
    assert ft.frustum_angle(P, box) == -np.pi / 2
    calib = frames.Calibration(P, R0, V2C)
    assert np.array_equal(frames.frustum_angle(calib, [box]), [-np.pi / 2])
    rotation = np.pi / 2.0 + ft.frustum_angle(P, box)
    assert rotation == 0.0
    rows = _lattice()
    assert np.array_equal(ft.rotate_rows(rows, rotation), rows)
    table = frames.box_table(calib, [box], [2], [0.75])
    assert table.shape == (1, frames.BOX_COLUMNS) and table[0, 13:18].tolist() == [1.0, 0.0, 0.0, 2.0, 0.75] and table[0, 4] == 0
    off = (100.0, 100.0, 300.0, 200.0)                                  # off-centre: the host scalars are the truth's
    assert frames.frustum_angle(calib, [box, off])[1] == ft.frustum_angle(P, off)
    quarter = ft.rotate_rows(np.array([[1, 5, 0, 9], [0, 5, 1, 9]], dtype=np.float32), np.pi / 2)
    assert np.allclose(quarter, [[0, 5, 1, 9], [-1, 5, 0, 9]], atol=1e-7) and np.array_equal(quarter[:, [1, 3]], [[5, 9], [5, 9]])


@pytest.mark.parametrize('ry', [0.0, np.pi / 2])
def test_label_is_the_axis_aligned_test_faces_included(ry):
    # Half extents 2 and 3 lie in one binade [2, 4), where half an ulp is 2.2e-16.  sin(pi / 2) is 1.0 exactly and fp64's cos(pi / 2)
    # is 6.1e-17, so a point on a face gets a cross term of at most 6.1e-17 * 3.25 = 2.0e-16 < half an ulp: it rounds back onto the
    # face or just inside it.  The quarter turn is therefore the axis-aligned test with the extents swapped, faces included, exactly.
    h, w, l, t = 1.5, 6.0, 4.0, np.array([1.0, 1.0, 10.0])
    ax = np.arange(-13, 14) * 0.25
    g = np.stack(np.meshgrid(ax, np.arange(-8, 3) * 0.25, ax, indexing='ij'), axis=-1).reshape(-1, 3)
    rows = np.concatenate([g + t, np.zeros((len(g), 1))], axis=1).astype(np.float32)
    got = ft.in_box_3d(rows, (h, w, l, *t, ry))
    if ry == 0.0:
        want = (np.abs(g[:, 0]) <= l / 2) & (np.abs(g[:, 2]) <= w / 2)
    else:
        want = (np.abs(g[:, 0]) <= w / 2) & (np.abs(g[:, 2]) <= l / 2)
    want &= (g[:, 1] <= 0) & (g[:, 1] >= -h)
    assert np.array_equal(got, want) and want.sum() == (17 * 25 * 7 if ry == 0.0 else 25 * 17 * 7)
    if ry == 0.0:       # one point in the middle of each of the six faces, and just beyond it
        faces = np.array([[l / 2, -0.5, 0], [-l / 2, -0.5, 0], [0, 0, 0], [0, -h, 0], [0, -0.5, w / 2], [0, -0.5, -w / 2]])
        beyond = faces + np.array([[.25, 0, 0], [-.25, 0, 0], [0, .25, 0], [0, -.25, 0], [0, 0, .25], [0, 0, -.25]])
        both = np.concatenate([np.concatenate([faces, beyond]) + t, np.zeros((12, 1))], axis=1).astype(np.float32)
        assert ft.in_box_3d(both, (h, w, l, *t, ry)).tolist() == [True] * 6 + [False] * 6


@pytest.mark.parametrize('ry', [0.0, np.pi / 2, 0.3, -2.1])
def test_corners_zero_and_six_average_to_the_centre(ry):
    box = (1.5, 1.75, 4.0, 1.0, 1.5, 10.0, ry)
    c = ft.corners(box)
    assert np.allclose((c[0] + c[6]) / 2, [1.0, 1.5 - 0.75, 10.0], rtol=0, atol=1e-15)
    assert np.array_equal(frames.box_corners([box])[0], c)
    if ry == 0.0:
        assert np.array_equal(c[:, 0], [3, 3, -1, -1, 3, 3, -1, -1]) and np.array_equal(c[:, 1], [1.5] * 4 + [0.0] * 4)
        assert np.array_equal(c[:, 2], [10.875, 9.125, 9.125, 10.875, 10.875, 9.125, 9.125, 10.875])


def test_keep_rules():
    assert not ft.keep((0, 100, 50, 124), 40)                           # 24 px high, with points
    assert not ft.keep((0, 100, 50, 125), 4)                            # 25 px high, 4 points
    assert ft.keep((0, 100, 50, 125), 5)                                # 25 px high, 5 points
    assert not ft.keep((0, 100, 50, 125), 40, positives=0)              # ground truth: points but no positive
    assert ft.keep((0, 100, 50, 125), 3, positives=1)                   # ground truth: one positive is enough
    assert not ft.keep((0, 100, 50, 124), 40, positives=7)
    # the whole extraction on a tiny frame: 6 points at z = 4 in one column of boxes
    scan = np.array([[2.5 + 0.25 * i, 0.25, 4.0, i] for i in range(6)], dtype=np.float32)       # u = 940 + 32 i, v = 219.5
    boxes = [(930, 200, 1200, 224), (930, 200, 1200, 225), (930, 200, 1040, 225), (930, 200, 1070, 225)]
    got = ft.extract(scan, P, R0, V2C, boxes, SIZE)
    assert got['counts'][:, 0].tolist() == [6, 6, 4, 5] and got['kept'].tolist() == [1, 3] and got['offsets'].tolist() == [0, 6, 11]
    assert np.array_equal(got['rows'], np.concatenate([scan, scan[:5]]))
    box3 = [(1.0, 1.0, 0.3, 2.5, 0.5, 4.0, 0.0)] * 3 + [(1.0, 1.0, 0.3, 50.0, 0.5, 4.0, 0.0)]
    got = ft.extract(scan, P, R0, V2C, boxes, SIZE, boxes_3d=box3)
    assert got['counts'].tolist() == [[6, 1], [6, 1], [4, 1], [5, 0]] and got['kept'].tolist() == [1, 2]
    assert got['labels'].tolist() == [1, 0, 0, 0, 0, 0] + [1, 0, 0, 0]


def test_parity_sampling_of_the_truth():
    scan = np.array([[2.5 + 0.25 * i, 0.25, 4.0, i] for i in range(6)], dtype=np.float32)
    boxes = [(930, 200, 1200, 225), (930, 200, 1040, 225)]
    choices = np.array([[0, 5, 9, -3], [0, 1, 2, 3]])
    f, hot, rot, score, valid = ft.batch(scan, P, R0, V2C, boxes, SIZE, [1, 2], [0.5, 0.25], choices, 4, frustum_rotate=False, bmax=3)
    assert valid.tolist() == [1, 0, 0] and np.array_equal(f[0], scan[[0, 5, 5, 0]].T) and not f[1:].any()
    assert hot.tolist() == [[0, 1, 0], [0, 0, 0], [0, 0, 0]] and score.tolist() == [0.5, 0, 0]
    assert rot[0] == np.float32(np.pi / 2 + ft.frustum_angle(P, boxes[0])) and not rot[1:].any()


def test_calibration_from_file(tmp_path):
    rng = np.random.RandomState(3)
    mats = {'P0': rng.rand(12), 'P2': rng.rand(12) * 700, 'R0_rect': rng.rand(9), 'Tr_velo_to_cam': rng.rand(12), 'Tr_imu_to_velo': rng.rand(12)}
    path = tmp_path / '000007.txt'
    path.write_text(''.join('{}: {}\n'.format(k, ' '.join(repr(float(x)) for x in v)) for k, v in mats.items()) + '\n')
    calib = frames.Calibration.from_file(str(path))
    assert np.array_equal(calib.P, mats['P2'].reshape(3, 4)) and np.array_equal(calib.R0, mats['R0_rect'].reshape(3, 3))
    assert np.array_equal(calib.V2C, mats['Tr_velo_to_cam'].reshape(3, 4))
    assert np.array_equal(calib.packed(), np.concatenate([mats['P2'], mats['Tr_velo_to_cam'], mats['R0_rect']]))
    (tmp_path / 'bad.txt').write_text('P2: 1 2 3\n')
    with pytest.raises(ValueError, match='R0_rect'):
        frames.Calibration.from_file(str(tmp_path / 'bad.txt'))
    scan = rng.rand(7, 4).astype(np.float32)
    scan.tofile(str(tmp_path / 'scan.bin'))
    assert np.array_equal(frames.read_scan(str(tmp_path / 'scan.bin')), scan)


def test_label_lines_are_the_reference_format():
    pred = np.array([[1.5, 1.6, 3.9, 1.0, 1.5, 10.0, -0.3, 0.9], [1.7, 0.6, 0.8, -2.0, 1.4, 20.0, 1.2, 0.4]])
    lines = frames.kitti_label_lines(['Car', 'Pedestrian'], [[10, 20, 30, 40], [1.5, 2.5, 3.5, 4.5]], pred, [1, 0])
    assert lines == ['Car -1 -1 -10 10.000000 20.000000 30.000000 40.000000 1.500000 1.600000 3.900000 1.000000 1.500000 10.000000 '
                     '-0.300000 0.900000\n']
    assert len(frames.kitti_label_lines(['Car', 'Pedestrian'], np.zeros((2, 4)), pred)) == 2


FRAME_EXPORTS = ['pvcnn_frame_tiles', 'pvcnn_frame_project', 'pvcnn_frame_count', 'pvcnn_frame_pack', 'pvcnn_frame_batch',
                 'pvcnn_frame_rotate_rows']


def test_the_exports_are_declared_bound_and_built_and_the_abi_version_stays():
    from pvcnn_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'pvcnn_hip.h')).read()
    for name in FRAME_EXPORTS:
        assert re.search(r'PVCNN_API\s+[\w\s\*]+?\b' + name + r'\s*\(', header), name
        assert name in _lib.SIGNATURES, name
    makefile = open(os.path.join(ROOT, 'pvcnn_amd', 'csrc', 'Makefile')).read()
    assert 'frames.hip' in re.search(r'^SRCS\s*:=(.*)$', makefile, flags=re.M).group(1).split()
    assert re.search(r'#define\s+PVCNN_ABI_VERSION\s+17\b', header) and _lib.ABI_VERSION == 17
    assert int(re.search(r'#define\s+PVCNN_FRAME_BOX_COLUMNS\s+(\d+)', header).group(1)) == frames.BOX_COLUMNS
    lib = _lib.load()
    assert lib.pvcnn_frame_tiles(1) == 1 and lib.pvcnn_frame_tiles(64) == 1 and lib.pvcnn_frame_tiles(65) == 2
    assert lib.pvcnn_frame_tiles(0) == 0 and lib.pvcnn_frame_tiles((1 << 30) + 1) == 0


def test_every_entry_point_refuses_to_run_without_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)      # (a machine with a GPU sees the same error)
    calib = frames.Calibration(P, R0, V2C)
    scan, boxes = _lattice(), [(0.0, 0.0, 1242.0, 375.0)]
    calls = [lambda: frames.project_scan(scan, calib, SIZE),
             lambda: frames.extract_frustums(scan, calib, boxes, SIZE, classes=['Car']),
             lambda: frames.frame_batch(scan, calib, boxes, SIZE, [0], scores=[1.0], num_points=8),
             lambda: frames.detect_frame(None, scan, calib, boxes, SIZE, [0], [1.0], torch.zeros(8, 3), num_points=8),
             lambda: frames.frame_batch(torch.from_numpy(scan), calib, boxes, SIZE, [0])]
    for call in calls:
        with pytest.raises(RuntimeError, match='no CPU implementation'):
            call()
    from pvcnn_amd.data import DeviceFrustumKitti
    cpu = frames.FrameFrustums(torch.zeros(1, 4), None, torch.tensor([0, 1]), torch.tensor([0]), ['Car'], np.zeros((1, 4)), np.zeros(1),
                               np.ones(1, dtype=np.int64), scores=np.ones(1))
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        DeviceFrustumKitti.from_frustums(cpu, 8)
