"""Device mode of every data kernel against tests/golden/device_draws.pt, bit for bit: what a seed means does not change.

The golden was recorded once, by tests/golden/gen_device_draws_golden.py, from `record()` below on the library of the commit its
docstring names; tests/test_device_draws_host.py checks the recording's integer draws against the numpy stream (draws_truth.py) on the
CPU.  The shapes are the smallest that reach every branch of the draws: S3DIS windows of 40 (picks with replacement), 64 and 70 points
(the sorted selection, padded to 64 and to 128 words) at N = 64; ShapeNet's jitter; Frustum-KITTI's flip and shift; frame_batch and
the frame store over several tiles with a ragged last one; augment's per-cloud and per-point draws; mask_select with k >= M and with
k < M (repeat and shuffle); a room whose cells resample and shuffle."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, SEED

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'device_draws.pt')
# seed[0] with bits in both halves, seed[1] above 2^32 (only its low half is the stream): the truncations show
SEED_WORDS = {'s3dis': (0x0123456789ABCDEF, (5 << 32) | 7), 'shapenet': (0x0FEDCBA987654321, (1 << 40) | 3),
              'frustum': (0x1111222233334444, (9 << 32) | 1), 'frame_batch': (0x2222333344445555, (2 << 32) | 11),
              'frame_store': (0x3333444455556666, (3 << 32) | 4), 'augment': (0x0444555566667777, (4 << 32) | 13),
              'mask_select': (0x0555666677778888, (6 << 32) | 5)}
S3DIS_COUNTS, S3DIS_POINTS = [40, 64, 70], 64
SHAPENET_COUNTS, SHAPENET_POINTS = [50, 130], 64
FRUSTUM_COUNTS, FRUSTUM_POINTS = [20, 33, 100], 32
FRAME_STORE_FRAMES, FRAME_STORE_POINTS, FRAME_STORE_BATCH = ((5, 300, 2), (6, 203, 2)), 32, 4       # test_gpu_frame_store.frame's arguments
MASK_CASES = {'k_ge_m': (100, 32, 0.6), 'k_lt_m': (100, 150, 0.4)}                                  # N, M, foreground share


def words(name):
    return torch.tensor(SEED_WORDS[name], dtype=torch.int64, device=DEV)


def frustum_clouds():
    """Clouds whose reflectance (channel 3, which neither flip nor shift touches) is the row's position in its item."""
    rng = np.random.RandomState(SEED + 7)
    clouds = [(rng.randn(n, 4) * [2, 1, 5, 1] + [0, 1, 20, 0]).astype(np.float32) for n in FRUSTUM_COUNTS]
    for c in clouds:
        c[:, 3] = np.arange(len(c), dtype=np.float32)
    return rng, clouds


def frustum_stores():
    from pvcnn_amd.data import DeviceFrustumKitti
    rng, clouds = frustum_clouds()
    classes, w = ('Car', 'Pedestrian', 'Cyclist'), len(clouds)
    names = [classes[i % 3] for i in range(w)]
    angles = [np.float64(a) for a in rng.uniform(-2, -1, size=w)]
    truth = DeviceFrustumKitti(clouds, [rng.randint(0, 2, size=n) for n in FRUSTUM_COUNTS], [rng.randn(8, 3) + [1, 1, 20] for _ in range(w)],
                               [np.float64(h) for h in rng.uniform(-np.pi, np.pi, size=w)], [rng.rand(3) + 1 for _ in range(w)], names,
                               angles, FRUSTUM_POINTS, classes=classes, class_name_to_size_template_id={'Car': 0, 'Pedestrian': 3, 'Cyclist': 5},
                               size_templates={c: rng.rand(3) + 1 for c in classes}, random_flip=True, random_shift=True, device=DEV)
    rgb = DeviceFrustumKitti.from_rgb_detection(clouds, names, angles, rng.rand(w), FRUSTUM_POINTS, classes=classes, device=DEV)
    return truth, rgb


def masks():
    rng = np.random.RandomState(SEED + 9)
    return {name: torch.from_numpy(rng.rand(2, n) < share) for name, (n, _, share) in MASK_CASES.items()}


def rooms():
    """(xyzrgb, prepare_room options): the one-block lattice of the shuffle test, and one block of the resampling test's lattice."""
    from test_gpu_rooms import _lattice_room
    shuffle = _lattice_room([(i, j, 0) for i in range(6) for j in range(5)], [1] * 30)[0]
    cells = [(i, j, k) for i in range(6) for j in range(6) for k in range(8)]
    resample = _lattice_room(cells, [2 if (i + j + k) % 2 == 0 else 4 for i, j, k in cells])[0]
    return {'shuffle': (shuffle, dict(max_num_points=10, block_size=1.5, grid_size=0.25)),
            'resample': (resample, dict(max_num_points=4096, block_size=1.5, grid_size=0.25))}


def _put(out, prefix, value):
    if isinstance(value, dict):
        for k, v in value.items():
            _put(out, f'{prefix}.{k}', v)
    elif isinstance(value, (tuple, list)):
        for i, v in enumerate(value):
            _put(out, f'{prefix}.{i}', v)
    elif value is not None:
        out[prefix] = value.detach().cpu().clone()


def record(backend):
    """name -> CPU tensor: the complete outputs of device mode of every data kernel for the fixed seed words."""
    from pvcnn_amd import frames
    from pvcnn_amd.augment import Augment
    from pvcnn_amd.data import DeviceShapeNet
    from pvcnn_amd.frame_store import DeviceKittiFrames
    from pvcnn_amd.rooms import prepare_room
    import test_gpu_augment as ta
    import test_gpu_data as td
    import test_gpu_frame_store as ts
    import test_gpu_frames as tf
    from test_gpu_rooms import _gen
    out = {}
    for channels, with_norm in ((9, True), (6, False)):
        store = td.indexed_s3dis(S3DIS_COUNTS, S3DIS_POINTS, with_normalized_coords=with_norm)
        _put(out, f's3dis{channels}', store.assemble([0, 1, 2], seed=words('s3dis')))
    rng = np.random.RandomState(SEED + 5)
    clouds = [np.concatenate([rng.randn(n, 6), rng.randint(0, 50, size=(n, 1))], axis=1) for n in SHAPENET_COUNTS]
    _put(out, 'shapenet', DeviceShapeNet(clouds, [3, 7], SHAPENET_POINTS, device=DEV).assemble([0, 1], seed=words('shapenet')))
    truth, rgb = frustum_stores()
    _put(out, 'frustum', truth.assemble([0, 1, 2], seed=words('frustum')))
    _put(out, 'frustum_rgb', rgb.assemble([0, 1, 2], seed=words('frustum')))
    scan, boxes, _, scores = tf.frame(0)
    _put(out, 'frame_batch', frames.frame_batch(scan, tf.calibration(), boxes, tf.SIZE, tf.CLASS_IDS, scores=scores, num_points=64,
                                                frustum_rotate=True, seed=words('frame_batch')))
    store = DeviceKittiFrames([(ts.frame(*f)[0], ts.calibration(), ts.SIZE) + ts.frame(*f)[1:] for f in FRAME_STORE_FRAMES],
                              FRAME_STORE_POINTS, class_name_to_size_template_id=ts.TEMPLATE_IDS, size_templates=ts.TEMPLATES,
                              random_flip=True, random_shift=True, frustum_rotate=True, shift_ratio=0.1)
    assert len(store) == FRAME_STORE_BATCH
    draws = store.empty_draws(FRAME_STORE_BATCH)
    _put(out, 'frame_store', store.assemble(list(range(FRAME_STORE_BATCH)), seed=words('frame_store'), draws_out=draws))
    _put(out, 'frame_store.draws', draws)
    for name, aug, c in (('s3dis', Augment.s3dis(**ta.ALL_ON), 9), ('shapenet', Augment.shapenet(**ta.ALL_ON), 22)):
        x, y = ta.batch(np.random.RandomState(SEED + 6), 2, c, 70)
        _put(out, f'augment_{name}.draw', aug.draw(2, words('augment')))
        _put(out, f'augment_{name}', aug.augment(x.to(DEV), y.to(DEV), seed=words('augment'), return_draws=True))
    for name, mask in masks().items():
        _put(out, f'mask_select.{name}', backend.mask_select(mask.to(DEV).contiguous(), MASK_CASES[name][1], seed=words('mask_select')))
    for name, (xyzrgb, options) in rooms().items():
        w = prepare_room(torch.from_numpy(xyzrgb).to(DEV), None, generator=_gen(SEED), **options)
        _put(out, f'room_{name}', {'rows': w.rows, 'indices': w.indices, 'offsets': w.offsets, 'window_block': w.window_block,
                                   'data_num': w.data_num})
    return out


def test_device_mode_writes_the_recorded_bits(hip):
    from test_gpu_frames import same
    want = torch.load(GOLDEN)
    got = record(hip)
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if not same(got[k], want[k])]
    assert not differ, differ
