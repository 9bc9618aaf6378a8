"""Device-resident datasets, host side (pvcnn_amd/data.py): the torch formulation of every assembly reproduces what the REFERENCE's
dataset classes + default_collate produced for the same draws (tests/golden/datasets.pt, written by tests/golden/gen_dataset_golden.py)
bit for bit; packing round-trips; DeviceLoader counts batches as DataLoader does; bad arguments are refused.  No GPU needed."""
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, RandomSampler, TensorDataset

from conftest import ROOT

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'datasets.pt')


@pytest.fixture(scope='module')
def golden():
    return torch.load(GOLDEN)


def same(got, want, what):
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(got.cpu(), want), what


def same_batch(got, want, what):
    for g, w in zip(got, want):
        if isinstance(w, dict):
            assert sorted(g) == sorted(w), what
            for k in w:
                same(g[k], w[k], f'{what}: {k}')
        else:
            same(g, w, what)


# ---- builders shared with tests/test_gpu_data.py ----
def s3dis_store(g, case, device='cpu'):
    from pvcnn_amd.data import DeviceS3DIS
    return DeviceS3DIS(g['data'], g['label_seg'], g['data_num'], g['num_points'], with_normalized_coords=case['with_normalized_coords'],
                       device=device)


def shapenet_store(g, case, device='cpu'):
    from pvcnn_amd.data import DeviceShapeNet
    return DeviceShapeNet([c.numpy() for c in g['clouds']], g['shape_ids'], g['num_points'], with_normal=case['with_normal'],
                          with_one_hot_shape_id=case['with_one_hot_shape_id'], normalize=case['normalize'], jitter=case['jitter'],
                          device=device)


def frustum_store(g, case, device='cpu', rgb=False):
    from pvcnn_amd.data import DeviceFrustumKitti
    clouds = [c.numpy() for c in g['point_clouds']]
    angles = [np.float64(a) for a in g['frustum_rotation_angles']]
    if rgb:
        return DeviceFrustumKitti.from_rgb_detection(clouds, g['class_names'], angles, g['probs'], g['num_points'], classes=g['classes'],
                                                     frustum_rotate=case['frustum_rotate'], device=device)
    return DeviceFrustumKitti(clouds, [m.numpy() for m in g['mask_logits']], [b.numpy() for b in g['boxes_3d']],
                              [np.float64(h) for h in g['heading_angles']], [s.numpy() for s in g['sizes']], g['class_names'], angles,
                              g['num_points'], classes=g['classes'], num_heading_angle_bins=g['num_heading_angle_bins'],
                              class_name_to_size_template_id=g['class_name_to_size_template_id'],
                              size_templates={k: v.numpy() for k, v in g['size_templates'].items()}, random_flip=case['random_flip'],
                              random_shift=case['random_shift'], frustum_rotate=case['frustum_rotate'], device=device)


def golden_cases(g):
    """(name, store builder, item indices, draws as keyword arguments, expected batch) of every golden case."""
    for i, c in enumerate(g['s3dis']['cases']):
        yield (f's3dis[{i}]', (lambda d, c=c: s3dis_store(g['s3dis'], c, d)), c['indices'], {'choices': c['choices']},
               (c['features'], c['targets']))
    for i, c in enumerate(g['shapenet']['cases']):
        yield (f'shapenet[{i}]', (lambda d, c=c: shapenet_store(g['shapenet'], c, d)), c['indices'],
               {'choices': c['choices'], 'jitter': c['jitter_draws']}, (c['features'], c['targets']))
    for i, c in enumerate(g['frustum']['cases']):
        yield (f'frustum[{i}]', (lambda d, c=c: frustum_store(g['frustum'], c, d)), c['indices'],
               {'choices': c['choices'], 'flip': c['flip'], 'shift': c['shift']}, (c['inputs'], c['targets']))
    for i, c in enumerate(g['frustum']['rgb_cases']):
        yield (f'frustum_rgb[{i}]', (lambda d, c=c: frustum_store(g['frustum'], c, d, rgb=True)), c['indices'], {'choices': c['choices']},
               (c['inputs'], c['targets']))


def test_golden_holds_the_cases_the_feature_is_specified_on(golden):
    s = golden['s3dis']
    n, N = s['data_num'].tolist(), s['num_points']
    assert any(1 < x < N for x in n) and any(x == N for x in n) and any(x > N for x in n) and any(x == 1 for x in n)
    assert {c['with_normalized_coords'] for c in s['cases']} == {True, False}
    forms = {(c['with_normal'], c['with_one_hot_shape_id'], c['jitter']) for c in golden['shapenet']['cases']}
    assert len(forms) == 8
    z = torch.cat([c['jitter_draws'].flatten() for c in golden['shapenet']['cases'] if c['jitter']])
    assert (z.abs() > 5).any()                                                       # the clip is exercised
    f = golden['frustum']
    assert set(f['class_names']) == set(f['classes']) and len(f['classes']) == 3
    assert len({(c['frustum_rotate'], c['random_flip'], c['random_shift']) for c in f['cases']}) == 8
    flips = torch.cat([c['flip'] for c in f['cases'] if c['random_flip']])
    assert (flips > 0.5).any() and (flips < 0.5).any() and (flips == 0.5).any()
    assert len(f['rgb_cases']) >= 1
    assert os.path.getsize(GOLDEN) < os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'pvcnn_c0p125_eval.pt'))


def test_torch_formulation_reproduces_the_reference_bit_for_bit(golden):
    count = 0
    for name, build, indices, draws, want in golden_cases(golden):
        store = build('cpu')
        same_batch(store.assemble_reference(indices, **draws), want, name)
        count += 1
    assert count == 2 + 9 + 8 + 2


def test_packing_round_trips(golden):
    s = golden['s3dis']
    store = s3dis_store(s, {'with_normalized_coords': True})
    assert len(store) == s['data'].shape[0] and store.max_n == int(s['data_num'].max())
    assert store.offsets.dtype == torch.int64 and store.offsets.tolist() == [0] + torch.cumsum(s['data_num'], 0).tolist()
    assert store.rows.dtype == torch.float32 and store.labels.dtype == torch.uint8           # 13 classes fit a byte
    for w in range(len(store)):
        rows, labels = store.item(w)
        n = int(s['data_num'][w])
        assert torch.equal(rows, s['data'][w, :n].float()) and torch.equal(labels.long(), s['label_seg'][w, :n].long())
    total = int(s['data_num'].sum())
    assert store.nbytes == total * 9 * 4 + total * 1 + (len(store) + 1) * 8
    # labels that need more than a byte, or a sign, get a wider type
    from pvcnn_amd.data import DeviceS3DIS
    wide = DeviceS3DIS(s['data'], s['label_seg'].long() * 100 - 5, s['data_num'], 16, device='cpu')
    assert wide.labels.dtype == torch.int16 and torch.equal(wide.item(2)[1].long(), s['label_seg'][2, :40].long() * 100 - 5)
    huge = DeviceS3DIS(s['data'], s['label_seg'].long() * 2 ** 40, s['data_num'], 16, device='cpu')
    assert huge.labels.dtype == torch.int64
    # ShapeNet and Frustum-KITTI keep every row of every item
    g = golden['shapenet']
    sn = shapenet_store(g, {'with_normal': True, 'with_one_hot_shape_id': True, 'normalize': False, 'jitter': False})
    for i, cloud in enumerate(g['clouds']):
        rows, labels = sn.item(i)
        assert torch.equal(rows, cloud[:, :6].float()) and torch.equal(labels.long(), cloud[:, 6].float().long())
    f = golden['frustum']
    fr = frustum_store(f, {'random_flip': False, 'random_shift': False, 'frustum_rotate': False})
    for i, cloud in enumerate(f['point_clouds']):
        rows, labels = fr.item(i)
        assert torch.equal(rows, cloud) and torch.equal(labels.double(), f['mask_logits'][i])
    assert fr.nbytes > fr.rows.numel() * 4 and fr.to('cpu').nbytes == fr.nbytes


@pytest.mark.parametrize('n,batch,drop_last', [(6, 4, False), (6, 4, True), (6, 3, False), (6, 7, False), (6, 7, True), (6, 1, True)])
def test_loader_counts_batches_as_dataloader_does(golden, n, batch, drop_last):
    from pvcnn_amd.data import DeviceLoader
    store = s3dis_store(golden['s3dis'], {'with_normalized_coords': True})
    assert len(store) == n
    ref = DataLoader(TensorDataset(torch.zeros(n, 9, 16), torch.zeros(n, 16, dtype=torch.int64)), batch_size=batch, drop_last=drop_last)
    loader = DeviceLoader(store, batch, shuffle=False, drop_last=drop_last)
    assert len(loader) == len(ref)
    assert loader.order.tolist() == list(range(n)) and loader.cursor.tolist() == [0]            # SequentialSampler
    ref_batches = list(ref)
    assert loader.batch_sizes() == [x.shape[0] for x, _ in ref_batches]
    for size, (x, y) in zip(loader.batch_sizes(), ref_batches):
        fx, fy = store.empty_batch(size)
        assert fx.shape == x.shape and fy.shape == y.shape and fx.dtype == x.dtype and fy.dtype == y.dtype
    assert [t.shape[0] for t in loader.static_batch()] == [batch, batch]


def test_loader_order_is_the_samplers_permutation(golden):
    from pvcnn_amd.data import DeviceLoader
    store = s3dis_store(golden['s3dis'], {'with_normalized_coords': True})
    g1, g2 = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    loader = DeviceLoader(store, 4, shuffle=True, generator=g1)                         # the first epoch's permutation
    assert loader.order.tolist() == list(RandomSampler(range(len(store)), generator=g2))
    first = loader.order.tolist()
    loader.cursor.add_(4)
    loader.new_epoch()                                                                  # same tensor, new permutation, cursor 0
    assert loader.order.tolist() != first
    assert sorted(loader.order.tolist()) == list(range(len(store))) and loader.cursor.tolist() == [0]
    halves = [DeviceLoader(store, 2, shuffle=False, rank=r, world_size=2) for r in range(2)]
    assert halves[0].order.tolist() == [0, 2, 4] and halves[1].order.tolist() == [1, 3, 5] and len(halves[0]) == 2


def test_constructor_and_argument_errors(golden):
    from pvcnn_amd.data import DeviceFrustumKitti, DeviceLoader, DeviceS3DIS, DeviceShapeNet
    s = golden['s3dis']
    with pytest.raises(ValueError, match=r'\(W, P, 9\)'):
        DeviceS3DIS(s['data'][:, :, :6], s['label_seg'], s['data_num'], 16, device='cpu')
    with pytest.raises(ValueError, match='must match'):
        DeviceS3DIS(s['data'], s['label_seg'][:3], s['data_num'], 16, device='cpu')
    with pytest.raises(ValueError, match=r'\[1, P\]'):
        DeviceS3DIS(s['data'], s['label_seg'], torch.zeros_like(s['data_num']), 16, device='cpu')
    with pytest.raises(ValueError, match='num_points'):
        DeviceS3DIS(s['data'], s['label_seg'], s['data_num'], 0, device='cpu')
    g = golden['shapenet']
    with pytest.raises(ValueError, match='one shape id per cloud'):
        DeviceShapeNet([c.numpy() for c in g['clouds']], g['shape_ids'][:2], 24, device='cpu')
    with pytest.raises(ValueError, match=r'\(n, 7\)'):
        DeviceShapeNet([g['clouds'][0].numpy()[:, :6]], [0], 24, device='cpu')
    with pytest.raises(ValueError, match='shape ids'):
        DeviceShapeNet([g['clouds'][0].numpy()], [16], 24, device='cpu')
    f = golden['frustum']
    clouds = [c.numpy() for c in f['point_clouds']]
    with pytest.raises(ValueError, match='class names'):
        DeviceFrustumKitti.from_rgb_detection(clouds, ['Tram'] * 6, f['frustum_rotation_angles'], f['probs'], 32, device='cpu')
    with pytest.raises(ValueError, match='one entry per point cloud'):
        DeviceFrustumKitti.from_rgb_detection(clouds, f['class_names'][:2], f['frustum_rotation_angles'], f['probs'], 32, device='cpu')
    store = frustum_store(f, {'random_flip': True, 'random_shift': True, 'frustum_rotate': True})
    case = f['cases'][7]
    idx = case['indices']
    with pytest.raises(ValueError, match='choices'):
        store.assemble_reference(idx)
    with pytest.raises(ValueError, match='flip'):
        store.assemble_reference(idx, choices=case['choices'])
    with pytest.raises(ValueError, match='choices of shape'):
        store.assemble_reference(idx, choices=case['choices'][:, :5], flip=case['flip'], shift=case['shift'])
    with pytest.raises(IndexError):
        store.assemble_reference([6], choices=case['choices'][:1], flip=case['flip'][:1], shift=case['shift'][:1])
    # the product path never computes on the host
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        store.assemble(idx, choices=case['choices'], flip=case['flip'], shift=case['shift'])
    with pytest.raises(ValueError, match='batch_size'):
        DeviceLoader(store, 0)
    with pytest.raises(ValueError, match='rank'):
        DeviceLoader(store, 2, rank=2, world_size=2)


def test_h5py_is_not_an_import_time_dependency():
    import sys
    import pvcnn_amd.data                                      # noqa: F401
    assert 'h5py' not in sys.modules
