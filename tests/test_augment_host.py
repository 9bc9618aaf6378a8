"""Batch augmentation, host side (pvcnn_amd/augment.py): the torch formulation on hand-written clouds, the composed matrix, argument
validation, and the library's argument refusals (no launch is made: nothing is dereferenced).  No GPU needed."""
import ctypes
import math

import numpy as np
import pytest
import torch

from pvcnn_amd.augment import DIRECTION, PARAMS, POSITION, Augment, compose_reference

SEED = 1588147245


def identity_params(b):
    p = torch.zeros((b, PARAMS), dtype=torch.float64)
    p[:, 0] = p[:, 4] = p[:, 8] = 1.0
    p[:, 9] = 1.0
    return p


def cloud(b, c, n, seed=SEED):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((b, c, n), generator=g), torch.randint(0, 13, (b, n), generator=g)


def test_all_stages_off_is_the_identity_bit_for_bit():
    x, y = cloud(3, 9, 257)
    got_x, got_y = Augment.s3dis().augment_reference(x, y, identity_params(3))
    assert got_x.dtype == torch.float32 and got_y.dtype == torch.int64
    assert torch.equal(got_x.view(torch.int32), x.view(torch.int32))
    assert torch.equal(got_y, y) and got_x.data_ptr() != x.data_ptr()
    # draws of a stage that is off are not needed and not looked at
    got_x, _ = Augment.shapenet().augment_reference(x, None, identity_params(3), jitter=torch.ones(3, 3, 257), keep=torch.zeros(3, 257))
    assert torch.equal(got_x, x)


def test_quarter_turn_about_z_of_a_hand_written_cloud():
    # points (1, 0, 5), (0, 2, -1), (3, 4, 0) with normals along x, y, z and a seventh channel that must pass through
    x = torch.tensor([[[1.0, 0.0, 3.0], [0.0, 2.0, 4.0], [5.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [7.0, 8.0, 9.0]]])
    aug = Augment(layout=[('position', 0), ('direction', 3)])
    raw = np.zeros((1, PARAMS))
    raw[0, 14] = math.pi / 2
    rp = compose_reference(raw)
    params = identity_params(1)
    params[0, :9] = torch.from_numpy(np.round(rp[0]).reshape(9))              # cos(pi / 2) = 6e-17 in fp64: the exact quarter turn
    assert np.abs(rp[0] - np.round(rp[0])).max() < 1e-15
    got, _ = aug.augment_reference(x, None, params)
    want = torch.tensor([[[0.0, -2.0, -4.0], [1.0, 0.0, 3.0], [5.0, -1.0, 0.0], [0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [7.0, 8.0, 9.0]]])
    assert torch.equal(got, want)


def test_directions_ignore_scale_translation_and_jitter():
    x, _ = cloud(2, 6, 33)
    aug = Augment.shapenet(scale=(0.5, 2.0), translate=1.0, jitter_sigma=0.1, jitter_clip=0.2)
    params = identity_params(2)
    params[:, 9] = torch.tensor([0.5, 2.0])
    params[:, 10:13] = torch.tensor([[0.25, -0.5, 1.0], [0.0, 0.125, -1.0]])
    z = torch.randn(2, 3, 33, generator=torch.Generator().manual_seed(1))
    z[0, 0, :2] = torch.tensor([50.0, -50.0])                                # clipped at both ends
    got, _ = aug.augment_reference(x, None, params, jitter=z)
    assert torch.equal(got[:, 3:6], x[:, 3:6])
    want = (params[:, 9, None, None] * x[:, :3].double() + params[:, 10:13, None] + (0.1 * z.double()).clamp(-0.2, 0.2)).float()
    assert torch.equal(got[:, :3], want)
    assert got[0, 0, 0].item() == np.float32(0.5 * float(x[0, 0, 0]) + 0.25 + 0.2)
    assert got[0, 0, 1].item() == np.float32(0.5 * float(x[0, 0, 1]) + 0.25 - 0.2)


def test_a_dropped_point_is_point_0_in_every_channel_and_in_its_target():
    x, y = cloud(2, 9, 40)
    aug = Augment.s3dis(scale=(0.9, 1.1), jitter_sigma=0.01, jitter_clip=0.05, dropout_max=0.875)
    params = identity_params(2)
    params[:, 9] = torch.tensor([0.9, 1.1])
    params[:, 13] = torch.tensor([0.5, 0.0])
    keep = torch.rand(2, 40, generator=torch.Generator().manual_seed(2))
    keep[0, 0] = 0.0                                                          # point 0 itself is never dropped
    keep[0, 7] = 0.5                                                          # u == ratio drops (PointNet++: <=)
    keep[1, 3] = 0.0                                                          # ... also at ratio 0
    z = torch.randn(2, 3, 40, generator=torch.Generator().manual_seed(3))
    got_x, got_y = aug.augment_reference(x, y, params, jitter=z, keep=keep)
    undropped_x, _ = aug.augment_reference(x, y, params, jitter=z, keep=torch.ones(2, 40))
    dropped = keep.double() <= params[:, 13, None]
    dropped[:, 0] = False
    assert dropped[0, 7] and dropped[1, 3] and 5 < int(dropped.sum()) < 35
    for b in range(2):
        for n in range(40):
            src = 0 if dropped[b, n] else n
            assert torch.equal(got_x[b, :, n], undropped_x[b, :, src]) and got_y[b, n] == y[b, src], (b, n)


def test_composed_matrix_is_orthogonal_with_the_determinant_of_its_flips():
    rng = np.random.RandomState(SEED)
    raw = np.zeros((512, PARAMS))
    raw[:, 14] = rng.uniform(-math.pi, math.pi, 512)
    raw[:, 15:18] = np.clip(0.06 * rng.randn(512, 3), -0.18, 0.18)
    raw[:, 18:21] = rng.random_sample((512, 3))
    for axis in (0, 1, 2):
        rp = compose_reference(raw, axis, (0.5, 0.25, 0.75))
        assert np.abs(rp @ rp.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-12
        flips = (raw[:, 18:21] < [0.5, 0.25, 0.75]).sum(axis=1)
        assert 0 in flips and 3 in flips
        assert np.abs(np.linalg.det(rp) - (-1.0) ** flips).max() <= 1e-12
    # without perturbation and flips: the plain rotation about the axis, which leaves the axis where it is
    raw[:, 15:21] = 0.0
    for axis in (0, 1, 2):
        rp = compose_reference(raw, axis)
        e = np.eye(3)[axis]
        assert np.abs(rp @ e - e).max() <= 1e-15 and np.abs(np.linalg.det(rp) - 1.0).max() <= 1e-12
    quarter = np.zeros(PARAMS)
    quarter[14] = math.pi / 2
    assert np.allclose(compose_reference(quarter, 2) @ [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], atol=1e-15)     # right-handed: x -> y about z
    assert np.allclose(compose_reference(quarter, 0) @ [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], atol=1e-15)     # y -> z about x
    assert np.allclose(compose_reference(quarter, 1) @ [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], atol=1e-15)     # z -> x about y
    # the method uses the object's own axis and probabilities
    aug = Augment(rotate_axis=1, rotate_max=1.0, flip_prob=(1.0, 0.0, 0.0))
    assert np.array_equal(aug.compose_reference(quarter), compose_reference(quarter, 1, (1.0, 0.0, 0.0)))


def test_argument_validation():
    from pvcnn_amd.data import DeviceLoader, DeviceS3DIS
    x, y = cloud(2, 6, 8)
    with pytest.raises(ValueError, match='overlap'):
        Augment(layout=[('position', 0), ('direction', 2)])
    with pytest.raises(ValueError, match='low <= high'):
        Augment(scale=(1.1, 0.9))
    with pytest.raises(ValueError, match='at most 4'):
        Augment(layout=[('position', 3 * k) for k in range(5)])
    with pytest.raises(ValueError, match='roles'):
        Augment(layout=[('colour', 3)])
    with pytest.raises(ValueError, match='clip'):
        Augment(jitter_sigma=0.01)
    with pytest.raises(ValueError):
        Augment(rotate_axis=3)
    with pytest.raises(ValueError):
        Augment(flip_prob=(0.5, 0.5))
    with pytest.raises(ValueError):
        Augment(dropout_max=1.5)
    Augment(jitter_sigma=0.01, jitter_clip=math.inf, perturb_sigma=0.06, perturb_clip=0.18, dropout_max=1.0)
    # a layout beyond C
    with pytest.raises(ValueError, match='channels 6..8'):
        Augment(layout=[('position', 0), ('direction', 6)]).augment_reference(x, y, identity_params(2))
    with pytest.raises(ValueError, match='channels 4..6'):
        Augment(layout=[('position', 4)]).augment_reference(x, y, identity_params(2))
    # draws: wrong shapes, a stage without its draws
    with pytest.raises(ValueError, match='params of shape'):
        Augment().augment_reference(x, y, torch.zeros(2, 12, dtype=torch.float64))
    with pytest.raises(ValueError, match='`jitter`'):
        Augment(jitter_sigma=0.01, jitter_clip=0.05).augment_reference(x, y, identity_params(2))
    with pytest.raises(ValueError, match='keep of shape'):
        Augment(dropout_max=0.5).augment_reference(x, y, identity_params(2), keep=torch.zeros(2, 9))
    with pytest.raises(ValueError, match='targets'):
        Augment().augment_reference(x, y[:, :4], identity_params(2))
    # the product path has no CPU implementation
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        Augment().augment(x, y)
    # loaders: a layout beyond the store's channels, a Frustum-KITTI store
    rng = np.random.RandomState(SEED)
    store = DeviceS3DIS(rng.rand(3, 20, 9), rng.randint(0, 13, (3, 20)), np.array([20, 12, 7]), 16, with_normalized_coords=False, device='cpu')
    assert DeviceLoader(store, 2, augment=Augment.s3dis(rotate_max=math.pi)).augment.rotate_max == math.pi
    assert DeviceLoader(store, 2).augment is None
    with pytest.raises(ValueError, match='channels 6..8'):
        DeviceLoader(store, 2, augment=Augment(layout=[('position', 0), ('direction', 6)]))


def test_a_frustum_store_is_refused_by_the_loader():
    from pvcnn_amd.data import DeviceLoader
    from test_data_host import GOLDEN, frustum_store
    g = torch.load(GOLDEN)['frustum']
    store = frustum_store(g, g['cases'][0])
    assert len(DeviceLoader(store, 2)) >= 1
    with pytest.raises(ValueError, match='Frustum-KITTI'):
        DeviceLoader(store, 2, augment=Augment(layout=[('position', 0)]))
    with pytest.raises(ValueError, match='Frustum-KITTI'):
        DeviceLoader(frustum_store(g, g['rgb_cases'][0], rgb=True), 2, augment=Augment())


def test_the_library_refuses_bad_arguments_before_any_launch():
    """pvcnn_augment_draw / pvcnn_augment_apply check their arguments on the host and return an error code: none of these calls reaches
    a launch, so the made-up addresses are never dereferenced."""
    from pvcnn_amd import _lib
    lib = _lib.load()
    assert {'pvcnn_augment_draw', 'pvcnn_augment_apply'} <= set(_lib.SIGNATURES)
    vp = ctypes.c_void_p
    src, dst, prm, tg, tg2, seed = 0x100000, 0x900000, 0x1100000, 0x1200000, 0x1900000, 0x2000000

    def apply(layout, c=9, n=64, b=2, src=src, dst=dst, drop=0, jit=0, seed=None, tsrc=None, tdst=None, stride=None, sigma=0.0):
        flat = (ctypes.c_int32 * 8)(*[v for pair in layout for v in pair])
        stride = c * n if stride is None else stride
        return lib.pvcnn_augment_apply(vp(src), stride, vp(tsrc), n, b, c, n, flat, len(layout), vp(prm), sigma, 0.05, jit, drop, None, None,
                                       vp(seed), vp(dst), stride, vp(tdst), n, None, None, None)

    def refused(rc, words):
        assert rc == -1 and words in lib.pvcnn_last_error_string().decode(), lib.pvcnn_last_error_string()

    refused(apply([(POSITION, 7)]), 'exceed the C channels')
    refused(apply([(POSITION, 0), (DIRECTION, 4)], c=6), 'exceed the C channels')
    refused(apply([(POSITION, 0), (DIRECTION, 2)]), 'overlap')
    refused(apply([(3, 0)]), 'role')
    refused(apply([(POSITION, 0)], dst=src, drop=1, seed=seed), 'must not alias')
    refused(apply([(POSITION, 0)], dst=src + 64, seed=seed), 'overlaps src')
    refused(apply([(POSITION, 0)], drop=1, seed=seed, tsrc=tg, tdst=tg), 'targets_dst must not alias')
    refused(apply([(POSITION, 0)], tsrc=tg, tdst=None), 'go together')
    refused(apply([(POSITION, 0)], drop=1), 'needs a device `seed`')
    refused(apply([(POSITION, 0)], jit=1, sigma=0.01), 'needs a device `seed`')
    refused(apply([(POSITION, 0)], stride=100), 'shorter than a sample')
    refused(apply([(POSITION, 0)], sigma=-1.0), 'negative')
    assert apply([(POSITION, 0)], b=0) == 0 and apply([], n=0, tsrc=tg, tdst=tg2) == 0                      # empty: no launch
    flat = (ctypes.c_int32 * 10)(*([POSITION, 0] * 5))
    refused(lib.pvcnn_augment_apply(vp(src), 576, None, 64, 2, 9, 64, flat, 5, vp(prm), 0.0, 0.0, 0, 0, None, None, None, vp(dst), 576,
                                    None, 64, None, None, None), 'at most four')

    def draw(b=4, axis=2, rot=0.0, ps=0.0, pc=0.0, flip=(0.0, 0.0, 0.0), scale=(1.0, 1.0), t=0.0, drop=0.0, seed=seed, params=prm):
        return lib.pvcnn_augment_draw(b, axis, rot, ps, pc, *flip, *scale, t, drop, vp(seed), vp(params), None)

    refused(draw(axis=3), 'axis')
    refused(draw(scale=(1.1, 0.9)), 'scale_lo <= scale_hi')
    refused(draw(flip=(0.0, 1.5, 0.0)), 'flip')
    refused(draw(drop=1.01), 'drop_max')
    refused(draw(rot=float('nan')), 'rot_max')
    refused(draw(t=-1.0), 'translate_max')
    refused(draw(seed=None), 'null pointer')
    assert draw(b=0) == 0
