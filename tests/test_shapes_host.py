"""Shapes on the device, host side: the numpy truth against itself, the torch formulation (what CPU tensors take) against the truth --
neighbour tables bit for bit, normals by the solver-independent inequalities --, the argument checks, `from_clouds` against the
constructor, and the three new symbols in the ABI.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import shapes_truth as T
from conftest import ROOT, SEED

RAGGED = [1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 2947]      # around k = 16, the kernel's 64-candidate tile, 4 tiles, many


def ragged_pack(ld, seed=SEED):
    rng = np.random.RandomState(seed % (2 ** 31))
    rows = (rng.rand(sum(RAGGED), ld) * 2 - 1).astype(np.float32)
    return rows, T.offsets_of(RAGGED)


def test_truth_lattice_facts_and_fast_truth():
    """The lattice cloud is what the tie rule is tested on: most queries have a tie across the k = 16 boundary, dozens of points are
    duplicates.  The selection-based truth (used for the large cloud) equals the literal definition."""
    x = T.lattice_cloud(11)
    d = np.sort(T.sq_distances(x, x), axis=1)
    assert (d[:, 15] == d[:, 16]).mean() > 0.7
    assert 900 - len(np.unique(x, axis=0)) >= 50
    exact = ((x[:, None, :].astype(np.float64) - x[None, :, :]) ** 2).sum(-1)
    assert np.array_equal(T.sq_distances(x, x).astype(np.float64), exact)                 # every operation exact
    for k in (1, 16, 64):
        want = T.k_nearest_definition(x, T.offsets_of([900]), k)
        assert np.array_equal(T.k_nearest_rows(x, np.arange(900), k), want)
        assert (want[:, 0] <= np.arange(900)).all()                                       # d = 0: the query or an earlier duplicate
    rows, offsets = ragged_pack(3)
    want = T.k_nearest_definition(rows, offsets, 16)
    a, b = offsets[-2], offsets[-1]
    assert np.array_equal(T.k_nearest_rows(rows[a:b], np.arange(b - a), 16), want[a:b])


@pytest.mark.parametrize('k', [1, 8, 16, 64])
def test_cpu_tensors_lattice(k):
    from pvcnn_amd import shapes
    x = T.lattice_cloud(11)
    got = shapes.k_nearest(torch.from_numpy(x), k)
    assert got.dtype == torch.int32 and got.device.type == 'cpu'
    assert np.array_equal(got.numpy(), T.k_nearest_definition(x, T.offsets_of([900]), k))


@pytest.mark.parametrize('ld', [3, 7])
def test_cpu_tensors_ragged_pack(ld):
    from pvcnn_amd import shapes
    rows, offsets = ragged_pack(ld)
    got = shapes.k_nearest(torch.from_numpy(rows), 16, offsets=offsets).numpy()
    assert np.array_equal(got, T.k_nearest_definition(rows, offsets, 16))
    for a, b in zip(offsets[:-1], offsets[1:]):
        assert (got[a:b, min(16, b - a):] == -1).all() and got[a:b].max() < b - a          # -1 tails, positions inside the cloud
    wide = torch.from_numpy(np.concatenate([rows, rows[:, :2]], axis=1))[:, :ld]            # a column slice of a wider store
    assert np.array_equal(shapes.k_nearest(wide, 16, offsets=torch.from_numpy(offsets)).numpy(), got)


@pytest.mark.parametrize('name,orient', [('sphere', 'outward'), ('plane_z0', 'viewpoint'), ('far_from_origin', None)])
def test_cpu_normals_meet_the_inequalities(name, orient):
    from pvcnn_amd import shapes
    x = T.normal_cases(SEED % 1000)[name]
    offsets = T.offsets_of([x.shape[0]])
    view = np.array([0.2, -0.1, 3.0], dtype=np.float32)
    normals, curvature = shapes.estimate_normals(torch.from_numpy(x), k=16, orient=orient, viewpoint=view if orient == 'viewpoint' else None,
                                                 return_curvature=True)
    knn = shapes.k_nearest(torch.from_numpy(x), 16).numpy()
    ref = {'outward': T.centroids(x, offsets), 'viewpoint': view, None: None}[orient]
    T.check_normals(x, offsets, knn, normals.numpy(), curvature.numpy(), mode=shapes._MODES[orient], ref=ref)
    if name == 'plane_z0':
        assert (normals[:, 2] >= 1 - 1e-6).all()                                           # towards a viewpoint above the plane


def test_cpu_degenerate_clouds_get_zero_normals():
    from pvcnn_amd import shapes
    rows = np.concatenate([np.tile(np.float32([[0.3, -0.2, 0.9]]), (40, 1)), np.float32([[1, 2, 3]]), np.float32([[0, 0, 0], [1, 0, 0]])])
    offsets = T.offsets_of([40, 1, 2])
    normals, curvature = shapes.estimate_normals(torch.from_numpy(rows), k=16, offsets=offsets, return_curvature=True)
    assert (normals == 0).all() and (curvature == 0).all()
    T.check_normals(rows, offsets, shapes.k_nearest(torch.from_numpy(rows), 16, offsets=offsets).numpy(), normals.numpy(), curvature.numpy())


def test_arguments_are_checked():
    from pvcnn_amd import shapes
    x = torch.rand(50, 3)
    for k in (0, 65, -1):
        with pytest.raises(ValueError, match='k in'):
            shapes.k_nearest(x, k)
        with pytest.raises(ValueError, match='k in'):
            shapes.estimate_normals(x, k=k)
    with pytest.raises(ValueError, match='max_cloud_points'):
        shapes.estimate_normals(x, k=8, max_cloud_points=49)
    shapes.estimate_normals(x, k=8, max_cloud_points=50)
    for bad in ([0, 20], [1, 50], [0, 20, 20, 50], [0, 30, 20, 50]):
        with pytest.raises(ValueError, match='offsets'):
            shapes.k_nearest(x, 4, offsets=bad)
    with pytest.raises(ValueError, match='orient'):
        shapes.estimate_normals(x, orient='inward')
    with pytest.raises(ValueError, match='viewpoint'):
        shapes.estimate_normals(x, orient='viewpoint')
    with pytest.raises(ValueError, match='viewpoint'):
        shapes.estimate_normals(x, orient='outward', viewpoint=[0, 0, 1])
    with pytest.raises(ValueError, match='points'):
        shapes.k_nearest(torch.rand(50, 2), 4)
    assert shapes.shape_part_classes(0) == (0, 4) and shapes.shape_part_classes(15) == (47, 50)


def test_prepare_shape_normalises_as_the_store_does():
    from pvcnn_amd import shapes
    from pvcnn_amd.data import DeviceShapeNet
    rng = np.random.RandomState(3)
    xyz = (rng.rand(300, 3) * [3, 1, 2] + [5, -2, 0.5]).astype(np.float32)
    rows = shapes.prepare_shape(xyz, k=8)                                                   # numpy in: on the GPU where there is one
    assert tuple(rows.shape) == (300, 6) and rows.dtype == torch.float32
    assert np.array_equal(rows[:, :3].cpu().numpy(), DeviceShapeNet.normalize_point_cloud(xyz))    # the reference's fp32 arithmetic
    assert torch.equal(rows[:, 3:], shapes.estimate_normals(rows[:, :3].contiguous(), k=8))  # (the same device: the same path)
    t = shapes.prepare_shape(torch.from_numpy(xyz), k=8)                                    # a tensor: fp64, rounded once
    x = xyz.astype(np.float64)
    x = x - x.mean(0)
    want = x / np.linalg.norm(x, axis=1).max()
    assert np.abs(t[:, :3].numpy() - want).max() <= 2.0 ** -24
    raw = shapes.prepare_shape(xyz, k=8, normalize=False).cpu()
    assert np.array_equal(raw[:, :3].numpy(), xyz)


def _split(seed=5):
    rng = np.random.RandomState(seed)
    sizes = [40, 7, 130, 2, 64]
    clouds = [(rng.rand(n, 3) * [2, 1, 0.5] + [1, 0, -3]).astype(np.float32) for n in sizes]
    labels = [rng.randint(0, 50, size=n) for n in sizes]
    return clouds, labels, [3, 0, 15, 7, 3]


def check_from_clouds(device):
    """from_clouds == the constructor on [xyz, estimate_normals(normalised xyz), label]: every table bit for bit, and one batch."""
    from pvcnn_amd import shapes
    from pvcnn_amd.data import DeviceShapeNet
    clouds, labels, shape_ids = _split()
    got = DeviceShapeNet.from_clouds(clouds, labels, shape_ids, 32, k=8, device=device)
    full = []
    for cloud, label in zip(clouds, labels):
        coords = torch.from_numpy(DeviceShapeNet.normalize_point_cloud(cloud)).to(device)
        normals = shapes.estimate_normals(coords, k=8).cpu().numpy()
        full.append(np.concatenate([cloud, normals, label[:, None].astype(np.float32)], axis=1))
    want = DeviceShapeNet(full, shape_ids, 32, device=device)
    for name in ('rows', 'labels', 'offsets', 'shape_ids'):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.device == b.device and torch.equal(a, b), name
    assert (got.rows[:, 3:6].abs().sum(1) > 0).sum().item() >= 40 + 7 + 130 + 64 - 8        # normals are there (cloud of 2: zeros)
    assert (got.num_points, got.with_normal, got.with_one_hot_shape_id, got.normalize, got.jitter, got.max_n) == \
           (want.num_points, want.with_normal, want.with_one_hot_shape_id, want.normalize, want.jitter, want.max_n)
    rng = np.random.RandomState(9)
    idx = [4, 0, 2, 1]
    choices = torch.from_numpy(rng.randint(0, 200, size=(4, 32)).astype(np.int32))
    jitter = torch.from_numpy(rng.randn(4, 3, 32))
    assemble = (lambda s: s.assemble(idx, choices=choices, jitter=jitter)) if torch.device(device).type == 'cuda' else \
               (lambda s: s.assemble_reference(idx, choices=choices, jitter=jitter))
    a, b = assemble(got), assemble(want)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and tuple(a[0].shape) == (4, 22, 32)
    plain = DeviceShapeNet.from_clouds(clouds, labels, shape_ids, 32, with_normal=False, normalize=False, jitter=False, device=device)
    assert (plain.rows[:, 3:6] == 0).all() and torch.equal(plain.rows[:, :3].cpu(), torch.from_numpy(np.concatenate(clouds)))
    return got


def test_from_clouds_equals_the_constructor_on_the_cpu():
    from pvcnn_amd.data import DeviceShapeNet
    check_from_clouds('cpu')
    clouds, labels, shape_ids = _split()
    with pytest.raises(ValueError, match=r'\(n, 3\)'):
        DeviceShapeNet.from_clouds([np.zeros((5, 7))], [np.zeros(5)], [0], 16, device='cpu')
    with pytest.raises(ValueError, match='one label array per cloud'):
        DeviceShapeNet.from_clouds(clouds, labels[:-1], shape_ids, 16, device='cpu')
    with pytest.raises(ValueError, match='k in'):
        DeviceShapeNet.from_clouds(clouds, labels, shape_ids, 16, k=65, device='cpu')


def test_abi_has_the_shape_entry_points_and_keeps_its_version():
    """An additive group: three new symbols, declared, bound and exported; the version does not move."""
    from pvcnn_amd import _lib
    from pvcnn_amd.modules.functional.backend import HipBackend
    header = open(os.path.join(ROOT, 'include', 'pvcnn_hip.h')).read()
    names = ('pvcnn_k_nearest', 'pvcnn_shape_normals', 'pvcnn_cloud_centroids')
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        assert re.search(r'PVCNN_API\s+int\s+' + name + r'\s*\(', header) and name in _lib.SIGNATURES and hasattr(lib, name)
    assert re.search(r'#define\s+PVCNN_K_NEAREST_MAX_K\s+64\b', header)
    assert _lib.load().pvcnn_version() == _lib.ABI_VERSION
    assert HipBackend.has_shapes and HipBackend.K_NEAREST_MAX_K == 64
    # arguments the library refuses before any launch (no device is touched)
    lib = _lib.load()
    vp = ctypes.c_void_p
    assert lib.pvcnn_k_nearest(vp(16), 4, 3, vp(16), 1, 65, vp(16), None) == -1
    assert lib.pvcnn_k_nearest(vp(16), 4, 2, vp(16), 1, 8, vp(16), None) == -1
    assert lib.pvcnn_k_nearest(vp(16), 2 ** 31, 3, vp(16), 1, 8, vp(16), None) == -1
    assert lib.pvcnn_shape_normals(vp(16), 4, 3, vp(16), 1, vp(16), 8, None, 1, vp(16), None, None) == -1     # oriented, no ref
    assert lib.pvcnn_k_nearest(None, 0, 3, None, 0, 8, None, None) == 0                                         # no rows: no launch


def test_the_product_path_has_no_cpu_fallback():
    from pvcnn_amd.modules.functional.backend import HipBackend
    be = HipBackend()
    rows, offsets = torch.rand(10, 3), torch.tensor([0, 10])
    with pytest.raises(RuntimeError, match='CUDA'):
        be.k_nearest(rows, offsets, 4)
    with pytest.raises(RuntimeError, match='CUDA'):
        be.shape_normals(rows, offsets, torch.zeros(10, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='CUDA'):
        be.cloud_centroids(rows, offsets)


def test_the_new_kernels_use_no_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources as kr
    if not os.path.exists(kr.DEFAULT_LIB) or not os.path.exists(kr.READELF):
        pytest.skip('libpvcnn_hip.so / llvm-readelf not present')
    table = kr.kernels()
    for family in ('k_nearest_kernel', 'shape_normals_kernel', 'cloud_centroids_kernel'):
        mine = {k: v for k, v in table.items() if family in k}
        assert mine, family
        assert all(v['vgpr_spill_count'] == 0 and v['scratch_bytes'] == 0 for v in mine.values()), mine
