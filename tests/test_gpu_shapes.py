"""Shapes on the device (csrc/shapes.hip) on the GPU: neighbour tables against the numpy truth with zero tolerance, normals against the
solver-independent inequalities of tests/shapes_truth.py on every point, and the layers above them -- `from_clouds`, `segment_shape`,
a captured graph -- against the same work composed by hand.

The bound of the normals is derived, not tuned (shapes_truth.epsilon): 8 (k + 4) 2^-24 of the trace.  A numpy fp32 restatement
(two-pass covariance, Jacobi) stays below 0.6 % of it on these clouds; the kernel accumulates in fp64."""
import functools

import numpy as np
import pytest
import torch

import shapes_truth as T
from conftest import SEED
from test_shapes_host import RAGGED, check_from_clouds, ragged_pack

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- neighbour tables: equality ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 8, 16, 64])
def test_lattice_cloud_ties_and_duplicates(hip, k):
    from pvcnn_amd import shapes
    x = T.lattice_cloud(11)
    got = shapes.k_nearest(dev(x), k)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (900, k)
    assert np.array_equal(got.cpu().numpy(), T.k_nearest_definition(x, T.offsets_of([900]), k))


@functools.lru_cache(maxsize=None)
def ragged_truth():
    rows, offsets = ragged_pack(3)
    return T.k_nearest_definition(rows, offsets, 16)


@pytest.mark.parametrize('ld', [3, 7])
def test_ragged_pack_in_one_call(hip, ld):
    from pvcnn_amd import shapes
    rows, offsets = ragged_pack(ld)
    if ld == 7:                                                    # the same xyz in a wider row: the same table
        rows[:, :3] = ragged_pack(3)[0]
    got = shapes.k_nearest(dev(rows), 16, offsets=offsets).cpu().numpy()
    assert np.array_equal(got, ragged_truth())
    for n, a, b in zip(RAGGED, offsets[:-1], offsets[1:]):
        assert (got[a:b, min(16, n):] == -1).all() and (got[a:b, :min(16, n)] >= 0).all() and got[a:b].max() < n
    if ld == 7:                                                    # numpy in, offsets as a device tensor, a column slice of the store
        again = shapes.k_nearest(dev(rows)[:, :5], 16, offsets=dev(offsets)).cpu().numpy()
        assert np.array_equal(again, got)


def random_clouds():
    rng = np.random.RandomState(SEED % 1000 + 1)
    u = rng.randn(2000, 3)
    return {'sphere': (u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32),
            'cube': (rng.rand(1500, 3) * 2 - 1).astype(np.float32),
            'offset': (1 + 0.01 * rng.rand(1500, 3)).astype(np.float32)}


@pytest.mark.parametrize('k', [8, 30])
@pytest.mark.parametrize('name', ['sphere', 'cube', 'offset'])
def test_random_clouds(hip, name, k):
    from pvcnn_amd import shapes
    x = random_clouds()[name]
    got = shapes.k_nearest(x, k).cpu().numpy()                     # numpy in: uploaded once
    assert np.array_equal(got, T.k_nearest_definition(x, T.offsets_of([x.shape[0]]), k))
    assert np.array_equal(got[:, 0], np.arange(x.shape[0]))        # distinct points: the query comes first


def test_large_cloud_sampled_queries(hip):
    from pvcnn_amd import shapes
    rng = np.random.RandomState(SEED % 1000 + 2)
    x = (rng.rand(20011, 3) * [4, 2, 1]).astype(np.float32)
    queries = np.sort(rng.choice(20011, size=2048, replace=False))
    got = shapes.k_nearest(dev(x), 30).cpu().numpy()
    assert got.min() >= 0 and got.max() < 20011
    assert np.array_equal(got[queries], T.k_nearest_rows(x, queries, 30))


# ---- normals: the inequalities, on every point ---------------------------------------------------------------------------------
OUTWARD = ('sphere', 'uniform_cube', 'box_surface', 'far_from_origin')
PLANES = ('plane_z0', 'plane_tilted_noisy')          # their centroid lies in the plane: "outward" is ambiguous, a viewpoint is not
VIEW = np.float32([[0.3, -0.2, 4.0], [10.0, 20.0, 30.0]])


@functools.lru_cache(maxsize=None)
def normals_of(k):
    """One pack per orientation and k, shared by the cases: name -> (cloud, table, normals, curvature, mode, ref)."""
    from pvcnn_amd import shapes
    cases = T.normal_cases(SEED % 1000)
    out = {}
    for names, orient in ((OUTWARD, 'outward'), (PLANES, 'viewpoint')):
        rows = np.concatenate([cases[n] for n in names])
        offsets = T.offsets_of([cases[n].shape[0] for n in names])
        d = dev(rows)
        view = VIEW if orient == 'viewpoint' else None
        normals, curvature = shapes.estimate_normals(d, k=k, offsets=offsets, orient=orient, viewpoint=view, return_curvature=True)
        knn = shapes.k_nearest(d, k, offsets=offsets).cpu().numpy()
        ref = VIEW if orient == 'viewpoint' else T.centroids(rows, offsets)
        if orient == 'outward':                                    # the centroid launch against the truth
            got = shapes._seam._backend.cloud_centroids(d, dev(offsets)).cpu().numpy()
            assert np.abs(got.astype(np.float64) - ref).max() <= 2.0 ** -23 * np.abs(ref).max()       # one ulp: the fp64 sums differ in order
            ref = got
        normals, curvature = normals.cpu().numpy(), curvature.cpu().numpy()
        for i, n in enumerate(names):
            a, b = offsets[i], offsets[i + 1]
            out[n] = (cases[n], knn[a:b], normals[a:b], curvature[a:b], shapes._MODES[orient], ref[i])
    return out


@pytest.mark.parametrize('k', [8, 16, 30])
@pytest.mark.parametrize('name', OUTWARD + PLANES)
def test_normals_meet_the_inequalities(hip, name, k):
    x, knn, normals, curvature, mode, ref = normals_of(k)[name]
    offsets = T.offsets_of([x.shape[0]])
    assert np.array_equal(knn, T.k_nearest_definition(x, offsets, k))
    worst = T.check_normals(x, offsets, knn, normals, curvature, mode=mode, ref=ref)
    print(name, k, worst)
    if name == 'plane_z0':
        assert (normals[:, 2] >= 1 - 1e-6).all()
    if name == 'sphere':                                           # outward on a sphere: along the radius
        assert (np.einsum('ni,ni->n', normals, x) > 0.8).all()


def test_lattice_plane_has_the_exact_normal(hip):
    """z constant on a lattice: the covariance has an exact zero eigenvalue and exact zero couplings to z."""
    from pvcnn_amd import shapes
    rng = np.random.RandomState(SEED % 1000 + 3)
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), indexing='ij'), -1).reshape(-1, 2)[rng.permutation(256)]
    x = np.c_[g / 16.0, np.full(256, 0.5)].astype(np.float32)
    offsets = T.offsets_of([256])
    view = np.float32([0.5, 0.5, -5.0])
    normals, curvature = shapes.estimate_normals(dev(x), k=16, orient='viewpoint', viewpoint=view, return_curvature=True)
    knn = shapes.k_nearest(dev(x), 16).cpu().numpy()
    T.check_normals(x, offsets, knn, normals.cpu().numpy(), curvature.cpu().numpy(), mode=2, ref=view)
    assert (normals[:, 2].abs() >= 1 - 1e-6).all() and (normals[:, 2] < 0).all()
    assert (curvature == 0).all()


def test_degenerate_clouds_get_zero_normals(hip):
    from pvcnn_amd import shapes
    rows = np.concatenate([np.tile(np.float32([[0.3, -0.2, 0.9]]), (40, 1)), np.float32([[1, 2, 3]]), np.float32([[0, 0, 0], [1, 0, 0]])])
    offsets = T.offsets_of([40, 1, 2])
    for orient in ('outward', None):
        normals, curvature = shapes.estimate_normals(dev(rows), k=16, offsets=offsets, orient=orient, return_curvature=True)
        assert (normals == 0).all() and (curvature == 0).all()
    knn = shapes.k_nearest(dev(rows), 16, offsets=offsets).cpu().numpy()
    assert np.array_equal(knn, T.k_nearest_definition(rows, offsets, 16))
    T.check_normals(rows, offsets, knn, normals.cpu().numpy(), curvature.cpu().numpy())


# ---- composition ---------------------------------------------------------------------------------------------------------------
def test_from_clouds_equals_the_constructor(hip):
    store = check_from_clouds(DEV)
    assert store.rows.is_cuda


def test_segment_shape_equals_the_composition_by_hand(hip):
    from pvcnn_amd import evaluate, shapes
    torch.manual_seed(SEED)
    model = torch.nn.Conv1d(22, 50, 1).to(DEV).eval()
    rng = np.random.RandomState(SEED % 1000 + 4)
    xyz = (rng.rand(3000, 3) * [2, 1, 1] + [4, 0, -1]).astype(np.float32)
    shape_id = 3
    predictions, votes = shapes.segment_shape(model, xyz, shape_id, k=8, rng=np.random.RandomState(5))
    start, end = shapes.shape_part_classes(shape_id)
    assert (start, end) == (votes.start_class, votes.end_class) == (8, 12)
    assert predictions.dtype == torch.int64 and predictions.is_cuda and tuple(predictions.shape) == (3000,)
    assert predictions.min().item() >= start and predictions.max().item() < end        # none is -1: every point was voted
    rows = shapes.prepare_shape(xyz, k=8)
    hot = torch.zeros((16, 3000), device=DEV)
    hot[shape_id] = 1.0
    by_hand = evaluate.ShapeVotes(3000, DEV, start, end)
    evaluate.shapenet_shape_votes(model, torch.cat([rows.t(), hot]).contiguous(), by_hand, rng=np.random.RandomState(5))
    assert torch.equal(predictions, by_hand.predictions()) and torch.equal(votes.confidences(), by_hand.confidences())
    given, _ = shapes.segment_shape(model, xyz, shape_id, normals=rows[:, 3:], rng=np.random.RandomState(5))
    assert torch.equal(given, predictions)
    with pytest.raises(TypeError):
        shapes.segment_shape(model, xyz, shape_id, normals=rows[:, 3:], k=8)


def test_the_two_launches_replay_in_a_graph(hip):
    """k_nearest + (centroids) + shape_normals captured on static buffers, one stream; replayed on new contents == eager."""
    be = hip
    rng = np.random.RandomState(SEED % 1000 + 5)
    sizes = [300, 5, 1200, 64]
    offsets = dev(T.offsets_of(sizes))
    first, second = ((rng.rand(sum(sizes), 3) * 2 - 1).astype(np.float32) for _ in range(2))
    rows = dev(first)
    knn = torch.empty((sum(sizes), 16), dtype=torch.int32, device=DEV)
    ref = torch.empty((len(sizes), 3), device=DEV)
    normals = torch.empty((sum(sizes), 3), device=DEV)
    curvature = torch.empty((sum(sizes),), device=DEV)

    def run():
        be.k_nearest(rows, offsets, 16, out=knn)
        be.cloud_centroids(rows, offsets, out=ref)
        be.shape_normals(rows, offsets, knn, ref, 1, out=normals, out_curvature=curvature)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    rows.copy_(dev(second))
    for t in (knn, ref, normals, curvature):
        t.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    fresh = dev(second)
    e_knn = be.k_nearest(fresh, offsets, 16)
    e_normals, e_curvature = be.shape_normals(fresh, offsets, e_knn, be.cloud_centroids(fresh, offsets), 1, want_curvature=True)
    assert torch.equal(knn, e_knn) and torch.equal(normals, e_normals) and torch.equal(curvature, e_curvature)
    assert np.array_equal(knn.cpu().numpy(), T.k_nearest_definition(second, T.offsets_of(sizes), 16))


def test_the_backend_refuses_malformed_arguments(hip):
    """Every argument message of the three backend methods, tripped once (they are checked before anything is launched)."""
    be = hip
    rows, offsets = torch.rand(20, 3, device=DEV), dev(T.offsets_of([20]))
    knn = be.k_nearest(rows, offsets, 4)
    ref = be.cloud_centroids(rows, offsets)
    for call, message in (
            (lambda: be.k_nearest(rows[:, :2], offsets, 4), 'rows'),
            (lambda: be.k_nearest(rows.t().contiguous().t(), offsets, 4), 'rows'),
            (lambda: be.k_nearest(rows.double(), offsets, 4), 'rows'),
            (lambda: be.k_nearest(rows, offsets.int(), 4), 'offsets'),
            (lambda: be.cloud_centroids(rows, offsets.cpu().to(DEV).view(1, 2)), 'offsets'),
            (lambda: be.k_nearest(rows, offsets, 0), r'k in \[1, 64\]'),
            (lambda: be.k_nearest(rows, offsets, 65), r'k in \[1, 64\]'),
            (lambda: be.k_nearest(rows, offsets, 4, out=torch.empty((20, 5), dtype=torch.int32, device=DEV)), 'out='),
            (lambda: be.k_nearest(rows, offsets, 4, out=torch.empty((20, 4), dtype=torch.int64, device=DEV)), 'out='),
            (lambda: be.shape_normals(rows, offsets, knn[:10].contiguous()), 'knn'),
            (lambda: be.shape_normals(rows, offsets, knn, mode=3), 'mode'),
            (lambda: be.shape_normals(rows, offsets, knn, None, 1), 'needs ref'),
            (lambda: be.shape_normals(rows, offsets, knn, ref[:, :2].contiguous(), 2), 'ref'),
            (lambda: be.shape_normals(rows, offsets, knn, ref, 1, out=torch.empty((20, 4), device=DEV)), 'out='),
            (lambda: be.cloud_centroids(rows, offsets, out=torch.empty((2, 3), device=DEV)), 'out=')):
        with pytest.raises(RuntimeError, match=message):
            call()
    normals, curvature = be.shape_normals(rows, offsets, knn, ref, 2)          # and the well-formed call still runs
    assert curvature is None and tuple(normals.shape) == (20, 3)


def test_non_finite_coordinates_stay_in_bounds(hip):
    """Finite coordinates are the contract; with others the result is unspecified, but every index lies in [-1, n) and a clean cloud in
    the same pack is untouched.  (A NaN distance is never inserted; queries with finite coordinates still get their finite neighbours.)"""
    from pvcnn_amd import shapes
    rng = np.random.RandomState(SEED % 1000 + 6)
    bad = (rng.rand(500, 3) * 2 - 1).astype(np.float32)
    hit = rng.choice(500, size=45, replace=False)
    bad[hit, rng.randint(0, 3, size=45)] = np.tile(np.float32([np.nan, np.inf, -np.inf]), 15)
    clean = (rng.rand(130, 3) * 2 - 1).astype(np.float32)
    rows, offsets = np.concatenate([bad, clean]), T.offsets_of([500, 130])
    got = shapes.k_nearest(dev(rows), 16, offsets=offsets).cpu().numpy()
    assert got[:500].min() >= -1 and got[:500].max() < 500
    finite = np.isfinite(bad).all(1)
    with np.errstate(all='ignore'):
        want = T.k_nearest_definition(rows, offsets, 16)           # (numpy sorts NaN last: a finite query's 16 nearest are finite)
    assert np.array_equal(got[:500][finite], want[:500][finite]) and np.array_equal(got[500:], want[500:])
    normals, curvature = shapes.estimate_normals(dev(rows), k=16, offsets=offsets, return_curvature=True)
    T.check_normals(clean, T.offsets_of([130]), got[500:], normals[500:].cpu().numpy(), curvature[500:].cpu().numpy(), mode=1,
                    ref=T.centroids(clean, T.offsets_of([130])))
