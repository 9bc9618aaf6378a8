"""FPS, ball query, grouping / gather and 3-NN interpolation (csrc/fps.hip, csrc/neighbors.hip, the CSR backwards of csr.h) judged by
truths of their own (tests/neighbors_truth.py, proven on the CPU in tests/test_neighbors_truth_host.py), through HipBackend.

  exact family        dyadic lattices: torch.equal with the integer truth.  Reaches: every launch shape of fps.hip up to the 1024-thread
                      kernel (N = 1, 2, 63-65, 1025, 8193) with ties at distance 0; the no-hit row and N = 0 of ball_query; points
                      exactly ON the sphere (the strict '<'); the padding loop's stride of 64 (U = 1, 64, 65, 128); the strict-'<'
                      insertion of the 3-NN on equidistant and duplicated centres, M < 3, and the tail block of three_nn_kernel.
  certificate family  six kinds of fp32 cloud, and one on either side of each FPS launch boundary (1024 / 1025, 8192 / 8193, the
                      LDS-copy limit 12266 / 12267, 16384 / 16385: fps_global_kernel), as the chain FPS -> gather -> ball query ->
                      grouping and FPS -> 3-NN interpolate; every stage certified in fp64 (DELTA = 8u, weights 32u, their sum 8u).
  hot-spot backwards  more than 8192 entries in one target range: the list-overflow path of csr_prep_kernel for grouping_bwd,
                      gather_bwd and three_nn_interp_bwd, directly and through the autograd functions; integer sums, torch.equal.
"""
import numpy as np
import pytest
import torch

import neighbors_truth as T
import pvcnn_amd.modules.functional as PF

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _coords(clouds):
    return _d(np.stack([T.as_coords(P) for P in clouds]))


# ---- exact family

@pytest.mark.parametrize('i', range(len(T.LATTICE_FPS_CASES)), ids=[f'N{c[0]}-M{c[2]}-B{c[3]}' for c in T.LATTICE_FPS_CASES])
def test_fps_equals_the_integer_truth(hip, i):
    clouds, m = T.lattice_fps_case(i)
    got = hip.furthest_point_sampling(_coords(clouds), m)
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), torch.from_numpy(np.stack([T.fps_exact(P, m) for P in clouds])))


@pytest.mark.parametrize('i', range(len(T.LATTICE_BALL_CASES)), ids=[f'N{c[0]}-M{c[2]}-U{c[3]}-r{c[4]}' for c in T.LATTICE_BALL_CASES])
def test_ball_query_equals_the_integer_truth(hip, i):
    Ps, Cs, u, r = T.lattice_ball_case(i)
    want = np.stack([T.ball_query_exact(P, C, r * r, u) for P, C in zip(Ps, Cs)])
    got = hip.ball_query(_coords(Cs), _coords(Ps), r / T.DENOM, u)
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize('i', range(len(T.LATTICE_NN_CASES)), ids=[f'N{c[0]}-M{c[2]}' for c in T.LATTICE_NN_CASES])
def test_three_nn_equals_the_integer_truth(hip, i):
    Ps, Cs = T.lattice_nn_case(i)
    feats = np.stack([T.int_features(i * 10 + bi, 5, Cs[0].shape[1]) for bi in range(len(Ps))])
    out, idx, w = [x.cpu().numpy() for x in hip.three_nearest_neighbors_interpolate_forward(_coords(Ps), _coords(Cs), _d(feats))]
    assert np.array_equal(idx, np.stack([T.three_nn_exact(P, C) for P, C in zip(Ps, Cs)]))
    for bi, (P, C) in enumerate(zip(Ps, Cs)):       # the 1e-10 clamp at d = 0 is not dyadic: weights and outputs by the certificate bounds
        assert T.three_nn_certificate(T.as_coords(P), T.as_coords(C), idx[bi], w[bi]) == []
        value, bound = T.interp_out_bound(feats[bi], idx[bi], w[bi])
        assert (np.abs(out[bi] - value) <= bound).all()


# ---- certificate family

@pytest.mark.parametrize('i', range(len(T.CLOUD_CASES)), ids=[f'{c[0]}-{c[2]}' for c in T.CLOUD_CASES])
def test_chain_passes_the_certificates(hip, i):
    clouds, m, radius = T.cloud_case(i)
    b, n, u = len(clouds), clouds[0].shape[1], T.CLOUD_U
    p = _d(np.stack(clouds))
    picked = hip.furthest_point_sampling(p, m)
    sampled = hip.gather_features_forward(p, picked).cpu().numpy()                  # the centres as the network forms them
    picked = picked.cpu().numpy()
    for bi, c in enumerate(clouds):
        assert T.fps_certificate(c, picked[bi]) == []
        assert np.array_equal(sampled[bi], c[:, picked[bi]])
    centers = np.stack([T.centers_of(c, picked[bi], 7000 + 10 * i + bi) for bi, c in enumerate(clouds)])
    balls = hip.ball_query(_d(centers), p, radius, u)
    feats = np.stack([T.int_features(i * 10 + bi, 4, n) for bi in range(b)])
    grouped = hip.grouping_forward(_d(feats), balls).cpu().numpy()
    balls = balls.cpu().numpy()
    cfeats = np.stack([T.int_features(i * 10 + 5 + bi, 4, centers.shape[2]) for bi in range(b)])
    out, idx, w = [x.cpu().numpy() for x in hip.three_nearest_neighbors_interpolate_forward(p, _d(centers), _d(cfeats))]
    for bi, c in enumerate(clouds):
        assert T.ball_query_certificate(c, centers[bi], radius, u, balls[bi]) == []
        assert np.array_equal(grouped[bi], T.gather_exact(feats[bi], balls[bi]))
        assert T.three_nn_certificate(c, centers[bi], idx[bi], w[bi]) == []
        value, bound = T.interp_out_bound(cfeats[bi], idx[bi], w[bi])
        assert (np.abs(out[bi] - value) <= bound).all()


# ---- hot-spot backwards

def _hot_weights(case):
    return (case['w_num'] / T.HOT_W_DENOM).astype(np.float32)


@pytest.mark.parametrize('name', T.HOT_CASES)
def test_hot_spot_backward_equals_the_integer_truth(hip, oracle, name):
    case = T.hot_case(name)
    g, idx, n = torch.from_numpy(case['g']), torch.from_numpy(case['idx']), case['n']
    if case['op'] == 'grouping':
        got, ref = hip.grouping_backward(g.to(DEV), idx.to(DEV), n), oracle.grouping_backward(g, idx, n)
    elif case['op'] == 'gather':
        got, ref = hip.gather_features_backward(g.to(DEV), idx.to(DEV), n), oracle.gather_features_backward(g, idx, n)
    else:
        w = torch.from_numpy(_hot_weights(case))
        got = hip.three_nearest_neighbors_interpolate_backward(g.to(DEV), idx.to(DEV), w.to(DEV), n)
        ref = oracle.three_nearest_neighbors_interpolate_backward(g, idx, w, n)
    assert torch.equal(got.cpu(), torch.from_numpy(T.hot_truth(case)))
    assert torch.equal(got.cpu(), ref)


@pytest.mark.parametrize('name', T.HOT_CASES)
def test_hot_spot_backward_through_autograd(hip, name):
    case = T.hot_case(name)
    g, n = _d(case['g']), case['n']
    if case['op'] == 'interp':
        P, C = T.interp_hot_geometry(case['g'].shape[2])
        f = _d(np.stack([T.int_features(bi, 3, 3) for bi in range(2)])).requires_grad_()
        out = PF.nearest_neighbor_interpolate(_coords(P), _coords(C), f)
        idx = np.stack([T.three_nn_exact(P[bi], C[bi]) for bi in range(2)])
        w_num = np.broadcast_to(np.array([2, 1, 1])[None, :, None], idx.shape)
        fi = f.detach().cpu().numpy().astype(np.int64)
        want_out = np.stack([T.interp_exact(fi[bi], idx[bi], w_num[bi]) for bi in range(2)]) / T.HOT_W_DENOM
        want = T.hot_truth(dict(op='interp', g=case['g'], idx=idx, w_num=w_num, n=3))
    else:
        f = _d(np.stack([T.int_features(bi, 3, n) for bi in range(2)])).requires_grad_()
        out = (PF.grouping if case['op'] == 'grouping' else PF.gather)(f, _d(case['idx']))
        fi = f.detach().cpu().numpy()
        want_out = np.stack([T.gather_exact(fi[bi], case['idx'][bi]) for bi in range(2)])
        want = T.hot_truth(case)
    assert torch.equal(out.detach().cpu(), torch.from_numpy(want_out.astype(np.float32)))
    out.backward(g)
    assert torch.equal(f.grad.cpu(), torch.from_numpy(want))
