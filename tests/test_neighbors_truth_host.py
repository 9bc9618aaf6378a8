"""The judges of tests/test_gpu_neighbors_exact.py, proven before they judge (no GPU): on every lattice case of the GPU file the exact
truths of neighbors_truth.py equal the CPU oracle; on every fp32 case the certificates accept the oracle's answers with ZERO complaints
(a condition, not a tolerance); and every planted fault is rejected."""
import numpy as np
import pytest
import torch

import neighbors_truth as T


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _coords(clouds):
    """list of (3, N) integer numerators -> (B, 3, N) fp32 tensor of the coordinates numerator / 8."""
    return _t(np.stack([T.as_coords(P) for P in clouds]))


# ---- exact truths == the oracle

@pytest.mark.parametrize('i', range(len(T.LATTICE_FPS_CASES)))
def test_fps_truth_is_the_oracle(oracle, i):
    clouds, m = T.lattice_fps_case(i)
    want = np.stack([T.fps_exact(P, m) for P in clouds])
    assert np.array_equal(oracle.furthest_point_sampling(_coords(clouds), m).numpy(), want)
    for P, row in zip(clouds, want):
        distinct = len(np.unique(P, axis=1).T)
        if m > distinct:   # the lattice is exhausted: every later step is a tie at distance 0 between ALL points, and point 0 wins it
            assert len(set(row[:distinct].tolist())) == distinct and (row[distinct:] == 0).all()


@pytest.mark.parametrize('i', range(len(T.LATTICE_BALL_CASES)))
def test_ball_query_truth_is_the_oracle(oracle, i):
    Ps, Cs, u, r = T.lattice_ball_case(i)
    want = np.stack([T.ball_query_exact(P, C, r * r, u) for P, C in zip(Ps, Cs)])
    got = oracle.ball_query(_coords(Cs), _coords(Ps), r / T.DENOM, u).numpy()
    assert np.array_equal(got, want)


def test_lattice_ball_cases_decide_the_strict_less_and_the_empty_row():
    on_sphere = no_hit = padded = full = decisive = 0
    for i in range(len(T.LATTICE_BALL_CASES)):
        Ps, Cs, u, r = T.lattice_ball_case(i)
        for P, C in zip(Ps, Cs):
            d = T.sq_dist_int(P, C)
            strict = T.ball_query_exact(P, C, r * r, u)
            if r > 0 and P.shape[1]:
                on_sphere += int((d == r * r).sum())
                decisive += not np.array_equal(strict, T.ball_query_exact(P, C, r * r + 1, u))      # '<=' would answer differently
            hits = (d < r * r).sum(axis=1)
            no_hit += int((hits == 0).sum())
            padded += int(((hits > 0) & (hits < u)).sum())
            full += int((hits >= u).sum())
    assert on_sphere >= 20 and decisive >= 5 and no_hit >= 3 and padded >= 3 and full >= 3, (on_sphere, decisive, no_hit, padded, full)


@pytest.mark.parametrize('i', range(len(T.LATTICE_NN_CASES)))
def test_three_nn_truth_is_the_oracle(oracle, i):
    Ps, Cs = T.lattice_nn_case(i)
    m = Cs[0].shape[1]
    feats = np.stack([T.int_features(i * 10 + bi, 5, m) for bi in range(len(Ps))])
    out, idx, w = [x.numpy() for x in oracle.three_nearest_neighbors_interpolate_forward(_coords(Ps), _coords(Cs), _t(feats))]
    for bi, (P, C) in enumerate(zip(Ps, Cs)):
        assert np.array_equal(idx[bi], T.three_nn_exact(P, C))
        assert T.three_nn_certificate(T.as_coords(P), T.as_coords(C), idx[bi], w[bi]) == []
        value, bound = T.interp_out_bound(feats[bi], idx[bi], w[bi])
        assert (np.abs(out[bi] - value) <= bound).all()
        if m >= 3:
            d = np.sort(T.sq_dist_int(P, C).T, axis=1)
            assert (d[:, 1:] == d[:, :-1]).any(), 'the case has equidistant centres'


def test_three_nn_tie_goes_to_the_smaller_index():
    P = np.array([[0], [0], [0]])
    C = np.array([[2, -2, 0, 0, 2], [0, 0, 2, -2, 0], [0, 0, 0, 0, 0]])          # five centres at distance 2, the last a duplicate
    assert T.three_nn_exact(P, C)[:, 0].tolist() == [0, 1, 2]
    assert T.three_nn_exact(P, C[:, :2])[:, 0].tolist() == [0, 1, 0] and T.three_nn_exact(P, C[:, :1])[:, 0].tolist() == [0, 0, 0]


def test_fps_tie_rule_is_k_mod_512_then_k():
    P = np.zeros((3, 1100), dtype=np.int64)
    P[0, [5, 517, 600, 1029]] = 7                                                # four equidistant candidates: k mod 512 = 5, 5, 88, 5
    assert T.fps_exact(P, 2).tolist() == [0, 5]
    P[0, 5] = 0
    assert T.fps_exact(P, 2).tolist() == [0, 517]
    P[0, [517, 1029]] = 0
    P[0, 513] = 7                                                                # k mod 512 = 1 beats 88 although 513 > 600 is false
    assert T.fps_exact(P, 2).tolist() == [0, 513]


@pytest.mark.parametrize('name', T.HOT_CASES)
def test_scatter_truths_are_the_oracle(oracle, name):
    case = T.hot_case(name)
    g, idx = _t(case['g']), _t(case['idx'])
    if case['op'] == 'grouping':
        got = oracle.grouping_backward(g, idx, case['n'])
    elif case['op'] == 'gather':
        got = oracle.gather_features_backward(g, idx, case['n'])
    else:
        got = oracle.three_nearest_neighbors_interpolate_backward(g, idx, _t((case['w_num'] / T.HOT_W_DENOM).astype(np.float32)), case['n'])
    assert np.array_equal(got.numpy(), T.hot_truth(case))
    counts = np.stack([np.bincount(row.reshape(-1), minlength=case['n']) for row in case['idx']])
    assert counts.sum(axis=1).min() > 8192, 'more entries than the in-LDS list of csr_prep_kernel holds, all in one range'


def test_forward_gather_truths_are_the_oracle(oracle):
    f = np.stack([T.int_features(bi, 3, 64) for bi in range(2)])
    for name in ('grouping_same_32', 'gather_two_targets'):
        idx = T.hot_case(name)['idx']
        fwd = oracle.grouping_forward if idx.ndim == 3 else oracle.gather_features_forward
        assert np.array_equal(fwd(_t(f), _t(idx)).numpy(), np.stack([T.gather_exact(f[bi], idx[bi]) for bi in range(2)]))
    case = T.hot_case('interp_three_targets')
    fm = np.stack([T.int_features(5 + bi, 3, 3) for bi in range(2)])
    P, C = T.interp_hot_geometry()
    out, idx, w = oracle.three_nearest_neighbors_interpolate_forward(_coords(P), _coords(C), _t(fm))
    assert np.array_equal(w.numpy(), np.broadcast_to(np.float32([0.5, 0.25, 0.25])[None, :, None], w.shape))
    assert np.array_equal(idx.numpy(), np.stack([T.three_nn_exact(P[bi], C[bi]) for bi in range(2)]))
    assert np.array_equal(out.numpy(), np.stack([T.interp_exact(fm[bi].astype(np.int64), idx[bi].numpy(), case['w_num'][bi]) / T.HOT_W_DENOM
                                                 for bi in range(2)]))


# ---- the certificates accept the oracle: zero complaints

def _oracle_chain(oracle, i):
    """The chain of the GPU file on the oracle: FPS -> centres -> ball query, and 3-NN from the centres back to the cloud."""
    clouds, m, radius = T.cloud_case(i)
    p = _t(np.stack(clouds))
    picked = oracle.furthest_point_sampling(p, m).numpy()
    centers = np.stack([T.centers_of(c, picked[bi], 7000 + 10 * i + bi) for bi, c in enumerate(clouds)])
    balls = oracle.ball_query(_t(centers), p, radius, T.CLOUD_U).numpy()
    feats = np.stack([T.int_features(i * 10 + bi, 4, centers.shape[2]) for bi in range(len(clouds))])
    out, idx, w = [x.numpy() for x in oracle.three_nearest_neighbors_interpolate_forward(p, _t(centers), _t(feats))]
    return clouds, radius, picked, centers, balls, feats, out, idx, w


@pytest.mark.parametrize('i', range(len(T.CLOUD_CASES)), ids=[f'{c[0]}-{c[2]}' for c in T.CLOUD_CASES])
def test_certificates_accept_the_oracle_without_a_single_complaint(oracle, i):
    clouds, radius, picked, centers, balls, feats, out, idx, w = _oracle_chain(oracle, i)
    hits = []
    for bi, p in enumerate(clouds):
        assert T.fps_certificate(p, picked[bi]) == []
        assert T.ball_query_certificate(p, centers[bi], radius, T.CLOUD_U, balls[bi]) == []
        assert T.three_nn_certificate(p, centers[bi], idx[bi], w[bi]) == []
        value, bound = T.interp_out_bound(feats[bi], idx[bi], w[bi])
        assert (np.abs(out[bi] - value) <= bound).all()
        r2 = float(np.float32(radius) * np.float32(radius))
        hits.append((T.sq_dist_f64(p, centers[bi]) < r2).sum(axis=1))
    hits = np.concatenate(hits)
    # the radius of the kind makes the case say something: rows without a hit, rows that are padded, rows that are full
    assert (hits == 0).any() and ((hits > 0) & (hits < T.CLOUD_U)).any() and (hits >= T.CLOUD_U).any(), np.bincount(np.minimum(hits, T.CLOUD_U))


# ---- the certificates have teeth

@pytest.fixture(scope='module')
def answer(oracle):
    clouds, radius, picked, centers, balls, feats, out, idx, w = _oracle_chain(oracle, 0)       # 'uniform', cloud 0
    return dict(p=clouds[0], radius=radius, picked=picked[0], centers=centers[0], balls=balls[0], idx=idx[0], w=w[0])


def _clear_steps(p, picked):
    """Per step j: (runner-up point, its distance / the maximum) of the fp64 replay."""
    out = {}
    for j, dist in T.fps_replay(p, picked):
        order = np.argsort(dist)
        out[j] = (int(order[-2]), dist[order[-2]] / dist[order[-1]])
    return out


def test_fps_certificate_rejects_swapped_picks(answer):
    bad = answer['picked'].copy()
    bad[[3, 10]] = bad[[10, 3]]
    assert T.fps_certificate(answer['p'], answer['picked']) == [] and T.fps_certificate(answer['p'], bad) != []


def test_fps_certificate_rejects_the_runner_up_of_another_step(answer):
    p, picked = answer['p'], answer['picked']
    steps = _clear_steps(p, picked)
    j = next(j for j in range(5, len(picked) - 1) if steps[j + 1][1] < 0.999 and steps[j + 1][0] not in picked[:j + 1])
    bad = picked.copy()
    bad[j] = steps[j + 1][0]                                  # at step j this point is not the furthest: it only is second at j + 1
    assert any(c.startswith(f'step {j}:') for c in T.fps_certificate(p, bad))
    assert T.fps_certificate(p, np.r_[1, picked[1:]]) != []   # and the start is pinned


def test_ball_certificate_rejects_planted_faults(answer):
    p, c, radius, u, balls = answer['p'], answer['centers'], answer['radius'], T.CLOUD_U, answer['balls']
    cert = lambda rows: T.ball_query_certificate(p, c, radius, u, rows)
    assert cert(balls) == []
    d = T.sq_dist_f64(p, c)
    r2 = float(np.float32(radius) * np.float32(radius))
    hits = (d < r2).sum(axis=1)
    short = int(np.flatnonzero((hits >= 4) & (hits < u))[0])            # a padded row with at least four hits
    # a hit replaced by a point at 1.01 r: move the cloud's point onto the ray instead of searching for one
    row = balls[short]
    q = p.copy()
    outside = int(np.flatnonzero(d[short] > 4 * r2)[-1])
    q[:, outside] = (c[:, short] + 1.01 * float(np.float32(radius)) * np.array([1.0, 0.0, 0.0])).astype(np.float32)
    planted = balls.copy()
    planted[short, :hits[short]] = np.sort(np.r_[row[:hits[short] - 1], outside])     # (the list stays ascending)
    assert any(f'row {short}:' in s and 'outside the ball' in s for s in T.ball_query_certificate(q, c, radius, u, planted))
    # a hit left out of the middle of a row
    gap = balls.copy()
    gap[short, 1:hits[short] - 1] = row[2:hits[short]]
    gap[short, hits[short] - 1] = row[0]
    assert any(f'row {short}:' in s and 'not listed' in s for s in cert(gap))
    full = int(np.flatnonzero(hits > u)[0])                              # ... also in a row that is full
    gap = balls.copy()
    later = np.flatnonzero(d[full] < r2)
    gap[full, 1:] = later[2:u + 1]
    assert any(f'row {full}:' in s and 'not listed' in s for s in cert(gap))
    # a wrong padding value
    pad = balls.copy()
    pad[short, -1] = row[1]
    assert any(f'row {short}:' in s for s in cert(pad))
    # a non-zero row where nothing is in reach, and an all-zero row where something is
    empty = int(np.flatnonzero(hits == 0)[-1])                           # (the far centre)
    ghost = balls.copy()
    ghost[empty, :] = 3
    assert any(f'row {empty}:' in s and 'not zeros' in s for s in cert(ghost))
    blank = balls.copy()
    blank[short, :] = 0
    assert any(f'row {short}:' in s for s in cert(blank))


def test_three_nn_certificate_rejects_planted_faults(answer):
    p, c, idx, w = answer['p'], answer['centers'], answer['idx'], answer['w']
    assert T.three_nn_certificate(p, c, idx, w) == []
    d = T.sq_dist_f64(p, c).T
    order = np.argsort(d, axis=1, kind='stable')
    ds = np.take_along_axis(d, order[:, :4], axis=1)
    j = int(np.flatnonzero((ds[:, 3] > 1.01 * ds[:, 2]) & (ds[:, 0] > 1e-6))[0])
    swapped = idx.copy()
    swapped[1, j] = order[j, 3]                               # the second and the fourth nearest exchanged
    assert any(f'point {j}:' in s for s in T.three_nn_certificate(p, c, swapped, w))
    twice = idx.copy()
    twice[2, j] = twice[0, j]
    assert any(f'point {j}:' in s and 'repeat' in s for s in T.three_nn_certificate(p, c, twice, w))
    off = w.copy()
    off[1, j] = np.float32(off[1, j] * (1 + 64 * T.U24))     # one weight off by 64u
    assert off[1, j] != w[1, j]
    assert any(f'point {j}:' in s and '32u' in s for s in T.three_nn_certificate(p, c, idx, off))
    scaled = (w.astype(np.float64) * (1 + 16 * T.U24)).astype(np.float32)   # every weight inside 32u, the sum 16u off
    assert any('sum to 1' in s for s in T.three_nn_certificate(p, c, idx, scaled))
