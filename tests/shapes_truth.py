"""The definitions of "Shapes on the device" (include/pvcnn_hip.h) restated in numpy, and the acceptance inequalities of the normals.

Neighbour tables: the squared distance in fp32 with one rounding per operation, candidates ordered by (d, j) -- zero tolerance.
Normals: everything is measured in fp64 on the RETURNED neighbour table, against inequalities that do not depend on the solver.
"""
import numpy as np

U = 2.0 ** -24     # the unit round-off of fp32


def offsets_of(sizes):
    out = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=out[1:])
    return out


def sq_distances(x, q):
    """(len(q), len(x)) fp32: d[i, j] = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)), dx = fl(x_j - q_i).  numpy rounds every fp32
    operation once and fuses nothing."""
    x, q = np.asarray(x, dtype=np.float32), np.asarray(q, dtype=np.float32)
    dx = x[None, :, 0] - q[:, None, 0]
    dy = x[None, :, 1] - q[:, None, 1]
    dz = x[None, :, 2] - q[:, None, 2]
    d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == np.float32
    return d


def k_nearest_definition(rows, offsets, k):
    """The definition, literally: per cloud a stable sort of every query's distances.  (R, k) int32, -1 beyond min(k, n)."""
    rows, offsets = np.asarray(rows, dtype=np.float32), np.asarray(offsets, dtype=np.int64)
    out = np.full((rows.shape[0], k), -1, dtype=np.int32)
    for a, b in zip(offsets[:-1], offsets[1:]):
        x = rows[a:b, :3]
        kk = min(k, b - a)
        out[a:b, :kk] = np.argsort(sq_distances(x, x), axis=1, kind='stable')[:, :kk]
    return out


def k_nearest_rows(x, queries, k, chunk=256):
    """The same table for the query rows `queries` of ONE cloud x (n, >= 3), without sorting whole rows: the k-th smallest distance
    by selection, then a stable sort of the few candidates not above it (ascending position, so ties keep the rule)."""
    x = np.asarray(x, dtype=np.float32)[:, :3]
    queries = np.asarray(queries, dtype=np.int64)
    kk = min(k, x.shape[0])
    out = np.full((queries.shape[0], k), -1, dtype=np.int32)
    for c0 in range(0, queries.shape[0], chunk):
        qi = queries[c0:c0 + chunk]
        d = sq_distances(x, x[qi])
        bar = np.partition(d, kk - 1, axis=1)[:, kk - 1]
        for i in range(qi.shape[0]):
            cand = np.flatnonzero(d[i] <= bar[i])
            out[c0 + i, :kk] = cand[np.argsort(d[i, cand], kind='stable')][:kk]
    return out


def centroids(rows, offsets):
    """(W, 3) fp32: the fp64 mean of every cloud, rounded once."""
    rows = np.asarray(rows)
    return np.stack([rows[a:b, :3].astype(np.float64).mean(0) for a, b in zip(offsets[:-1], offsets[1:])]).astype(np.float32)


def covariances(rows, offsets, knn):
    """fp64, on the given table -> (C (R, 3, 3), eigenvalues (R, 3) ascending, v0 (R, 3), trace (R,), count (R,)); rows with fewer than
    three neighbours get zeros."""
    rows, knn = np.asarray(rows), np.asarray(knn)
    r = rows.shape[0]
    cov = np.zeros((r, 3, 3))
    count = np.zeros(r, dtype=np.int64)
    for a, b in zip(offsets[:-1], offsets[1:]):
        c = min(knn.shape[1], b - a)
        count[a:b] = c
        idx = knn[a:b, :c]
        assert (idx >= 0).all() and (idx < b - a).all() and (knn[a:b, c:] == -1).all()
        if c < 3:
            continue
        p = rows[a:b, :3].astype(np.float64)[idx]
        q = p - p.mean(1, keepdims=True)
        cov[a:b] = np.einsum('nki,nkj->nij', q, q)
    lam, vec = np.linalg.eigh(cov)
    return cov, lam, vec[:, :, 0], np.trace(cov, axis1=1, axis2=2), count


def epsilon(k):
    """The bound of the Rayleigh excess, in units of the trace: an fp32 covariance of k terms is off by at most (k + 3) u tr per entry,
    3 (k + 3) u tr in norm, the minimiser of the perturbed quotient exceeds lambda_0 by at most twice that; the rest of
    8 (k + 4) u is the solver's."""
    return 8.0 * (k + 4) * U


def check_normals(rows, offsets, knn, normals, curvature=None, mode=0, ref=None):
    """Assert every per-point requirement; returns the worst figures (for the record), each as a share of its bound."""
    rows, normals = np.asarray(rows), np.asarray(normals)
    assert normals.dtype == np.float32 and normals.shape == (rows.shape[0], 3)
    k = knn.shape[1]
    eps = epsilon(k)
    cov, lam, v0, tr, count = covariances(rows, offsets, knn)
    n = normals.astype(np.float64)
    zero = (count < 3) | (tr == 0)
    assert (normals[zero] == 0).all(), 'a point without a plane must get the zero normal'
    live = ~zero
    length = np.linalg.norm(n[live], axis=1)
    assert (np.abs(length - 1) <= 4 * U).all(), np.abs(length - 1).max()
    excess = np.einsum('ni,nij,nj->n', n, cov, n) - lam[:, 0]
    assert (excess[live] <= eps * tr[live]).all(), (excess[live] / tr[live]).max() / eps
    gap = lam[:, 1] - lam[:, 0]
    sep = live & (gap > 0)
    sin2 = 1 - np.einsum('ni,ni->n', n, v0) ** 2
    assert (sin2[sep] <= eps * tr[sep] / gap[sep]).all()
    worst = {'rayleigh': float((excess[live] / tr[live]).max() / eps) if live.any() else 0.0,
             'length': float(np.abs(length - 1).max() / (4 * U)) if live.any() else 0.0}
    if curvature is not None:
        curvature = np.asarray(curvature)
        assert curvature.dtype == np.float32 and curvature.shape == (rows.shape[0],)
        assert (curvature[zero] == 0).all()
        err = np.abs(curvature[live].astype(np.float64) - lam[live, 0] / tr[live])
        assert (err <= 2 * eps).all(), err.max() / (2 * eps)
        worst['curvature'] = float(err.max() / (2 * eps)) if live.any() else 0.0
    if mode:
        p = rows[:, :3].astype(np.float64)
        cloud = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
        away = p - np.asarray(ref, dtype=np.float64).reshape(-1, 3)[cloud]
        if mode == 2:
            away = -away
        assert (np.einsum('ni,ni->n', n, away) >= -1e-6 * np.linalg.norm(away, axis=1)).all()
    return worst


# ---- the clouds of the normals' cases ----------------------------------------------------------------------------------------
def normal_cases(seed, n=700):
    """name -> (n, 3) fp32: sphere, plane z = 0, tilted noisy plane, cube, box surface, a small sphere far from the origin."""
    rng = np.random.RandomState(seed)
    u = rng.randn(n, 3)
    sphere = (u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
    plane = np.c_[rng.rand(n, 2) * 2 - 1, np.zeros(n)].astype(np.float32)
    rot, _ = np.linalg.qr(rng.randn(3, 3))
    tilted = ((plane + np.c_[np.zeros((n, 2)), 0.002 * rng.randn(n)]) @ rot.T + 0.3).astype(np.float32)
    cube = (rng.rand(n, 3) * 2 - 1).astype(np.float32)
    m = n // 3
    box = np.concatenate([np.c_[rng.rand(m, 2), np.zeros(m)], np.c_[rng.rand(m), np.zeros(m), rng.rand(m)],
                          np.c_[np.zeros(n - 2 * m), rng.rand(n - 2 * m, 2)]]).astype(np.float32)
    far = (sphere * np.float32(0.01) + np.float32(1.0)).astype(np.float32)
    return {'sphere': sphere, 'plane_z0': plane, 'plane_tilted_noisy': tilted, 'uniform_cube': cube, 'box_surface': box,
            'far_from_origin': far}


def lattice_cloud(seed, n=900):
    """Coordinates randint(0, 16) / 16: every operation of the distance is exact, ties and duplicates abound."""
    return (np.random.RandomState(seed).randint(0, 16, size=(n, 3)).astype(np.float32) / np.float32(16))
