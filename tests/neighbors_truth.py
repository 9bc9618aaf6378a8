"""Truths of their own for the PointNet++ neighbourhood operators (csrc/fps.hip, csrc/neighbors.hip and their CSR backwards):
furthest point sampling, ball query, grouping / gather, 3-NN interpolation.  numpy only; the oracle is not imported here.

Two kinds of judge, both per cloud (coordinates (3, N), like one sample of the (B, 3, N) tensors):

  exact truths   on INTEGER coordinates (the numerators of dyadic coordinates k / 8): every squared distance is an integer, every fp32
                 evaluation of it is exact whatever the contraction, so the answer is unique and `==` is the bar.
  certificates   fp64 checks of an ANSWER on any fp32 cloud.  They state what a correct answer must satisfy and need no tie rule,
                 no rounding model and no excluded rows.  U24 = 2^-24 is the unit round-off of fp32.
                 One fp32 evaluation of d^2 = dx^2 + dy^2 + dz^2: each difference is one rounding (1u), each square one more on top of
                 twice that (3u), the two additions of non-negative terms one each (5u), and a fused multiply-add only removes
                 roundings: relative error <= 5u for every contraction choice.  DELTA = 8u is that bound with a margin -- derived,
                 not measured.

Every certificate returns the list of its complaints (strings that name the row); an accepted answer returns [].
"""
import functools

import numpy as np

U24 = 2.0 ** -24
DELTA = 8 * U24           # relative error granted to one fp32 squared distance (5u derived, see above)
W_SUM_TOL = 8 * U24       # |w0 + w1 + w2 - 1|: w_s = fl(n_s * inv), inv = fl(1 / S), S the fp32 sum of the numerators n_s: two roundings in
#                           S, one in inv, one per product -> the exact sum of the returned weights is within 4u of 1; 8u granted
W_REL_TOL = 32 * U24      # each weight, relative: 10u for each of the two products of 5u-accurate distances in the quotient
#                           (numerator 10u, denominator 10u) + 6u for the product, sum, reciprocal and scale roundings
CLAMP_LO = float(np.float32(1e-10))
CLAMP_HI = float(np.float32(1e10))
FPS_SLOTS = 512           # the tie rule of fps.hip:12-15: smallest (k mod 512, k) among equidistant candidates


# ------------------------------------------------------------------------------------------------
# exact truths (integer coordinates)
# ------------------------------------------------------------------------------------------------

def _ints(a):
    a = np.asarray(a)
    assert a.dtype.kind in 'iu', 'the exact truths take integer numerators'
    return a.astype(np.int64)


def sq_dist_int(P, C):
    """(M, N) int64: squared distances between the centres C (3, M) and the points P (3, N)."""
    P, C = _ints(P), _ints(C)
    return ((C[:, :, None] - P[:, None, :]) ** 2).sum(axis=0)


def fps_exact(P, m):
    """P (3, N) integers, m <= N -> (m,) int32.  Start at 0; running minimum squared distances in integers; each step the arg-max,
    ties to the smallest (k mod 512, k)."""
    P = _ints(P)
    n = P.shape[1]
    out = np.zeros(m, dtype=np.int32)
    k = np.arange(n)
    order = np.lexsort((k, k % FPS_SLOTS))                  # candidates in the order of the tie rule
    Po = P[:, order]
    dist = np.full(n, np.iinfo(np.int64).max, dtype=np.int64)   # (in tie order)
    old = 0
    for j in range(1, m):
        d = ((Po - P[:, old:old + 1]) ** 2).sum(axis=0)
        np.minimum(dist, d, out=dist)
        old = int(order[np.argmax(dist)])                   # argmax: the FIRST maximum of the tie order
        out[j] = old
    return out


def ball_query_exact(P, C, r2, u):
    """P (3, N), C (3, M) integers, r2 the integer squared radius -> (M, u) int32: the first u indices, ascending, with d^2 < r2
    (strictly); the remaining slots repeat the first hit; a row without a hit is all zeros."""
    d = sq_dist_int(P, C)
    out = np.zeros((d.shape[0], u), dtype=np.int32)
    for i in range(d.shape[0]):
        hits = np.flatnonzero(d[i] < r2)[:u]
        if hits.size:
            out[i, :] = hits[0]
            out[i, :hits.size] = hits
    return out


def three_nn_exact(P, C):
    """P (3, N), C (3, M) integers -> (3, N) int32: per point the three centres with the smallest (d^2, index); with M < 3 the
    missing slots are index 0.  (A stable sort by d^2 IS the strict-'<' insertion of the kernel.)"""
    d = sq_dist_int(P, C).T                                 # (N, M)
    out = np.zeros((3, d.shape[0]), dtype=np.int32)
    k = min(3, d.shape[1])
    if k:
        out[:k] = np.argsort(d, axis=1, kind='stable')[:, :k].T
    return out


def gather_exact(f, idx):
    """f (C, N), idx (...) -> (C, ...): the forward of gather (idx (M,)) and of grouping (idx (M, U))."""
    return np.asarray(f)[:, np.asarray(idx, dtype=np.int64)]


def index_scatter_exact(g, idx, n):
    """The backward of gather / grouping in integers: g (C, ...) integers, idx (...) -> (C, n) int64, gx[c, idx[e]] += g[c, e]."""
    g, idx = _ints(g), np.asarray(idx, dtype=np.int64).reshape(-1)
    g = g.reshape(g.shape[0], -1)
    out = np.zeros((g.shape[0], n), dtype=np.int64)
    for c in range(g.shape[0]):
        np.add.at(out[c], idx, g[c])
    return out


def interp_exact(f, idx, w_num):
    """The forward of the 3-NN interpolation in integers: f (C, M) integers, idx (3, N), w_num (3, N) integer numerators of the
    weights -> (C, N) int64 numerators of the outputs (same denominator as the weights)."""
    f, idx, w_num = _ints(f), np.asarray(idx, dtype=np.int64), _ints(w_num)
    return (f[:, idx] * w_num[None]).sum(axis=1)


def interp_scatter_exact(g, idx, w_num, m):
    """Its backward: g (C, N) integers -> (C, m) int64 numerators, gx[c, idx[s, j]] += w_num[s, j] * g[c, j]."""
    g, idx, w_num = _ints(g), np.asarray(idx, dtype=np.int64), _ints(w_num)
    out = np.zeros((g.shape[0], m), dtype=np.int64)
    for c in range(g.shape[0]):
        for s in range(3):
            np.add.at(out[c], idx[s], w_num[s] * g[c])
    return out


# ------------------------------------------------------------------------------------------------
# certificates (fp64 checks of an answer on fp32 coordinates)
# ------------------------------------------------------------------------------------------------

def _f64(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, 'the certificates judge answers to fp32 inputs'
    return a.astype(np.float64)


def sq_dist_f64(p, c):
    """(M, N) fp64 squared distances between the centres c (3, M) and the points p (3, N), both fp32."""
    p, c = _f64(p), _f64(c)
    return ((c[:, :, None] - p[:, None, :]) ** 2).sum(axis=0)


def fps_replay(p, idx):
    """The fp64 replay the certificate judges by: for every step j >= 1 the distances of all points to the set idx[:j].
    Yields (j, dist (N,) fp64)."""
    p = _f64(p)
    dist = np.full(p.shape[1], np.inf)
    for j in range(1, len(idx)):
        prev = int(idx[j - 1])
        np.minimum(dist, ((p - p[:, prev:prev + 1]) ** 2).sum(axis=0), out=dist)
        yield j, dist


def fps_certificate(p, idx):
    """idx[0] == 0, and at every later step the chosen point's fp64 distance to the points chosen so far is at least (1 - DELTA)
    times the largest such distance of the cloud -- exactly 0 when that maximum is 0."""
    idx = np.asarray(idx)
    n = np.asarray(p).shape[1]
    bad = []
    if len(idx) == 0:
        return bad
    if ((idx < 0) | (idx >= n)).any():
        return ['index out of range']
    if idx[0] != 0:
        bad.append(f'step 0: starts at {int(idx[0])}, not at 0')
    for j, dist in fps_replay(p, idx):
        top, got = dist.max(), dist[int(idx[j])]
        if (got != 0.0) if top == 0.0 else (got < (1.0 - DELTA) * top):
            bad.append(f'step {j}: point {int(idx[j])} at {got!r}, the furthest is at {top!r}')
    return bad


def ball_query_certificate(p, c, radius, u, out):
    """out (M, u) int: every row is [a strictly ascending list of hits][its first element, repeated]; every listed point is inside
    r2 (1 + DELTA); every point inside r2 (1 - DELTA) below the last listed index -- below N when the list is shorter than u -- is
    listed; a row is all zeros when nothing is inside r2 (1 + DELTA).  r2 = float32(radius)^2 rounded to fp32 (neighbors.hip:127)."""
    out = np.asarray(out)
    n, m = np.asarray(p).shape[1], np.asarray(c).shape[1]
    assert out.shape == (m, u)
    r2 = float(np.float32(radius) * np.float32(radius))
    d = sq_dist_f64(p, c)
    may, must = d < r2 * (1.0 + DELTA), d < r2 * (1.0 - DELTA)
    bad = []
    for i in range(m):
        row = out[i].astype(np.int64)
        if u == 0:
            continue
        if ((row < 0) | (row >= max(n, 1))).any():
            bad.append(f'row {i}: index out of range')
            continue
        if not may[i].any():
            if row.any():
                bad.append(f'row {i}: no point is in reach, the row is not zeros')
            continue
        if not row.any() and not may[i, 0]:                 # the row claims "no hit"
            if must[i].any():
                bad.append(f'row {i}: claims no hit, point {int(np.flatnonzero(must[i])[0])} is inside')
            continue
        ln = 1
        while ln < u and row[ln] > row[ln - 1]:
            ln += 1
        listed = row[:ln]
        if (row[ln:] != row[0]).any():
            bad.append(f'row {i}: slots behind the {ln} hits do not repeat the first hit')
        if not may[i, listed].all():
            bad.append(f'row {i}: lists point {int(listed[~may[i, listed]][0])} outside the ball')
        limit = n if ln < u else int(listed[-1])
        owed = np.flatnonzero(must[i, :limit])
        missing = np.setdiff1d(owed, listed)
        if missing.size:
            bad.append(f'row {i}: point {int(missing[0])} is inside and comes before index {limit}, but is not listed')
    return bad


def three_nn_weights_f64(d3):
    """The definition of the weights on three squared distances (..., 3) fp64 (inf: no such centre): clamp to [1e-10f, 1e10f],
    w0 = d1 d2 / S, w1 = d0 d2 / S, w2 = d0 d1 / S with S = d0 d1 + d0 d2 + d1 d2."""
    d = np.clip(d3, CLAMP_LO, CLAMP_HI)
    d0, d1, d2 = d[..., 0], d[..., 1], d[..., 2]
    s = d0 * d1 + d0 * d2 + d1 * d2
    return np.stack([d1 * d2 / s, d0 * d2 / s, d0 * d1 / s], axis=-1)


def three_nn_certificate(p, c, idx, w):
    """idx, w (3, N): per point the three indices are distinct (M >= 3; with M < 3 the missing slots are index 0), their fp64
    distances do not decrease beyond DELTA, no other centre is closer than (1 - DELTA) times the third, the weights sum to 1
    within 8u and each is within 32u, relative, of the definition evaluated in fp64 on the returned indices."""
    idx, w = np.asarray(idx).astype(np.int64), np.asarray(w)
    n, m = np.asarray(p).shape[1], np.asarray(c).shape[1]
    assert idx.shape == (3, n) and w.shape == (3, n) and w.dtype == np.float32 and m >= 1
    bad = []
    if ((idx < 0) | (idx >= m)).any():
        return ['index out of range']
    k = min(3, m)
    d = sq_dist_f64(p, c).T                                  # (N, M)
    rows = np.arange(n)
    d3 = np.full((n, 3), np.inf)
    for s in range(k):
        d3[:, s] = d[rows, idx[s]]

    def complain(mask, what):
        for j in np.flatnonzero(mask)[:8]:
            bad.append(f'point {int(j)}: {what} (indices {idx[:, j].tolist()}, distances {d3[j].tolist()}, weights {w[:, j].tolist()})')
        if mask.sum() > 8:
            bad.append(f'... and {int(mask.sum()) - 8} more points: {what}')

    if k < 3:
        complain((idx[k:] != 0).any(axis=0), 'a slot without a centre is not index 0')
    same = np.zeros(n, dtype=bool)
    for a in range(k):
        for b in range(a + 1, k):
            same |= idx[a] == idx[b]
    complain(same, 'indices repeat')
    for s in range(k - 1):
        complain(d3[:, s] * (1.0 - DELTA) > d3[:, s + 1], f'neighbour {s} is farther than neighbour {s + 1}')
    if m > k:
        others = d.copy()
        for s in range(k):
            others[rows, idx[s]] = np.inf
        complain(others.min(axis=1) < (1.0 - DELTA) * d3[:, k - 1], 'a centre that is not listed is closer than the last listed one')
    w64 = w.astype(np.float64).T                             # (N, 3)
    complain(~(np.abs(w64.sum(axis=1) - 1.0) <= W_SUM_TOL), 'the weights do not sum to 1 within 8u')
    want = three_nn_weights_f64(d3)
    complain(~(np.abs(w64 - want) <= W_REL_TOL * want).all(axis=1), 'a weight is more than 32u from its definition')
    return bad


def interp_out_bound(f, idx, w):
    """The 3-NN interpolation output from the RETURNED indices and weights: (value (C, N) fp64, bound (C, N)).  The kernel forms
    fma(f2, w2, fma(f0, w0, f1 * w1)): at most three roundings, each of a partial sum that is at most sum |f_s w_s| when the
    terms have one sign and is bounded by it otherwise -> |out - value| <= 3u sum |f_s w_s|, plus u |value| for the fp32 result
    itself being compared; 4u sum |f_s w_s| granted."""
    f, idx, w = _f64(f), np.asarray(idx).astype(np.int64), _f64(w)
    terms = f[:, idx] * w[None]                              # (C, 3, N)
    return terms.sum(axis=1), 4 * U24 * np.abs(terms).sum(axis=1)


# ------------------------------------------------------------------------------------------------
# seeded generators
# ------------------------------------------------------------------------------------------------

DENOM = 8     # the lattice coordinates are numerators / 8; lattice points sit on even numerators (multiples of 1/4)


def lattice_cloud(seed, n, dims):
    """(3, n) int64 numerators: the points 2 * (i, j, k) of a dims[0] x dims[1] x dims[2] lattice, shuffled; n above the lattice size
    repeats points (exact duplicates), n below it leaves some out.  Every squared distance stays below 2^24 numerator units."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(s) for s in dims], indexing='ij')).reshape(3, -1) * 2
    total = g.shape[1]
    pick = rng.permutation(total)[:n] if n <= total else np.concatenate([np.arange(total), rng.integers(0, total, n - total)])
    return g[:, rng.permutation(pick)].astype(np.int64)


def lattice_centers(seed, P, m, far=400):
    """(3, m) int64 numerators: in turn a cloud point, a cloud point moved by one numerator along x (off the lattice: no d^2 = 0)
    and a far point that no radius used here reaches; with an empty cloud, points near the origin."""
    rng = np.random.default_rng(seed)
    n = P.shape[1]
    C = np.zeros((3, m), dtype=np.int64)
    for i in range(m):
        base = P[:, rng.integers(0, n)] if n else rng.integers(0, 8, 3)
        if i % 3 == 1:
            base = base + np.array([1, 0, 0])
        elif i % 3 == 2 and m > 2:
            base = base + far + np.array([i, 0, 0])
        C[:, i] = base
    return C


def as_coords(Pi):
    """Integer numerators -> the fp32 coordinates numerator / 8 (exact)."""
    return (np.asarray(Pi, dtype=np.float64) / DENOM).astype(np.float32)


# FPS on lattices: (N, lattice dims, M, B).  N: every launch shape of fps.hip from its smallest (1, 2; one wave with 63 / 64 / 65 points;
# 1024 -> 1025: the 64-thread to the 512-thread kernel; 8192 -> 8193: to the 1024-thread kernel), cubic and non-cubic lattices;
# M = N: once the lattice is exhausted every step is a tie at distance 0.
LATTICE_FPS_CASES = [
    (1, (1, 1, 1), 1, 3), (2, (2, 1, 1), 2, 3), (63, (4, 4, 4), 63, 3), (64, (4, 4, 4), 64, 1), (65, (4, 4, 4), 65, 3),
    (216, (6, 6, 6), 216, 1), (729, (9, 9, 8), 729, 3), (1025, (10, 10, 10), 1025, 1), (1728, (12, 12, 12), 600, 3),
    (8193, (20, 20, 20), 8193, 1),
]

# ball query on lattices: (N, lattice dims, M, U, r numerator, B).  Radius 6/8 puts the lattice points (6,0,0), (4,4,2) away from a
# cloud-point centre exactly ON the sphere, radius 5/8 the points (5,0,0), (3,4,0) away from an off-lattice centre; radius 0 hits nothing.
LATTICE_BALL_CASES = [
    (1000, (10, 10, 10), 77, 64, 6, 2), (1000, (10, 10, 10), 77, 65, 5, 2), (1000, (10, 10, 9), 5, 128, 6, 2),
    (1000, (10, 10, 10), 4, 5, 5, 2), (1000, (10, 10, 10), 1, 1, 6, 2), (65, (4, 4, 4), 5, 128, 6, 2), (64, (4, 4, 4), 4, 64, 5, 2),
    (63, (4, 4, 4), 77, 65, 6, 2), (1, (1, 1, 1), 4, 5, 6, 2), (1, (1, 1, 1), 1, 1, 5, 1), (0, (1, 1, 1), 5, 5, 6, 2),
    (0, (1, 1, 1), 1, 64, 5, 1), (1000, (10, 10, 10), 77, 5, 0, 2), (65, (4, 4, 4), 4, 1, 0, 2),
]

# 3-NN on lattices: (N, point lattice dims, M, centre lattice dims, B).  The centres are a coarse lattice with repeats: every point has
# equidistant centres, and duplicated ones.  N = 255 / 256 / 257 / 1000: the tail block of three_nn_kernel (256 threads).
LATTICE_NN_CASES = [
    (1, (1, 1, 1), 1, (1, 1, 1), 2), (255, (7, 6, 6), 2, (2, 1, 1), 2), (256, (8, 8, 4), 3, (2, 1, 1), 2), (257, (8, 8, 4), 64, (4, 3, 3), 2),
    (1000, (10, 10, 10), 64, (4, 4, 3), 2), (1000, (10, 10, 10), 3, (3, 1, 1), 1), (257, (7, 6, 6), 1, (1, 1, 1), 1), (1000, (10, 10, 9), 2, (1, 1, 1), 1),
]


@functools.lru_cache(maxsize=None)
def lattice_fps_case(i):
    """-> list over the B clouds of (P int (3, N),), a different shuffle per cloud."""
    n, dims, m, b = LATTICE_FPS_CASES[i]
    return [lattice_cloud(1000 * i + bi, n, dims) for bi in range(b)], m


@functools.lru_cache(maxsize=None)
def lattice_ball_case(i):
    """-> (list of P (3, N), list of C (3, M), U, r numerator)."""
    n, dims, m, u, r, b = LATTICE_BALL_CASES[i]
    Ps = [lattice_cloud(2000 * i + bi, n, dims) for bi in range(b)]
    Cs = [lattice_centers(2000 * i + 500 + bi, P, m) for bi, P in enumerate(Ps)]
    return Ps, Cs, u, r


@functools.lru_cache(maxsize=None)
def lattice_nn_case(i):
    """-> (list of P (3, N), list of C (3, M)): the centres on a coarse lattice (spacing 3 lattice steps), shuffled, repeated up to M."""
    n, dims, m, cdims, b = LATTICE_NN_CASES[i]
    Ps = [lattice_cloud(3000 * i + bi, n, dims) for bi in range(b)]
    Cs = [lattice_cloud(3000 * i + 500 + bi, m, cdims) * 3 for bi in range(b)]
    return Ps, Cs


CLOUD_KINDS = ('uniform', 'clusters', 'twins', 'far', 'tiny', 'line')
# ball radius per kind at N = 1500 (it shrinks with the density, cloud_radius): some rows with fewer than U = 16 hits, most with more
CLOUD_RADIUS = {'uniform': 0.15, 'clusters': 2e-3, 'twins': 0.15, 'far': 0.15, 'tiny': 1.5e-5, 'line': 5e-3}


def cloud_radius(kind, n):
    return CLOUD_RADIUS[kind] * (1500.0 / n) ** (1.0 if kind == 'line' else 1.0 / 3.0)


def fp32_cloud(kind, seed, n):
    """(3, n) fp32.  uniform: the unit cube; clusters: eight Gaussian blobs of sigma 1e-3; twins: groups of four -- a point, an exact
    duplicate, and its 1-ulp neighbours up and down in every coordinate; far: the unit cube at offset 1000; tiny: the unit cube
    scaled by 1e-4; line: points on one straight line."""
    rng = np.random.default_rng(seed)
    if kind == 'uniform':
        p = rng.random((3, n))
    elif kind == 'clusters':
        mid = rng.random((3, 8))
        p = mid[:, rng.integers(0, 8, n)] + 1e-3 * rng.standard_normal((3, n))
    elif kind == 'twins':
        base = (rng.random((3, (n + 3) // 4)) + 0.25).astype(np.float32)
        up, down = np.nextafter(base, np.float32(np.inf)), np.nextafter(base, np.float32(-np.inf))
        p = np.concatenate([base, base, up, down], axis=1)[:, :n]
        p = p[:, rng.permutation(n)]
    elif kind == 'far':
        p = rng.random((3, n)) + 1000.0
    elif kind == 'tiny':
        p = rng.random((3, n)) * 1e-4
    elif kind == 'line':
        a, d = rng.random((3, 1)), rng.standard_normal((3, 1))
        p = a + d / np.linalg.norm(d) * rng.random((1, n))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(p, dtype=np.float32)


def off_cloud_points(seed, p, k=4):
    """(3, k + 1) fp32 centres that are no cloud points: k midpoints of random pairs, and one point ten cloud extents away (no hit)."""
    rng = np.random.default_rng(seed)
    n = p.shape[1]
    a, b = rng.integers(0, n, k), rng.integers(0, n, k)
    mid = (p[:, a].astype(np.float64) + p[:, b]) / 2
    lo, hi = p.min(axis=1, keepdims=True).astype(np.float64), p.max(axis=1, keepdims=True)
    away = hi + 10 * np.maximum(hi - lo, 1e-6)
    return np.concatenate([mid, away], axis=1).astype(np.float32)


# the certificate family: (kind, B, N, M of FPS).  The six kinds at (2, 1500, 96); then one kind on either side of each FPS launch
# boundary: 1024 / 1025 (64 -> 512 threads), 8192 / 8193 (512 -> 1024 threads), 12266 / 12267 (the last cloud whose LDS copy fits
# 144 KiB next to the slots of 16 waves: 3 * 4 * N + 256 <= 147456), 16384 / 16385 (the global-memory kernel).
CLOUD_CASES = [(kind, 2, 1500, 96) for kind in CLOUD_KINDS] + [
    ('uniform', 1, 1024, 32), ('clusters', 1, 1025, 32), ('twins', 1, 8192, 32), ('far', 1, 8193, 32),
    ('tiny', 1, 12266, 32), ('line', 1, 12267, 32), ('twins', 1, 16384, 32), ('uniform', 1, 16385, 32),
]
CLOUD_U = 16
CLOUD_OFF = 4     # off-cloud centres per cloud, plus the one far away


@functools.lru_cache(maxsize=None)
def cloud_case(i):
    """-> (list over B of p (3, N) fp32, M, radius)."""
    kind, b, n, m = CLOUD_CASES[i]
    return [fp32_cloud(kind, 4000 * i + bi, n) for bi in range(b)], m, cloud_radius(kind, n)


def int_features(seed, c, n, lo=-8, hi=9):
    """(c, n) fp32 with small integer values: gathers of them, and their sums with dyadic weights, are exact."""
    return np.random.default_rng(seed).integers(lo, hi, (c, n)).astype(np.float32)


def centers_of(p, picked, seed):
    """The centres of the certificate family: the FPS output of the cloud followed by CLOUD_OFF + 1 off-cloud points."""
    return np.ascontiguousarray(np.concatenate([p[:, np.asarray(picked, dtype=np.int64)], off_cloud_points(seed, p, CLOUD_OFF)], axis=1))


# ------------------------------------------------------------------------------------------------
# hot-spot backwards: more than 8192 entries on one target range (the list-overflow path of csr_prep_kernel), small-integer
# gradients and weights 1/2, 1/4, 1/4: every partial sum is an integer multiple of 1/4 below 2^24 / 4, so every order of summation
# gives the same fp32 result and `==` with the integer truth is the bar.
# ------------------------------------------------------------------------------------------------

HOT_CASES = ('grouping_one_point', 'grouping_same_32', 'gather_two_targets', 'interp_three_targets')
HOT_W_DENOM = 4


@functools.lru_cache(maxsize=None)
def hot_case(name):
    """-> dict(op, idx int32, g fp32 (integer values), n targets[, w_num]) with a leading batch axis of 2 on idx / g / w_num."""
    rng = np.random.default_rng(HOT_CASES.index(name) + 77)
    b, c = 2, 3
    if name == 'grouping_one_point':                 # all M * U = 16384 indices of a cloud on one point of N = 64
        idx = np.empty((b, 128, 128), dtype=np.int32)
        idx[0], idx[1] = 5, 63
        return dict(op='grouping', idx=idx, g=rng.integers(-4, 5, (b, c, 128, 128)).astype(np.float32), n=64)
    if name == 'grouping_same_32':                   # a ball query in a dense cluster: every row the same 32 points, then its first hit
        idx = np.empty((b, 256, 64), dtype=np.int32)
        for bi in range(b):
            pts = np.sort(rng.permutation(64)[:32])
            idx[bi, :, :32], idx[bi, :, 32:] = pts, pts[0]
        return dict(op='grouping', idx=idx, g=rng.integers(-4, 5, (b, c, 256, 64)).astype(np.float32), n=64)
    if name == 'gather_two_targets':                 # M = 16384 onto 2 targets
        idx = np.array([[7, 8], [0, 63]], dtype=np.int32)[np.arange(b)[:, None], rng.integers(0, 2, (b, 16384))]
        return dict(op='gather', idx=np.ascontiguousarray(idx), g=rng.integers(-4, 5, (b, c, 16384)).astype(np.float32), n=64)
    if name == 'interp_three_targets':               # M = 3, N = 4096: 12288 entries on three targets
        idx = np.stack([np.stack([rng.permutation(3) for _ in range(4096)], axis=1) for _ in range(b)]).astype(np.int32)   # (b, 3, N)
        w_num = np.broadcast_to(np.array([2, 1, 1], dtype=np.int64)[None, :, None], idx.shape).copy()
        return dict(op='interp', idx=idx, w_num=w_num, g=rng.integers(-4, 5, (b, c, 4096)).astype(np.float32), n=3)
    raise ValueError(name)


def hot_truth(case):
    """(B, C, n) fp32: the integer truth of the backward of `case`."""
    g = case['g'].astype(np.int64)
    if case['op'] == 'interp':
        rows = [interp_scatter_exact(g[bi], case['idx'][bi], case['w_num'][bi], case['n']) / HOT_W_DENOM for bi in range(len(g))]
    else:
        rows = [index_scatter_exact(g[bi], case['idx'][bi], case['n']) for bi in range(len(g))]
    out = np.stack(rows)
    assert np.abs(out).max() < 2 ** 24 / HOT_W_DENOM and (out * HOT_W_DENOM == np.round(out * HOT_W_DENOM)).all()
    return out.astype(np.float32)


def interp_hot_geometry(n=4096):
    """Integer numerators (/ 8) of a geometry whose 3-NN weights are exactly 1/2, 1/4, 1/4: every point sits at (0,0,0) or (1,1,0),
    the centres at A = (1,0,0), B = (0,1,1), C = (0,1,-1): squared distances 1, 2, 2 -> products 2, 2, 4, sum 8.  Cloud 0 lists the
    centres as (A, B, C), cloud 1 as (B, A, C).  -> (P (2, 3, n), C (2, 3, 3))."""
    rng = np.random.default_rng(99)
    spots = np.array([[0, 0, 0], [8, 8, 0]]).T                                   # (3, 2)
    P = np.stack([spots[:, rng.integers(0, 2, n)] for _ in range(2)])
    A, B, C = [8, 0, 0], [0, 8, 8], [0, 8, -8]
    return P.astype(np.int64), np.stack([np.array([A, B, C]).T, np.array([B, A, C]).T]).astype(np.int64)
