"""Seeded input generators shared by the CPU file that checks them (test_eval_truth_host.py) and the GPU fuzz files
(test_gpu_eval_fuzz.py, test_gpu_boxes_fuzz.py).  numpy only."""
import math

import numpy as np

from eval_truth import box_corners_f64

# ---- logits of the confidence test -----------------------------------------------------------------------------------------------


def confidence_logits(seed, b, c, n):
    """(B, C, N) float32: N(0, 4^2); the first 1/32 of the points of every cloud (at most 4096) has magnitudes up to +-80, and a
    tenth of the entries of classes >= 1 there is -inf (class 0 stays finite, so no point is all -inf).  In that block a narrow
    class range often lies > 87 below the maximum: both of its probabilities underflow in fp32 and its class cannot be told, which
    is what bounds the block's share (the excluded share is capped at 1 % per case)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((b, c, n), dtype=np.float32) * np.float32(4.0)
    k = min(max(n // 32, 1), 4096)
    x[:, :, :k] = rng.uniform(-80.0, 80.0, size=(b, c, k)).astype(np.float32)
    if c > 1:
        hole = rng.random((b, c - 1, k)) < 0.1
        blk = x[:, 1:, :k]
        blk[hole] = -np.inf
    return x


# (C, [(lo, hi) ...]) of the smaller confidence cases, at B = 4, N = 20000, seed 11 + C
CONFIDENCE_SMALL_CASES = [(1, [(0, 1)]), (2, [(0, 2), (1, 2)]), (50, [(0, 50), (12, 16), (47, 50)])]


# ---- box pairs -------------------------------------------------------------------------------------------------------------------
# a box is (center (x, y, z), heading, size (l, w, h)); its length axis is (cos heading, -sin heading) in (x, z)


def _random_box(rng, scale='kitti'):
    kind = rng.integers(0, 3)
    l, w, h = [(rng.uniform(3.2, 5.0), rng.uniform(1.4, 2.0), rng.uniform(1.3, 2.0)),       # car
               (rng.uniform(0.5, 1.2), rng.uniform(0.4, 0.9), rng.uniform(1.5, 2.0)),       # pedestrian
               (rng.uniform(1.4, 2.0), rng.uniform(0.4, 0.8), rng.uniform(1.5, 1.9))][kind]  # cyclist
    center = (rng.uniform(-30, 30), rng.uniform(0.0, 2.0), rng.uniform(5, 70))
    return center, rng.uniform(-math.pi, math.pi), (l, w, h)


def _near(rng, box):
    (x, y, z), a, (l, w, h) = box
    s = rng.uniform(0.8, 1.25, 3)
    return ((x + rng.normal(0, 0.5), y + rng.normal(0, 0.2), z + rng.normal(0, 0.5)), a + rng.normal(0, 0.3),
            (l * s[0], w * s[1], h * s[2]))


def _shift_along(box, frac):
    (x, y, z), a, (l, w, h) = box
    return ((x + frac * l * math.cos(a), y, z - frac * l * math.sin(a)), a, (l, w, h))


def _shrink(box, anchor, s):
    """The box scaled by s about a point of its own frame: anchor (u, v) in units of (l/2, w/2)."""
    (x, y, z), a, (l, w, h) = box
    lx, lz = anchor[0] * l / 2 * (1 - s), anchor[1] * w / 2 * (1 - s)
    c, sn = math.cos(a), math.sin(a)
    return ((x + c * lx + sn * lz, y, z - sn * lx + c * lz), a, (l * s, w * s, h))


def _grid_box(rng):
    """Axis-aligned, integer centre and even integer sizes: every corner is an integer, exactly, in fp32."""
    return ((float(rng.integers(-40, 41)), float(rng.integers(0, 3)), float(rng.integers(5, 60))), 0.0,
            (float(2 * rng.integers(1, 4)), float(2 * rng.integers(1, 3)), 2.0))


def box_pair_families(seed=20240521, n=1.0):
    """-> {family: [(box_a, box_b), ...]}: the parametric families of the box fuzz.  Areas >= 0.01 m^2, offsets <= 100 m."""
    rng = np.random.default_rng(seed)
    k = lambda m: max(int(m * n), 4)                                                    # noqa: E731
    fam = {}
    fam['kitti_random'] = [(b, _near(rng, b)) for b in (_random_box(rng) for _ in range(k(500)))]
    fam['kitti_far'] = [(_random_box(rng), _random_box(rng)) for _ in range(k(100))]
    fracs = [0.0, 0.25, 0.5, 0.75, 1.0, 1.5, -0.5]
    fam['edge_shift_grid'] = [(b, _shift_along(b, fracs[i % len(fracs)])) for i, b in enumerate(_grid_box(rng) for _ in range(k(140)))]
    fam['edge_shift_rotated'] = [(b, _shift_along(b, fracs[i % len(fracs)] if i % 2 else rng.uniform(0, 1.2)))
                                 for i, b in enumerate(_random_box(rng) for _ in range(k(260)))]
    turned = []
    for i in range(k(400)):
        (c, a, (l, w, h)) = _grid_box(rng) if i % 4 == 0 else _random_box(rng)
        if i % 2 == 0:
            w = l                                                                       # equal extents: a square turns onto itself
        eps = [0.0, 1e-7, -1e-7, 1e-4, -1e-4][i % 5]
        turned.append(((c, a, (l, w, h)), (c, a + (i % 4) * math.pi / 2 + eps, (l, w, h))))
    fam['quarter_turns'] = turned
    anchors = [(1, 1), (1, -1), (-1, -1), (1, 0), (0, 1), (-1, 0), (0, 0)]               # corners, edge midpoints, centre
    fam['shrunk_inside'] = []
    for i in range(k(420)):
        b = _grid_box(rng) if i % 3 == 0 else _random_box(rng)
        s = 0.5 if i % 3 == 0 else rng.uniform(0.2, 0.95)
        fam['shrunk_inside'].append((b, _shrink(b, anchors[i % len(anchors)], s)))
    fam['slivers'] = []
    for i in range(k(300)):
        c, a, (l, w, h) = _random_box(rng)
        l = rng.uniform(10.0, 20.0)
        sliver = (c, a, (l, l / 1000.0, h))
        other = [(c, a + rng.normal(0, 1e-3), (l, l / 1000.0, h)), _near(rng, sliver), (c, a + math.pi / 2, (l, l / 1000.0, h)),
                 _near(rng, (c, a, (4.0, 1.6, h)))][i % 4]
        fam['slivers'].append((sliver, other))
    fam['heights'] = []
    for i in range(k(300)):
        (x, _, z), a, (l, w, _) = _random_box(rng)
        b1 = ((x, 1.0, z), a, (l, w, 2.0))                                               # y range [0, 2]
        y2, h2 = [(3.0, 2.0), (1.0, 1.0), (5.0, 2.0), (2.0, 2.0), (1.25, 0.5)][i % 5]     # touch, nest, disjoint, half, nest
        b2 = _near(rng, b1)
        fam['heights'].append((b1, ((b2[0][0], y2, b2[0][2]), b2[1], (b2[2][0], b2[2][1], h2))))
    return fam


def pair_corners(pair):
    """(3, 8) float32 corner sets of a pair, as the meter holds them (fp64 formula, then fp32)."""
    return tuple(box_corners_f64(*b).astype(np.float32) for b in pair)


def quad_box(points, y_top, y_bottom):
    """(3, 8) float32 corners of a prism over the BEV quad points[0..3] ((x, z) of corners 0..3)."""
    c = np.zeros((3, 8), dtype=np.float32)
    for i, (x, z) in enumerate(points):
        c[0, i] = c[0, i + 4] = x
        c[2, i] = c[2, i + 4] = z
    c[1, :4] = y_top
    c[1, 4:] = y_bottom
    return c


def vertex_on_edge_pairs(seed=7, n=200):
    """A 4 x 2 integer rectangle and a diamond of integer / half-integer vertices, one of them placed ON an edge or a corner of the
    rectangle, both shifted by integers: every coordinate is exact in fp32, so 'on the edge' is exact.
    -> [(corners_a, corners_b)]"""
    rng = np.random.default_rng(seed)
    rect = [(4, 0), (4, 2), (0, 2), (0, 0)]
    out = []
    for i in range(n):
        r = [1.0, 0.5, 1.5, 2.0][i % 4]                                                  # diamond half-diagonal
        # the diamond's left vertex at (vx, vz): on the right edge x = 4 (touching from outside), on it from inside (right vertex),
        # on a corner, or on the top edge
        mode = i % 5
        if mode == 0:
            cx, cz = 4 + r, 1.0                                                          # left vertex (4, 1): a point of contact
        elif mode == 1:
            cx, cz = 4 - r, 1.0                                                          # right vertex (4, 1): inside, touching
        elif mode == 2:
            cx, cz = 4.0, 2 + r                                                          # bottom vertex on the corner (4, 2)
        elif mode == 3:
            cx, cz = 2.0, 2 - r                                                          # top vertex (2, 2) on the top edge, inside
        else:
            cx, cz = 4.0, 1.0                                                            # centre on the edge: two edges cross it
        diamond = [(cx + r, cz), (cx, cz + r), (cx - r, cz), (cx, cz - r)]
        ox, oz = float(rng.integers(-60, 61)), float(rng.integers(-60, 61))
        mv = lambda pts: [(x + ox, z + oz) for x, z in pts]                              # noqa: E731
        a, b = quad_box(mv(rect), 2.0, 0.0), quad_box(mv(diamond), 1.5, 0.5)
        out.append((a, b) if i % 2 == 0 else (b, a))
    return out


def mirrored(corners):
    """The same box with its corners in the opposite (clockwise) order: corners 1 and 3 (and 5 and 7) swapped."""
    return np.ascontiguousarray(corners[:, [0, 3, 2, 1, 4, 7, 6, 5]])


def box_iou_pairs(seed=20240521, n=1.0):
    """-> (names, corners_1 (M, 3, 8), corners_t (M, 3, 8)) float32: every family of the box_iou_3d fuzz."""
    names, c1, ct = [], [], []
    for fam, pairs in box_pair_families(seed, n).items():
        for p in pairs:
            a, b = pair_corners(p)
            names.append(fam); c1.append(a); ct.append(b)
    for a, b in vertex_on_edge_pairs(n=max(int(200 * n), 10)):
        names.append('vertex_on_edge'); c1.append(a); ct.append(b)
    rng = np.random.default_rng(seed + 1)
    base = len(names)
    for i in rng.choice(base, size=max(int(300 * n), 8), replace=False):                # clockwise against counter-clockwise
        names.append('mirrored'); c1.append(mirrored(c1[i])); ct.append(ct[i] if i % 2 else mirrored(ct[i]))
    for i in rng.choice(base, size=max(int(100 * n), 4), replace=False):                # bit-identical boxes
        names.append('identical'); c1.append(c1[i]); ct.append(c1[i].copy())
    return names, np.stack(c1), np.stack(ct)


def camera_box(box):
    """(x, y, z, l, h, w, ry) of the KITTI camera format; its BEV rbox is (x, z, l, w, ry)."""
    (x, y, z), a, (l, w, h) = box
    return [x, y, z, l, h, w, a]


def overlap_boxes(seed=20240522, per_family=18):
    """-> (boxes (N, 7), query_boxes (N, 7)) fp64: pair i of every parametric family sits on the diagonal (box i, query i)."""
    b, q = [], []
    for fam, pairs in box_pair_families(seed, 0.2).items():
        for p in pairs[:per_family]:
            b.append(camera_box(p[0])); q.append(camera_box(p[1]))
    return np.array(b, dtype=np.float64), np.array(q, dtype=np.float64)


def bev(boxes):
    return np.ascontiguousarray(np.asarray(boxes)[:, [0, 2, 3, 5, 6]], dtype=np.float32)
