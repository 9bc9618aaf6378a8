"""The definition of the KITTI frame store (include/pvcnn_hip.h "KITTI frame store", pvcnn_amd/frame_store.py) restated in plain numpy on
top of tests/frames_truth.py: elementwise fp64 expressions in the stated order, one rounding per operation, no BLAS.  The kernel is held
to this bit for bit in parity mode; tests/test_frame_store_host.py proves it against closed forms and pvcnn_amd.data.angle_to_bin_id.
Nothing of this stage exists in the reference (the original preparation script is another project's), so no golden file stands behind it."""
import numpy as np

import frames_truth as ft

PARAMS = 12


def random_shift_box2d(box, u, shift_ratio=0.1):
    """One box (xmin, ymin, xmax, ymax) and its four uniforms -> the perturbed box, (4,) fp64."""
    xmin, ymin, xmax, ymax = (np.float64(a) for a in box)
    u0, u1, u2, u3 = (np.float64(a) for a in u)
    r = np.float64(shift_ratio)
    w, h, cx, cy = xmax - xmin, ymax - ymin, (xmin + xmax) / 2, (ymin + ymax) / 2
    cx2, cy2 = cx + (w * r) * (u0 * 2 - 1), cy + (h * r) * (u1 * 2 - 1)
    h2, w2 = h * ((1 + (u2 * 2) * r) - r), w * ((1 + (u3 * 2) * r) - r)
    return np.array([cx2 - w2 / 2, cy2 - h2 / 2, cx2 + w2 / 2, cy2 + h2 / 2], dtype=np.float64)


def floor_mod(x, m):
    """numpy's % written out: fmod, then the divisor added when the remainder is non-zero and of the other sign."""
    r = np.fmod(np.float64(x), np.float64(m))
    if r == 0:
        return np.float64(0.0)
    return r + m if (r < 0) != (m < 0) else r


def angle_to_bin(angle, num_angle_bins):
    """(bin id, fp64 residual) as pvcnn_amd.data.angle_to_bin_id."""
    two_pi = 2 * np.pi
    a = floor_mod(angle, two_pi)
    per_bin = two_pi / float(num_angle_bins)
    shifted = floor_mod(a + per_bin / 2, two_pi)
    bin_id = int(shifted / per_bin)
    return bin_id, shifted - (bin_id * per_bin + per_bin / 2)


def rotation_angle(P, box):
    return np.pi / 2.0 + ft.frustum_angle(P, box)


def params_row(P, box, u, shift_ratio=0.1):
    """The parity row of one sample: the uniforms, the perturbed box, its rotation angle, cos, sin, zero."""
    pbox = random_shift_box2d(box, u, shift_ratio)
    angle = rotation_angle(P, pbox)
    return np.concatenate([np.asarray(u, dtype=np.float64), pbox, [angle, np.cos(angle), np.sin(angle), 0.0]])


def accepted(box, positives, min_box_height=25):
    """The original's rule for a perturbed box: still high enough, still one point of the object."""
    return bool(float(box[3]) - float(box[1]) >= min_box_height and positives > 0)


def frame_points(scan, P, R0, V2C, image_size, clip_distance=2.0):
    """What the store keeps of a frame: (rows (n, 4) fp32, uv (n, 2) fp64) of its in-image points, ascending point index."""
    rows, uv, seen = ft.project(scan, P, R0, V2C, image_size, clip_distance)
    return rows[seen], uv[seen]


def select(points, box, box_3d):
    """(selected (n,) bool, positive (n,) bool) of a 2-D box over the stored points of a frame."""
    rows, uv = points
    sel = ft.in_box(uv, np.ones(len(rows), dtype=bool), box)
    return sel, sel & ft.in_box_3d(rows, box_3d)


def admitted(points, box, box_3d, min_box_height=25):
    return accepted(box, int(select(points, box, box_3d)[1].sum()), min_box_height)


def box_used(points, P, box, box_3d, row, shift_ratio=0.1, min_box_height=25):
    """-> (used, box, rotation angle, cos, sin, why): the perturbed box of `row` if it passes the rule, else the item's own box with the
    host's angle; why is 'accepted', 'low', 'lost' (no positive point left) or 'off' (shift_ratio == 0)."""
    own = np.asarray(box, dtype=np.float64)
    angle = rotation_angle(P, own)
    fallback = (0, own, angle, np.cos(angle), np.sin(angle))
    if shift_ratio == 0:
        return fallback + ('off',)
    pbox = np.asarray(row[4:8], dtype=np.float64)
    if not float(pbox[3]) - float(pbox[1]) >= min_box_height:
        return fallback + ('low',)
    if not select(points, pbox, box_3d)[1].any():
        return fallback + ('lost',)
    return 1, pbox, np.float64(row[8]), np.float64(row[9]), np.float64(row[10]), 'accepted'


def sample(points, P, item, row, choices, flip, shift, *, num_heading_angle_bins=12, frustum_rotate=False, random_flip=False,
           random_shift=False, shift_ratio=0.1, min_box_height=25):
    """One sample.  item: dict(box (4,), box_3d (7,) h w l x y z ry, one_hot (K,), size_residual (3,) fp32, size_template_id, class_id).
    choices (N,) positions among the selected points (clamped); flip, shift: the fp64 draws.  -> dict of the batch's rows + 'used'."""
    rows = points[0]
    used, box, angle, c, s, _ = box_used(points, P, item['box'], item['box_3d'], row, shift_ratio, min_box_height)
    sel, pos = select(points, box, item['box_3d'])
    k = int(sel.sum())
    pick = np.clip(np.asarray(choices, dtype=np.int64), 0, k - 1)
    pts = rows[sel][pick].copy()
    label = pos[sel][pick].astype(np.int64)
    corners = ft.corners(item['box_3d'])
    centre = (corners[0, :] + corners[6, :]) / 2.0
    heading = np.float64(item['box_3d'][6])
    if frustum_rotate:
        x, z = pts[:, 0].astype(np.float64), pts[:, 2].astype(np.float64)
        pts[:, 0] = (x * c + z * (-s)).astype(np.float32)
        pts[:, 2] = (x * s + z * c).astype(np.float32)
        centre = np.array([centre[0] * c + centre[2] * (-s), centre[1], centre[0] * s + centre[2] * c])
        heading = heading - angle
    dist = np.sqrt(centre[0] * centre[0] + centre[1] * centre[1])
    flipped = bool(random_flip and flip > 0.5)
    if flipped:
        pts[:, 0] = -pts[:, 0]
        centre[0] = -centre[0]
        heading = np.pi - heading
    if random_shift:
        move = np.minimum(np.maximum(np.float64(shift) * dist * 0.05, dist * 0.8), dist * 1.2)
        pts[:, 2] = (pts[:, 2].astype(np.float64) + move).astype(np.float32)
        centre[2] = centre[2] + move
    bin_id, residual = angle_to_bin(heading, num_heading_angle_bins)
    return {'features': np.ascontiguousarray(pts.T), 'one_hot_vectors': np.asarray(item['one_hot'], dtype=np.float32),
            'mask_logits': label, 'center': centre.astype(np.float32), 'heading_bin_id': np.int64(bin_id),
            'heading_residual': np.float32(residual), 'size_template_id': np.int64(item['size_template_id']),
            'size_residual': np.asarray(item['size_residual'], dtype=np.float32), 'class_id': np.int64(item['class_id']),
            'used': np.int32(used)}


def batch(samples):
    """Stack `sample` results: name -> (B, ...) array."""
    return {k: np.stack([np.asarray(s[k]) for s in samples]) for k in samples[0]}
