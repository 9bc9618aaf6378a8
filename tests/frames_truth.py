"""The definition of the KITTI frame stage (include/pvcnn_hip.h "KITTI frames", pvcnn_amd/frames.py) restated in plain numpy: elementwise
fp64 expressions in the stated order, one rounding per operation, no BLAS (np.dot's summation order and use of fused multiply-adds are
not ours to know).  The kernels are held to this bit for bit; tests/test_frames_host.py proves it against closed forms.  Nothing of
this stage exists in the reference, so there is no golden file behind it."""
import numpy as np


def project(scan, P, R0, V2C, image_size, clip_distance=2.0):
    """scan (N, 4) fp32 -> (rows (N, 4) fp32, uv (N, 2) fp64, in_image (N,) bool)."""
    scan = np.asarray(scan, dtype=np.float32).reshape(-1, 4)
    P, R0, V2C = (np.asarray(a, dtype=np.float64) for a in (P, R0, V2C))
    width, height = image_size
    x, y, z = (scan[:, c].astype(np.float64) for c in range(3))
    ref = [((V2C[i, 0] * x + V2C[i, 1] * y) + V2C[i, 2] * z) + V2C[i, 3] for i in range(3)]
    rect = [(R0[i, 0] * ref[0] + R0[i, 1] * ref[1]) + R0[i, 2] * ref[2] for i in range(3)]
    img = [((P[i, 0] * rect[0] + P[i, 1] * rect[1]) + P[i, 2] * rect[2]) + P[i, 3] for i in range(3)]
    with np.errstate(divide='ignore', invalid='ignore'):
        u, v = img[0] / img[2], img[1] / img[2]
        in_image = (u >= 0) & (u < width) & (v >= 0) & (v < height) & (x > clip_distance)
    rows = np.stack([rect[0].astype(np.float32), rect[1].astype(np.float32), rect[2].astype(np.float32), scan[:, 3]], axis=1)
    return rows, np.stack([u, v], axis=1), in_image


def in_box(uv, in_image, box_2d):
    """(N,) bool: the points of 2-D box (xmin, ymin, xmax, ymax)."""
    xmin, ymin, xmax, ymax = (float(a) for a in box_2d)
    u, v = uv[:, 0], uv[:, 1]
    with np.errstate(invalid='ignore'):
        return in_image & (u >= xmin) & (u < xmax) & (v >= ymin) & (v < ymax)


def in_box_3d(rows, box_3d):
    """(N,) bool: stored fp32 rows inside the 3-D box (h, w, l, tx, ty, tz, ry), faces included; cos and sin from the host."""
    h, w, l, tx, ty, tz, ry = (float(a) for a in box_3d)
    c, s = np.cos(ry), np.sin(ry)
    dx = rows[:, 0].astype(np.float64) - tx
    dy = rows[:, 1].astype(np.float64) - ty
    dz = rows[:, 2].astype(np.float64) - tz
    xl = c * dx - s * dz
    zl = s * dx + c * dz
    return (np.abs(xl) <= l / 2) & (np.abs(zl) <= w / 2) & (dy <= 0) & (dy >= -h)


def frustum_angle(P, box_2d):
    P = np.asarray(P, dtype=np.float64)
    cu = (float(box_2d[0]) + float(box_2d[2])) / 2
    x = ((cu - P[0, 2]) * 20) / P[0, 0] + P[0, 3] / (-P[0, 0])
    return -np.arctan2(20.0, x)


def corners(box_3d):
    """(8, 3) fp64 corners of (h, w, l, tx, ty, tz, ry) in the original's order."""
    h, w, l, tx, ty, tz, ry = (float(a) for a in box_3d)
    xs = np.array([l / 2, l / 2, -l / 2, -l / 2, l / 2, l / 2, -l / 2, -l / 2])
    ys = np.array([0, 0, 0, 0, -h, -h, -h, -h], dtype=np.float64)
    zs = np.array([w / 2, -w / 2, -w / 2, w / 2, w / 2, -w / 2, -w / 2, w / 2])
    c, s = np.cos(ry), np.sin(ry)
    return np.stack([(c * xs + s * zs) + tx, ys + ty, (-s * xs + c * zs) + tz], axis=1)


def rotate_rows(rows, rotation_angle):
    """rows (n, 4) fp32 rotated to the frustum centre: fp64 from the fp32 row, rounded once."""
    c, s = np.cos(rotation_angle), np.sin(rotation_angle)
    x, z = rows[:, 0].astype(np.float64), rows[:, 2].astype(np.float64)
    out = rows.copy()
    out[:, 0] = (x * c + z * (-s)).astype(np.float32)
    out[:, 2] = (x * s + z * c).astype(np.float32)
    return out


def keep(box_2d, count, positives=None, min_box_height=25, min_points=5):
    """The original's rules: with ground truth (positives given) a box at least min_box_height high with one positive point; without,
    at least min_box_height high with at least min_points points."""
    tall = float(box_2d[3]) - float(box_2d[1]) >= min_box_height
    if positives is not None:
        return bool(tall and positives > 0)
    return bool(tall and count >= min_points and count > 0)


def extract(scan, P, R0, V2C, boxes_2d, image_size, boxes_3d=None, min_box_height=25, min_points=5, clip_distance=2.0):
    """-> dict: kept, offsets, rows, labels (None without boxes_3d), counts (M, 2), frustum_angles (kept), uv, in_image, all_rows."""
    rows, uv, in_image = project(scan, P, R0, V2C, image_size, clip_distance)
    boxes_2d = np.asarray(boxes_2d, dtype=np.float64).reshape(-1, 4)
    kept, out_rows, out_labels, counts = [], [], [], []
    for m, box in enumerate(boxes_2d):
        sel = in_box(uv, in_image, box)
        label = (in_box_3d(rows, boxes_3d[m]) & sel) if boxes_3d is not None else None
        counts.append((int(sel.sum()), int(label.sum()) if label is not None else 0))
        if keep(box, counts[-1][0], counts[-1][1] if label is not None else None, min_box_height, min_points):
            kept.append(m)
            out_rows.append(rows[sel])                # boolean indexing: ascending point index
            if label is not None:
                out_labels.append(label[sel].astype(np.uint8))
    offsets = np.zeros(len(kept) + 1, dtype=np.int64)
    if kept:
        np.cumsum([len(r) for r in out_rows], out=offsets[1:])
    return {'kept': np.asarray(kept, dtype=np.int64), 'offsets': offsets,
            'rows': np.concatenate(out_rows) if kept else np.zeros((0, 4), dtype=np.float32),
            'labels': None if boxes_3d is None else (np.concatenate(out_labels) if kept else np.zeros((0,), dtype=np.uint8)),
            'counts': np.asarray(counts, dtype=np.int64).reshape(-1, 2),
            'frustum_angles': np.asarray([frustum_angle(P, boxes_2d[m]) for m in kept], dtype=np.float64),
            'uv': uv, 'in_image': in_image, 'all_rows': rows}


def batch(scan, P, R0, V2C, boxes_2d, image_size, class_ids, scores, choices, num_points, num_classes=3, frustum_rotate=True, bmax=None,
          min_box_height=25, min_points=5, clip_distance=2.0):
    """Parity-mode `frame_batch`: choices (M, num_points) positions among every box's selected points (clamped to [0, k))."""
    rows, uv, in_image = project(scan, P, R0, V2C, image_size, clip_distance)
    boxes_2d = np.asarray(boxes_2d, dtype=np.float64).reshape(-1, 4)
    m_boxes = len(boxes_2d)
    bmax = m_boxes if bmax is None else bmax
    features = np.zeros((bmax, 4, num_points), dtype=np.float32)
    one_hot = np.zeros((bmax, num_classes), dtype=np.float32)
    rotation_angle = np.zeros((bmax,), dtype=np.float32)
    rgb_score = np.zeros((bmax,), dtype=np.float64)
    valid = np.zeros((bmax,), dtype=np.uint8)
    for m, box in enumerate(boxes_2d):
        sel = in_box(uv, in_image, box)
        k = int(sel.sum())
        if not keep(box, k, None, min_box_height, min_points):
            continue
        angle = np.pi / 2.0 + frustum_angle(P, box)
        cloud = rows[sel]
        if frustum_rotate:
            cloud = rotate_rows(cloud, angle)
        pick = np.clip(np.asarray(choices[m], dtype=np.int64), 0, k - 1)
        features[m] = cloud[pick].T
        one_hot[m, int(class_ids[m])] = 1
        rotation_angle[m] = np.float32(angle)
        rgb_score[m] = scores[m]
        valid[m] = 1
    return features, one_hot, rotation_angle, rgb_score, valid
