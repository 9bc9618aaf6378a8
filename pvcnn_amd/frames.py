"""KITTI frames on the device: a LiDAR sweep, a calibration and 2-D boxes -> frustums (csrc/frames.hip).

Reference: datasets/kitti/frustum.py only reads `frustum_carpedcyc_{split}[_rgb_detection].pickle`; the reference cannot produce these
files (it points to frustum-pointnets' prepare_data.py), so nothing in it goes from a sweep to a 3-D box.  This module is that stage:

    extract_frustums      one frame -> the packed frustums of its boxes (what the pickles hold), for `DeviceFrustumKitti.from_frustums`
    frame_batch           one frame -> the batch one iteration of the rgb-detection loader yields, with no device-to-host copy
    detect_frame          frame_batch -> model -> `kitti.frustum_box_predictions`: an (M, 8) table of 3-D boxes
    kitti_label_lines     the table -> the lines evaluate/kitti/frustum/eval.py:254-256 writes (host only)
    random_shift_box2d    the original's training-time perturbation of 2-D boxes (host only; per sample on the device: frame_store.py)

The definition (projection, image and box tests, the label, the rotation; include/pvcnn_hip.h, "KITTI frames") is fp64 with one
rounding per operation; tests/frames_truth.py restates it in numpy and the kernels are held to it bit for bit.  Everything that needs a
trigonometric function is a per-box scalar, computed here on the host in numpy fp64 and uploaded with the boxes in one table
(`box_table`).  The label is the box-frame form of the original's hull test: NOT scipy's Delaunay hull -- the two can differ only for
points within rounding of a face of the box.

Host synchronisation: `extract_frustums` makes exactly one device-to-host copy, the (M, 2) counts that size the packed outputs;
`frame_batch` makes none; `detect_frame` makes one, its result.  All of them go through `_read`, which counts them (`copies_made()`).

The product path needs device tensors (or numpy arrays, uploaded once) and the native library: there is no CPU implementation.
"""
import numpy as np
import torch

from . import _lib
from .modules.functional.backend import _device_call as _call, check_seed, fresh_seed

__all__ = ['Calibration', 'FrameFrustums', 'read_scan', 'frustum_angle', 'random_shift_box2d', 'box_corners', 'box_table', 'project_scan',
           'extract_frustums', 'frame_batch', 'detect_frame', 'kitti_label_lines', 'copies_made', 'BOX_COLUMNS']

BOX_COLUMNS = 18                     # PVCNN_FRAME_BOX_COLUMNS
MAX_BOXES = 4096                     # PVCNN_FRAME_MAX_BOXES
_copies = 0


def copies_made():
    """Device-to-host copies this module has made so far (every one goes through `_read`)."""
    return _copies


def _read(t):
    """The one place this module reads device memory on the host."""
    global _copies
    _copies += 1
    return t.cpu().numpy()


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError('KITTI frames need a GPU and the native library -- there is no CPU implementation')
    return torch.device('cuda', torch.cuda.current_device())


class Calibration:
    """P (3, 4) the camera's projection, R0 (3, 3) the rectifying rotation, V2C (3, 4) velodyne -> camera: numpy fp64, and a cached
    device copy (33 doubles: P, V2C, R0)."""

    def __init__(self, P, R0, V2C):
        self.P = np.ascontiguousarray(np.asarray(P, dtype=np.float64).reshape(3, 4))
        self.R0 = np.ascontiguousarray(np.asarray(R0, dtype=np.float64).reshape(3, 3))
        self.V2C = np.ascontiguousarray(np.asarray(V2C, dtype=np.float64).reshape(3, 4))
        self._device_copy = {}

    @classmethod
    def from_file(cls, path):
        """A KITTI object calib file: the lines `P2:`, `R0_rect:` and `Tr_velo_to_cam:`."""
        rows = {}
        with open(path, 'r') as f:
            for line in f:
                key, sep, values = line.partition(':')
                if sep and values.strip():
                    rows[key.strip()] = values.split()
        missing = [k for k in ('P2', 'R0_rect', 'Tr_velo_to_cam') if k not in rows]
        if missing:
            raise ValueError(f'{path}: no line {missing[0]}:')
        return cls([float(v) for v in rows['P2']], [float(v) for v in rows['R0_rect']], [float(v) for v in rows['Tr_velo_to_cam']])

    def packed(self):
        """(33,) fp64: P, V2C, R0 row-major, the kernels' layout."""
        return np.concatenate([self.P.reshape(-1), self.V2C.reshape(-1), self.R0.reshape(-1)])

    def device(self, device):
        key = str(device)
        if key not in self._device_copy:
            self._device_copy[key] = torch.from_numpy(self.packed()).to(device)
        return self._device_copy[key]


def read_scan(path):
    """A KITTI velodyne .bin -> (N, 4) fp32 numpy (x, y, z, reflectance)."""
    return np.fromfile(path, dtype=np.float32).reshape(-1, 4)


def frustum_angle(calib, boxes_2d):
    """(M,) fp64: the original's frustum angle of every 2-D box (xmin, ymin, xmax, ymax): the box centre's column back-projected at
    depth 20, -arctan2(20, X) with X = ((cu - P[0,2]) * 20) / P[0,0] + P[0,3] / (-P[0,0])."""
    boxes_2d = np.asarray(boxes_2d, dtype=np.float64).reshape(-1, 4)
    P = calib.P
    cu = (boxes_2d[:, 0] + boxes_2d[:, 2]) / 2
    x = ((cu - P[0, 2]) * 20) / P[0, 0] + P[0, 3] / (-P[0, 0])
    return -np.arctan2(np.full_like(x, 20.0), x)


def random_shift_box2d(boxes_2d, draws, shift_ratio=0.1):
    """(M, 4) fp64: the original's training-time perturbation of 2-D boxes (xmin, ymin, xmax, ymax) -- the centre shifted by up to
    shift_ratio of the box's size, width and height rescaled by 1 -+ shift_ratio -- for `draws` (M, 4) uniforms in [0, 1), in the
    original's order: centre x, centre y, height, width.  The definition is include/pvcnn_hip.h's ("KITTI frame store"), elementwise
    fp64; the rows of `DeviceKittiFrames`' parity `params` are built with it, and with `extract_frustums` on its result the original's
    frozen `augmentX` copies can be made.  shift_ratio == 0 returns the boxes as they are."""
    boxes = np.asarray(boxes_2d, dtype=np.float64).reshape(-1, 4)
    u = np.asarray(draws, dtype=np.float64).reshape(-1, 4)
    if u.shape[0] != boxes.shape[0]:
        raise ValueError('four draws per box expected')
    r = float(shift_ratio)
    if r == 0.0:
        return boxes.copy()
    xmin, ymin, xmax, ymax = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
    w, h, cx, cy = xmax - xmin, ymax - ymin, (xmin + xmax) / 2, (ymin + ymax) / 2
    cx2, cy2 = cx + (w * r) * (u[:, 0] * 2 - 1), cy + (h * r) * (u[:, 1] * 2 - 1)
    h2, w2 = h * ((1 + (u[:, 2] * 2) * r) - r), w * ((1 + (u[:, 3] * 2) * r) - r)
    return np.stack([cx2 - w2 / 2, cy2 - h2 / 2, cx2 + w2 / 2, cy2 + h2 / 2], axis=1)


def box_corners(boxes_3d):
    """(M, 8, 3) fp64 corners of 3-D boxes (h, w, l, x, y, z, ry) in the rectified camera frame, in the original's order:
    x = +-l/2 (+ + - - + + - -), y = (0 0 0 0 -h -h -h -h), z = (+ - - + + - - +) w/2, rotated about y by ry, shifted by (x, y, z).
    Corners 0 and 6 average to the box centre (datasets/kitti/frustum.py:120)."""
    b = np.asarray(boxes_3d, dtype=np.float64).reshape(-1, 7)
    h, w, l, ry = b[:, 0:1], b[:, 1:2], b[:, 2:3], b[:, 6:7]
    x = l / 2 * np.array([1, 1, -1, -1, 1, 1, -1, -1], dtype=np.float64)
    y = -h * np.array([0, 0, 0, 0, 1, 1, 1, 1], dtype=np.float64)
    z = w / 2 * np.array([1, -1, -1, 1, 1, -1, -1, 1], dtype=np.float64)
    c, s = np.cos(ry), np.sin(ry)
    return np.stack([(c * x + s * z) + b[:, 3:4], y + b[:, 4:5], (-s * x + c * z) + b[:, 5:6]], axis=2)


def box_table(calib, boxes_2d, class_ids=None, scores=None, boxes_3d=None):
    """(M, BOX_COLUMNS) fp64 numpy: the kernels' box table (include/pvcnn_hip.h), every angle-dependent scalar computed here."""
    boxes_2d = np.asarray(boxes_2d, dtype=np.float64).reshape(-1, 4)
    m = boxes_2d.shape[0]
    if m > MAX_BOXES:
        raise ValueError(f'at most {MAX_BOXES} boxes per frame')
    t = np.zeros((m, BOX_COLUMNS), dtype=np.float64)
    t[:, 0:4] = boxes_2d
    if boxes_3d is not None:
        b = np.asarray(boxes_3d, dtype=np.float64).reshape(-1, 7)
        if b.shape[0] != m:
            raise ValueError('one 3-D box (h, w, l, x, y, z, ry) per 2-D box expected')
        t[:, 4] = 1
        t[:, 5:11] = b[:, 0:6]
        t[:, 11], t[:, 12] = np.cos(b[:, 6]), np.sin(b[:, 6])
    rotation = np.pi / 2.0 + frustum_angle(calib, boxes_2d)
    t[:, 13], t[:, 14], t[:, 15] = np.cos(rotation), np.sin(rotation), rotation
    if class_ids is not None:
        t[:, 16] = np.asarray(class_ids, dtype=np.float64).reshape(m)
    if scores is not None:
        t[:, 17] = np.asarray(scores, dtype=np.float64).reshape(m)
    return t


def _device_scan(scan):
    """(cap, 4) fp32 on the device: a device tensor as it is, a numpy array uploaded once."""
    if isinstance(scan, torch.Tensor):
        if scan.device.type != 'cuda':
            raise RuntimeError('KITTI frames need a CUDA (HIP) tensor or a numpy array -- there is no CPU implementation')
        x = scan
    else:
        x = torch.from_numpy(np.ascontiguousarray(scan, dtype=np.float32)).to(_device())
    if x.dim() != 2 or x.shape[1] != 4 or x.shape[0] < 1 or x.dtype != torch.float32:
        raise ValueError(f'scan (N, 4) float32 with N >= 1 expected, got {tuple(x.shape)} {x.dtype}')
    return x.contiguous()


def _device_table(calib, boxes_2d, class_ids, scores, boxes_3d, device):
    """The box table on the device: a prepared (M, BOX_COLUMNS) fp64 device tensor as it is (nothing is uploaded: a captured graph
    reads the tensor it was captured with), host boxes through `box_table`."""
    if isinstance(boxes_2d, torch.Tensor) and boxes_2d.device.type == 'cuda':
        if boxes_2d.dim() != 2 or boxes_2d.shape[1] != BOX_COLUMNS or boxes_2d.dtype != torch.float64 or not boxes_2d.is_contiguous():
            raise ValueError(f'a device box table is a contiguous (M, {BOX_COLUMNS}) float64 tensor (box_table)')
        return boxes_2d
    if isinstance(boxes_2d, torch.Tensor):
        boxes_2d = boxes_2d.numpy()
    return torch.from_numpy(box_table(calib, boxes_2d, class_ids, scores, boxes_3d)).to(device)


def _count_word(count, device):
    if count is None:
        return None
    if not isinstance(count, torch.Tensor) or count.dtype != torch.int32 or count.numel() != 1 or count.device != device:
        raise ValueError('count = one int32 word on the scan\'s device')
    return count


def _project(x, calib, image_size, clip_distance, count):
    width, height = image_size
    cap, dev = x.shape[0], x.device
    rows = torch.empty((cap, 4), dtype=torch.float32, device=dev)
    uv = torch.empty((cap, 2), dtype=torch.float64, device=dev)
    in_image = torch.empty((cap,), dtype=torch.uint8, device=dev)
    _call('frame_project', x, x, cap, cap, _count_word(count, dev), calib.device(dev), float(width), float(height), float(clip_distance),
          rows, uv, in_image)
    return rows, uv, in_image


def _count(rows, uv, in_image, table, with_labels):
    cap, dev, m = rows.shape[0], rows.device, table.shape[0]
    tiles = _lib.load().pvcnn_frame_tiles(cap)
    mask = torch.empty((m, tiles), dtype=torch.int64, device=dev)
    label_mask = torch.empty((m, tiles), dtype=torch.int64, device=dev) if with_labels else None
    prefix = torch.empty((m, tiles + 1), dtype=torch.int32, device=dev)
    counts = torch.empty((m, 2), dtype=torch.int32, device=dev)
    _call('frame_count', rows, uv, in_image, rows, cap, table, m, mask, label_mask, prefix, counts)
    return mask, label_mask, prefix, counts


def project_scan(scan, calib, image_size, *, clip_distance=2.0, count=None):
    """The projection launch alone -> (rows (cap, 4) fp32: rectified camera coordinates and reflectance, uv (cap, 2) fp64,
    in_image (cap,) uint8), on the device.  image_size = (width, height)."""
    return _project(_device_scan(scan), calib, image_size, clip_distance, count)


class FrameFrustums:
    """The kept frustums of one frame, packed like `data._Store`: item w owns rows offsets[w] .. offsets[w + 1].
    On the device: rows (R, 4) fp32 (the pickle's `point_clouds`), labels (R,) uint8 or None (`mask_logits`), offsets (W + 1,) int64,
    kept (W,) int64 (indices into the input boxes).
    On the host, one entry per item: class_names, boxes_2d (W, 4), frustum_angles (W,), counts (W,); with ground truth boxes_3d
    (W, 8, 3) corners, heading_angles (W,), sizes (W, 3) = (l, w, h); without, scores (W,)."""

    def __init__(self, rows, labels, offsets, kept, class_names, boxes_2d, frustum_angles, counts, boxes_3d=None, heading_angles=None,
                 sizes=None, scores=None):
        self.rows, self.labels, self.offsets, self.kept = rows, labels, offsets, kept
        self.class_names, self.boxes_2d, self.frustum_angles, self.counts = list(class_names), boxes_2d, frustum_angles, counts
        self.boxes_3d, self.heading_angles, self.sizes, self.scores = boxes_3d, heading_angles, sizes, scores
        self.device = rows.device

    def __len__(self):
        return len(self.class_names)

    def item(self, w):
        """(rows (n, 4) fp32, labels (n,) uint8 or None) of item w, on the device."""
        a, b = int(self.counts[:w].sum()), int(self.counts[:w + 1].sum())
        return self.rows[a:b], None if self.labels is None else self.labels[a:b]


def extract_frustums(scan, calib, boxes_2d, image_size, *, classes, boxes_3d=None, scores=None, min_box_height=25, min_points=None,
                     clip_distance=2.0):
    """The frustums of one frame.  scan (N, 4) fp32 (device tensor, or numpy uploaded once); boxes_2d (M, 4) xmin, ymin, xmax, ymax;
    image_size (width, height); classes: the M class names; boxes_3d (M, 7) h, w, l, x, y, z, ry in the rectified camera frame, or None.
    With boxes_3d a box is kept iff ymax - ymin >= min_box_height and it has at least one positive point (the original's rule for
    ground truth); without, iff ymax - ymin >= min_box_height and count >= min_points (default 5: its rgb-detection rule).
    One device-to-host copy: the (M, 2) counts.  -> FrameFrustums."""
    x = _device_scan(scan)
    dev = x.device
    boxes = np.asarray(boxes_2d, dtype=np.float64).reshape(-1, 4)
    m = boxes.shape[0]
    classes = list(classes)
    if len(classes) != m:
        raise ValueError('one class name per box expected')
    if m == 0:
        raise ValueError('a frame without boxes has no frustums')
    truth = boxes_3d is not None
    if truth:
        b3 = np.asarray(boxes_3d, dtype=np.float64).reshape(-1, 7)
        if min_points is not None:
            raise ValueError('min_points is the rule without ground truth; with boxes_3d a box needs one positive point')
    else:
        min_points = 5 if min_points is None else int(min_points)
        scores = np.ones(m) if scores is None else np.asarray(scores, dtype=np.float64).reshape(m)
    table = torch.from_numpy(box_table(calib, boxes, None, None if truth else scores, boxes_3d)).to(dev)
    rows, uv, in_image = _project(x, calib, image_size, clip_distance, None)
    mask, label_mask, prefix, counts = _count(rows, uv, in_image, table, truth)
    n = _read(counts).astype(np.int64)
    tall = (boxes[:, 3] - boxes[:, 1]) >= min_box_height
    keep = tall & ((n[:, 1] > 0) if truth else ((n[:, 0] >= min_points) & (n[:, 0] > 0)))
    kept = np.nonzero(keep)[0].astype(np.int64)
    offsets = np.zeros(kept.size + 1, dtype=np.int64)
    np.cumsum(n[kept, 0], out=offsets[1:])
    total = int(offsets[-1])
    out_rows = torch.empty((total, 4), dtype=torch.float32, device=dev)
    out_labels = torch.empty((total,), dtype=torch.uint8, device=dev) if truth else None
    kept_dev, offsets_dev = torch.from_numpy(kept).to(dev), torch.from_numpy(offsets).to(dev)
    if kept.size and total:
        _call('frame_pack', rows, rows, x.shape[0], mask, label_mask, prefix, m, kept_dev, offsets_dev, kept.size, total, out_rows,
              out_labels)
    angles = frustum_angle(calib, boxes)
    if truth:
        extra = dict(boxes_3d=box_corners(b3)[kept], heading_angles=b3[kept, 6].copy(), sizes=b3[kept][:, [2, 1, 0]].copy())
    else:
        extra = dict(scores=scores[kept].copy())
    return FrameFrustums(out_rows, out_labels, offsets_dev, kept_dev, [classes[i] for i in kept], boxes[kept].copy(), angles[kept],
                         n[kept, 0].copy(), **extra)


def _empty_batch(bmax, num_points, k, dev):
    f = torch.float32
    return ({'features': torch.empty((bmax, 4, num_points), dtype=f, device=dev), 'one_hot_vectors': torch.empty((bmax, k), dtype=f, device=dev)},
            {'rotation_angle': torch.empty((bmax,), dtype=f, device=dev), 'rgb_score': torch.empty((bmax,), dtype=torch.float64, device=dev)},
            torch.empty((bmax,), dtype=torch.uint8, device=dev))


def frame_batch(scan, calib, boxes_2d, image_size, class_ids=None, *, num_points=1024, frustum_rotate=True, scores=None, out=None,
                count=None, choices=None, seed=None, num_classes=3, min_box_height=25, min_points=5, clip_distance=2.0):
    """What one iteration of the rgb-detection loader yields for the boxes of one frame, straight from the scan: (inputs
    {'features' (B, 4, num_points), 'one_hot_vectors' (B, num_classes)}, targets {'rotation_angle' (B,) fp32, 'rgb_score' (B,) fp64},
    valid (B,) uint8), B = M or the rows of `out`.  No device-to-host copy; a plain chain of four launches, capturable:
      out     static tensors of Bmax >= M rows, the structure this function returns; rows of boxes that are too low
              (ymax - ymin < min_box_height) or hold fewer than min_points points, and rows m >= M, are all zero with valid = 0;
      count   a device int32 word: the scan holds count[0] points in a larger static buffer;
      boxes_2d  host boxes (M, 4) with class_ids (M,) and scores (M,), or a prepared device table (`box_table`, uploaded by the
              caller: a captured graph reads that tensor, so new boxes are copied into it);
      choices (M, num_points) int32 positions among a box's selected points (parity mode: numpy's draws), else a Philox stream
              keyed by `seed` (two int64 device words; default: drawn from torch's device generator)."""
    x = _device_scan(scan)
    dev = x.device
    table = _device_table(calib, boxes_2d, class_ids, scores, None, dev)
    m, num_points, k = table.shape[0], int(num_points), int(num_classes)
    if num_points < 1 or k < 1:
        raise ValueError('num_points >= 1 and num_classes >= 1 expected')
    if out is None:
        out = _empty_batch(m, num_points, k, dev)
    inputs, targets, valid = out
    bmax = valid.shape[0]
    want = _empty_batch(0, num_points, k, dev)
    for got, like in ((inputs, want[0]), (targets, want[1])):
        for name, t in like.items():
            o = got[name]
            if tuple(o.shape) != (bmax,) + tuple(t.shape[1:]) or o.dtype != t.dtype or o.device != dev or not o.is_contiguous():
                raise ValueError(f'out[{name}]: contiguous {t.dtype} tensor of shape {(bmax,) + tuple(t.shape[1:])} on {dev} expected')
    if bmax < m or valid.dtype != torch.uint8 or valid.device != dev:
        raise ValueError(f'out: at least {m} rows and a uint8 valid mask on {dev} expected')
    if choices is not None:
        choices = torch.as_tensor(choices).to(device=dev, dtype=torch.int32).contiguous()
        if tuple(choices.shape) != (m, num_points):
            raise ValueError(f'choices of shape {(m, num_points)} expected, got {tuple(choices.shape)}')
        seed = None
    else:
        seed = fresh_seed(dev) if seed is None else check_seed(seed, dev)
    rows, uv, in_image = _project(x, calib, image_size, clip_distance, count)
    if m:
        mask, _, prefix, counts = _count(rows, uv, in_image, table, False)
    else:
        mask = prefix = counts = None
    _call('frame_batch', rows, rows, x.shape[0], mask, prefix, counts, table if m else None, m, bmax, num_points, k, int(bool(frustum_rotate)),
          int(min_points), float(min_box_height), choices, seed, inputs['features'], inputs['one_hot_vectors'], targets['rotation_angle'],
          targets['rgb_score'], valid)
    return inputs, targets, valid


def detect_frame(model, scan, calib, boxes_2d, image_size, class_ids, scores, size_templates, *, num_heading_angle_bins=12,
                 **batch_options):
    """3-D boxes of one frame: `frame_batch`, the model under no_grad, `kitti.frustum_box_predictions`.
    -> (predictions (M, 8) fp64 numpy [h, w, l, cx, cy, cz, ry, score], valid (M,) bool numpy).  size_templates: (NS, 3) tensor.
    The only copy to the host is the result.  batch_options: `frame_batch`'s keywords."""
    from . import kitti
    inputs, targets, valid = frame_batch(scan, calib, boxes_2d, image_size, class_ids, scores=scores, **batch_options)
    dev = valid.device
    b = valid.shape[0]
    table = torch.zeros((b, 9), dtype=torch.float64, device=dev)
    with torch.no_grad():
        outputs = model(inputs)
        predictions = torch.zeros((b, 8), dtype=torch.float64, device=dev)
        kitti.frustum_box_predictions(predictions, outputs, targets, 0, size_templates,
                                      kitti.heading_angle_bin_centers(num_heading_angle_bins, dev))
        table[:, :8] = predictions
        table[:, 8] = valid.to(torch.float64)
    host = _read(table)
    return np.ascontiguousarray(host[:, :8]), host[:, 8] != 0


def kitti_label_lines(class_names, boxes_2d, predictions, valid=None):
    """The lines evaluate/kitti/frustum/eval.py:254-256 writes, one per valid box (host only): type, -1 -1 -10, the 2-D box, then
    h w l x y z ry score.  Written to NNNNNN.txt they are what `kitti.eval_from_files` reads."""
    predictions = np.asarray(predictions, dtype=np.float64).reshape(-1, 8)
    boxes_2d = np.asarray(boxes_2d, dtype=np.float64).reshape(-1, 4)
    valid = np.ones(len(predictions), dtype=bool) if valid is None else np.asarray(valid).astype(bool).reshape(-1)
    if not (len(class_names) == len(boxes_2d) == len(predictions) == len(valid)):
        raise ValueError('one class name, 2-D box, prediction and valid flag per box expected')
    return ['{} -1 -1 -10 {:f} {:f} {:f} {:f} {:f} {:f} {:f} {:f} {:f} {:f} {:f} {:f}\n'.format(class_names[i], *boxes_2d[i], *predictions[i])
            for i in range(len(predictions)) if valid[i]]
