"""KITTI box geometry on the device: the reference's get_box_iou_3d, the AP evaluation's overlaps and the --evaluate prediction table.

Reference: meters/kitti/utils.get_box_iou_3d clips on the host (Python + scipy); evaluate/kitti/utils/iou.py:rotate_iou_gpu_eval is
a numba.cuda kernel (it does not run on ROCm), and d3_box_overlap (evaluate/kitti/utils/eval.py:58-103) follows it with a host loop;
evaluate/kitti/frustum/eval.py:168-244 copies the decoded boxes to the host every batch and fills the table in a numba loop.  Here
all of them are launches of csrc/boxes.hip, one intersection routine for all (see include/pvcnn_hip.h, ABI v16).

`rotate_iou_gpu_eval` and `d3_box_overlap` keep the reference's signatures (numpy in, float32 numpy out), so they can be assigned over
`evaluate.kitti.utils.eval`'s module globals.

The AP evaluation itself (evaluate/kitti/utils/eval.py: image_box_overlap, clean_data, compute_statistics_jit, get_thresholds,
fused_compute_statistics -- `@numba.jit` loops over ~4 million greedy matchings for KITTI val) is here too: `get_official_eval_result`,
`do_eval`, `eval_class` and `image_box_overlap` keep the reference's signatures and results; `get_label_annotations` /
`eval_from_files` read KITTI label files, so neither numba nor the reference's evaluate.kitti.utils is needed.  The annotations are
packed once into flat device arrays with per-image prefix offsets; overlaps, clean_data, both matching passes, the thresholds and the
sums over the images are launches of csrc/kitti_ap.hip (one wave per matching) with no device-to-host copy between them; the host
reads pr, the thresholds and their counts at the end and forms the precision curves.
"""
import pathlib
import re

import numpy as np
import torch

from .modules.functional import backend as _be

__all__ = ['box_iou_3d', 'rotate_iou_gpu_eval', 'd3_box_overlap', 'heading_angle_bin_centers', 'frustum_box_predictions',
           'image_box_overlap', 'eval_class', 'do_eval', 'get_official_eval_result', 'get_label_annotation', 'get_label_annotations',
           'eval_from_files', 'MAX_BOXES_PER_IMAGE']


def box_iou_3d(corners_1, corners_t):
    """get_box_iou_3d on (B, 3, 8) device tensors -> (iou_3d, iou_2d), (B) float64 device tensors."""
    c1 = corners_1.float().contiguous()
    ct = corners_t.float().contiguous()
    return _be._backend.box_iou_3d(c1, ct)


def _device(device_id):
    return torch.device('cuda', int(device_id))


def rotate_iou_gpu_eval(boxes, query_boxes, criterion=-1, device_id=0):
    """(N, K) float32 numpy: criterion -1 IoU, 0 inter / area(query box), 1 inter / area(box), other the intersection, of rboxes
    (x, y, dx, dy, angle) -- the reference's rotate_iou_gpu_eval on the device."""
    boxes = np.ascontiguousarray(boxes, dtype=np.float32)
    query_boxes = np.ascontiguousarray(query_boxes, dtype=np.float32)
    n, k = boxes.shape[0], query_boxes.shape[0]
    if n == 0 or k == 0:
        return np.zeros((n, k), dtype=np.float32)
    dev = _device(device_id)
    out = _be._backend.rotate_iou(torch.from_numpy(boxes).to(dev), torch.from_numpy(query_boxes).to(dev), criterion)
    return out.cpu().numpy()


def d3_box_overlap(boxes, qboxes, criterion=-1, z_axis=1, z_center=1.0):
    """(N, K) float32 numpy: the reference's d3_box_overlap (BEV intersection, height overlap, criterion) in one launch.
    boxes (N, 7), qboxes (K, 7): x, y, z, l, h, w, ry (kitti camera format: z_axis=1)."""
    bev_axes = list(range(7))
    bev_axes.pop(z_axis + 3)
    bev_axes.pop(z_axis)
    boxes = np.asarray(boxes)
    qboxes = np.asarray(qboxes)
    n, k = boxes.shape[0], qboxes.shape[0]
    if n == 0 or k == 0:
        return np.zeros((n, k), dtype=np.float32)
    dev = torch.device('cuda', torch.cuda.current_device())

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)
    out = _be._backend.rotate_iou(up(boxes[:, bev_axes], np.float32), up(qboxes[:, bev_axes], np.float32), criterion,
                                  boxes_3d=up(boxes, np.float64), query_boxes_3d=up(qboxes, np.float64), z_axis=z_axis,
                                  z_center=z_center)
    return out.cpu().numpy()


def heading_angle_bin_centers(num_heading_angle_bins, device):
    """The reference's float32 torch.arange(0, 2 pi, 2 pi / NH) on `device`."""
    return torch.arange(0, 2 * np.pi, 2 * np.pi / num_heading_angle_bins).to(device)


def frustum_box_predictions(predictions, outputs, targets, current_step, size_templates, heading_angle_bin_centers):
    """The decode of evaluate/kitti/frustum/eval.py:180-185 and update_predictions, on the device: rows current_step ..
    current_step + B - 1 of `predictions` ((len(dataset), 8) float64 device tensor) become [h, w, l, cx, cy, cz, angle, rgb_score].
    outputs: the model's dict; targets: the loader's dict ('rotation_angle', 'rgb_score').  Returns current_step + B."""
    heads = tuple(outputs[k].float().contiguous() for k in
                  ('center', 'heading_scores', 'heading_residuals', 'size_scores', 'size_residuals'))
    dev = heads[0].device
    rotation_angle = targets['rotation_angle'].to(dev, torch.float64).contiguous()
    rgb_score = targets['rgb_score'].to(dev, torch.float64).contiguous()
    bin_centers = heading_angle_bin_centers.to(dev, torch.float32).contiguous()
    templates = size_templates.to(dev, torch.float32).contiguous()
    _be._backend.frustum_predictions(heads, bin_centers, templates, rotation_angle, rgb_score, predictions, current_step)
    return current_step + heads[0].shape[0]


# ---- the AP evaluation (evaluate/kitti/utils/eval.py, common.py) ---------------------------------------------------------------------
MAX_BOXES_PER_IMAGE = 2048               # PVCNN_KITTI_AP_MAX_BOXES: ground truths, and detections, of one image
NUM_SAMPLE_POINTS = 41
# clean_data's class table, lower-cased; class 5 is 'car' again and shares code 0 (include/pvcnn_hip.h)
_NAME_CODES = {'car': 0, 'pedestrian': 1, 'cyclist': 2, 'van': 3, 'person_sitting': 4, 'tractor': 6, 'trailer': 7}
_CLASS_TO_NAME = {0: 'Car', 1: 'Pedestrian', 2: 'Cyclist', 3: 'Van', 4: 'Person_sitting', 5: 'car', 6: 'tractor', 7: 'trailer'}


def image_box_overlap(boxes, query_boxes, criterion=-1):
    """(N, K) float64 numpy: the reference's image_box_overlap of (x1, y1, x2, y2) boxes on the device, bit-equal to its expression.
    criterion -1 IoU, 0 inter / area(box), 1 inter / area(query box), other the intersection."""
    boxes = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 4)
    query_boxes = np.ascontiguousarray(query_boxes, dtype=np.float64).reshape(-1, 4)
    n, k = boxes.shape[0], query_boxes.shape[0]
    if n == 0 or k == 0:
        return np.zeros((n, k), dtype=np.float64)
    dev = torch.device('cuda', torch.cuda.current_device())
    return _be._backend.image_box_overlap(torch.from_numpy(boxes).to(dev), torch.from_numpy(query_boxes).to(dev), criterion).cpu().numpy()


def _name_codes(names):
    names = np.asarray(names)
    if names.size == 0:
        return np.zeros((0,), dtype=np.int32)
    unique, inverse = np.unique(names, return_inverse=True)
    table = np.array([-2 if u == 'DontCare' else _NAME_CODES.get(str(u).lower(), -1) for u in unique], dtype=np.int32)
    return table[inverse.reshape(-1)]


class _Packed:
    """Ground-truth and detection annotations of I images as flat device arrays with per-image prefix offsets (gt_off, dt_off, dc_off,
    pair_off: int64, I + 1 words).  Built once per evaluation; the three metrics share it."""

    def __init__(self, gt_annos, dt_annos, device=None):
        assert len(gt_annos) == len(dt_annos)
        if len(gt_annos) == 0:
            raise ValueError('no images to evaluate')
        dev = device if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.device = dev
        self.images = len(gt_annos)

        def cat(annos, key, width=None):
            parts = [np.asarray(a[key], dtype=np.float64).reshape((-1,) if width is None else (-1, width)) for a in annos]
            return np.concatenate(parts, 0)

        def offsets(counts):
            return np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(counts, dtype=np.int64)])

        def up(a, dtype):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)
        gt_counts = np.array([len(a['name']) for a in gt_annos], dtype=np.int64)
        dt_counts = np.array([len(a['name']) for a in dt_annos], dtype=np.int64)
        self.G, self.D = int(gt_counts.sum()), int(dt_counts.sum())
        self.max_gt, self.max_dt = int(gt_counts.max()), int(dt_counts.max())
        gt_name = _name_codes(np.concatenate([np.asarray(a['name']).reshape(-1).astype(str) for a in gt_annos]))
        dt_name = _name_codes(np.concatenate([np.asarray(a['name']).reshape(-1).astype(str) for a in dt_annos]))
        gt_image = np.repeat(np.arange(self.images), gt_counts)
        dc_counts = np.bincount(gt_image[gt_name == -2], minlength=self.images)
        self.dontcares = int(dc_counts.sum())
        self.pairs = int((gt_counts * dt_counts).sum())
        self.gt_counts, self.dt_counts = gt_counts, dt_counts
        self.gt_off, self.dt_off = up(offsets(gt_counts), np.int64), up(offsets(dt_counts), np.int64)
        self.dc_off, self.pair_off = up(offsets(dc_counts), np.int64), up(offsets(gt_counts * dt_counts), np.int64)
        self.gt_name, self.dt_name = up(gt_name, np.int32), up(dt_name, np.int32)
        self.gt_bbox, self.dt_bbox = up(cat(gt_annos, 'bbox', 4), np.float64), up(cat(dt_annos, 'bbox', 4), np.float64)
        self.gt_alpha, self.dt_alpha = up(cat(gt_annos, 'alpha'), np.float64), up(cat(dt_annos, 'alpha'), np.float64)
        self.gt_occluded, self.gt_truncated = up(cat(gt_annos, 'occluded'), np.float64), up(cat(gt_annos, 'truncated'), np.float64)
        self.dt_score = up(cat(dt_annos, 'score'), np.float64)
        self._host_3d = [np.concatenate([cat(annos, 'location', 3), cat(annos, 'dimensions', 3), cat(annos, 'rotation_y')[:, None]], 1)
                         for annos in (dt_annos, gt_annos)]
        self._boxes_3d = {}

    def boxes_3d(self, z_axis):
        """(bev_dt, bev_gt float32 (., 5), full_dt, full_gt float64 (., 7)): (x, y, z, l, h, w, ry) and its BEV columns."""
        if z_axis not in self._boxes_3d:
            bev_axes = list(range(7))
            bev_axes.pop(z_axis + 3)
            bev_axes.pop(z_axis)
            dt, gt = self._host_3d
            dev = self.device
            self._boxes_3d[z_axis] = tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to(dev) for a, t in
                                           ((dt[:, bev_axes], np.float32), (gt[:, bev_axes], np.float32), (dt, np.float64), (gt, np.float64)))
        return self._boxes_3d[z_axis]


def _class_ints(current_classes):
    name_to_class = {v: n for n, v in _CLASS_TO_NAME.items()}
    if not isinstance(current_classes, (list, tuple, np.ndarray)):
        current_classes = [current_classes]
    return [name_to_class[c] if isinstance(c, str) else int(c) for c in current_classes]


def _curves(pr, counts, compute_aos):
    """precision / orientation (cells.., 41) from pr (cells.., 41, 4) and the number of thresholds per cell: tp / (tp + fp) and
    similarity / (tp + fp) in the used slots, then each slot the maximum of itself and everything behind it."""
    precision = np.zeros(pr.shape[:-1])
    aos = np.zeros(pr.shape[:-1])
    with np.errstate(invalid='ignore', divide='ignore'):
        for cell in np.ndindex(*counts.shape):
            n = int(counts[cell])
            found = pr[cell][:n, 0] + pr[cell][:n, 1]
            precision[cell][:n] = pr[cell][:n, 0] / found
            if compute_aos:
                aos[cell][:n] = pr[cell][:n, 3] / found
            for i in range(n):
                precision[cell][i] = np.max(precision[cell][i:])
                if compute_aos:
                    aos[cell][i] = np.max(aos[cell][i:])
    return precision, aos


def _eval_class_packed(packed, current_classes, difficulties, metric, min_overlaps, compute_aos, z_axis, z_center, overlaps=None, details=False):
    """eval_class on packed annotations.  overlaps: the flat per-image blocks to match on instead of the device's own; details: also
    return the intermediate results (host copies) under 'details'."""
    be = _be._backend
    dev = packed.device
    min_overlaps = np.asarray(min_overlaps)
    classes = _class_ints(list(current_classes))
    difficulties = [int(d) for d in difficulties]
    if any(c < 0 or c > 7 for c in classes) or any(d < 0 or d > 2 for d in difficulties):
        raise ValueError('classes must be in 0..7 and difficulties in 0..2')
    rows = np.ascontiguousarray(min_overlaps[:, metric, :len(classes)], dtype=np.float64)        # (K, M)
    if rows.shape[1] != len(classes) or not (rows >= 0).all():
        raise ValueError('min_overlaps must be (K, 3, num_classes) and >= 0')
    if overlaps is None:
        overlaps = be.kitti_ap_overlaps(packed, metric, z_axis=z_axis, z_center=z_center)
    overlaps = overlaps.to(torch.float64)
    clean = be.kitti_ap_clean(packed, torch.tensor(classes, dtype=torch.int32, device=dev),
                              torch.tensor(difficulties, dtype=torch.int32, device=dev))
    rows_dev = torch.from_numpy(rows).to(dev)
    tp_scores = be.kitti_ap_match(packed, overlaps, clean, rows_dev)
    thresholds, counts = be.kitti_ap_thresholds(tp_scores, clean[3])
    pr = be.kitti_ap_stats(packed, overlaps, clean, rows_dev, thresholds, counts, metric, compute_aos)
    pr, thresholds, counts = pr.cpu().numpy(), thresholds.cpu().numpy(), counts.cpu().numpy()
    precision, aos = _curves(pr, counts, compute_aos)
    ret = {'precision': precision, 'orientation': aos, 'thresholds': thresholds, 'min_overlaps': min_overlaps}
    if details:
        ret['details'] = {'overlaps': overlaps.cpu().numpy(), 'ignored_gt': clean[0].cpu().numpy(), 'ignored_det': clean[1].cpu().numpy(),
                          'dc_index': clean[2].cpu().numpy(), 'num_valid_gt': clean[3].cpu().numpy(), 'tp_scores': tp_scores.cpu().numpy(),
                          'counts': counts, 'pr': pr}
    return ret


def eval_class(gt_annos, dt_annos, current_classes, difficulties, metric, min_overlaps, compute_aos=False, z_axis=1, z_center=1.0,
               num_parts=50):
    """The reference's eval_class on the device: {'precision', 'orientation', 'thresholds' (num_class, num_difficulty, num_min_overlap,
    41), 'min_overlaps'}.  metric 0 bbox, 1 bev, 2 3d; min_overlaps (num_min_overlap, 3, num_class).  num_parts is accepted and
    ignored (only the per-image overlap blocks are formed); any number of images >= 1 works; at most MAX_BOXES_PER_IMAGE ground
    truths, and as many detections, per image (RuntimeError beyond)."""
    return _eval_class_packed(_Packed(gt_annos, dt_annos), current_classes, difficulties, metric, min_overlaps, compute_aos, z_axis,
                              z_center)


def do_eval(gt_annos, dt_annos, current_classes, min_overlaps, compute_aos=False, difficulties=(0, 1, 2), z_axis=1, z_center=1.0):
    """{'bbox', 'bev', '3d'} -> eval_class's dict; the annotations are packed once for the three metrics."""
    packed = _Packed(gt_annos, dt_annos)
    return {name: _eval_class_packed(packed, current_classes, difficulties, metric, min_overlaps, compute_aos, z_axis, z_center)
            for metric, name in enumerate(('bbox', 'bev', '3d'))}


def _mean_ap(precision):
    """The 11-point AP in percent over the last axis of 41 recall positions (every fourth)."""
    total = 0
    for i in range(0, precision.shape[-1], 4):
        total = total + precision[..., i]
    return total / 11 * 100


def get_official_eval_result(gt_annos, dt_annos, current_classes, difficulties=(0, 1, 2), z_axis=1, z_center=1.0):
    """(metrics, results, results_str) of the reference's get_official_eval_result: the bbox / bev / 3d (/ aos) AP table at the official
    KITTI overlaps.  AOS is computed when the first non-empty detection `alpha` is not -10."""
    per_class = [0.7, 0.5, 0.5, 0.7, 0.5, 0.7, 0.7, 0.7]
    min_overlaps = np.array([[per_class, per_class, per_class]])
    classes = _class_ints(current_classes)
    min_overlaps = min_overlaps[:, :, classes]
    compute_aos = False
    for anno in dt_annos:
        if np.asarray(anno['alpha']).shape[0] != 0:
            compute_aos = bool(anno['alpha'][0] != -10)
            break
    metrics = do_eval(gt_annos, dt_annos, classes, min_overlaps, compute_aos, difficulties, z_axis=z_axis, z_center=z_center)
    results, lines = {}, []
    for j, cls in enumerate(classes):
        name = _CLASS_TO_NAME[cls]
        ap = {key: _mean_ap(metrics[key]['precision'][j, :, 0]) for key in ('bbox', 'bev', '3d')}
        lines.append(name + ' AP(Average Precision)@{:.2f}, {:.2f}, {:.2f}:'.format(*min_overlaps[0, :, j]))
        for key, label in (('bbox', 'bbox'), ('bev', 'bev '), ('3d', '3d  ')):
            lines.append(f'{label} AP:' + ', '.join(f'{v:.2f}' for v in ap[key]))
        if compute_aos:
            lines.append('aos  AP:' + ', '.join(f'{v:.2f}' for v in _mean_ap(metrics['bbox']['orientation'][j, :, 0])))
        results[name] = ap
    return metrics, results, ''.join(line + '\n' for line in lines)


def get_label_annotation(label_path):
    """One KITTI label file -> the annotation dict the evaluation reads.  A line is: type truncated occluded alpha, bbox (left top right
    bottom), dimensions (height width length), location (x y z), rotation_y and, for detections, a score.  'dimensions' come out as
    (length, height, width), the camera-frame order of the box columns."""
    with open(label_path, 'r') as f:
        rows = [line.split() for line in f if line.strip()]

    def column(lo, hi, width):
        return np.array([[float(v) for v in r[lo:hi]] for r in rows], dtype=np.float64).reshape(-1, width)
    anno = {'name': np.array([r[0] for r in rows]),
            'truncated': column(1, 2, 1).reshape(-1),
            'occluded': np.array([int(r[2]) for r in rows], dtype=np.int64),
            'alpha': column(3, 4, 1).reshape(-1),
            'bbox': column(4, 8, 4),
            'dimensions': column(8, 11, 3)[:, [2, 0, 1]],
            'location': column(11, 14, 3),
            'rotation_y': column(14, 15, 1).reshape(-1)}
    anno['score'] = column(15, 16, 1).reshape(-1) if rows and len(rows[0]) == 16 else np.zeros(len(rows))
    return anno


def get_label_annotations(label_folder, image_ids=None):
    """The annotations of the label files NNNNNN.txt of a folder: all of them in order (image_ids None), the first n (an int) or the
    listed ids."""
    folder = pathlib.Path(label_folder)
    if image_ids is None:
        image_ids = sorted(int(p.stem) for p in folder.glob('*.txt') if re.match(r'^\d{6}.txt$', p.name))
    if not isinstance(image_ids, list):
        image_ids = list(range(image_ids))
    return [get_label_annotation(folder / f'{idx:06d}.txt') for idx in image_ids]


def eval_from_files(prediction_folder, ground_truth_folder, image_ids=None, verbose=False):
    """(metrics, results) of get_official_eval_result for classes Car, Pedestrian, Cyclist over two folders of KITTI label files;
    image_ids: a list of ids or a text file with one id per line (the ground truths to read; the predictions are read in full)."""
    predictions = get_label_annotations(prediction_folder)
    if isinstance(image_ids, str):
        with open(image_ids, 'r') as f:
            image_ids = [int(line) for line in f if line.strip()]
    ground_truths = get_label_annotations(ground_truth_folder, image_ids=image_ids)
    metrics, results, results_str = get_official_eval_result(ground_truths, predictions, current_classes=[0, 1, 2])
    if verbose:
        print(results_str)
    return metrics, results
