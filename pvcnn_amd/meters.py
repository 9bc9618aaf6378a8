"""Meters of train.py on the device: drop-ins for the reference's meters/s3dis.py, meters/shapenet.py and meters/kitti/frustum.py.

Reference: `MeterS3DIS.update` makes 3 x num_classes `.item()` calls per batch and `MeterShapeNet.update` loops over clouds and classes
with `.item()` -- host syncs that would dominate a replayed training step.  Here `update` only launches one kernel
(csrc/evaluate.hip: pvcnn_seg_meter_update) that accumulates integer counts on the device: it never syncs, so it can be captured
into a hipGraph.  `compute` makes ONE device-to-host copy and does the final arithmetic in Python floats in the reference's own order,
so its result is bit-equal to the reference meter's on the same tensors.

Constructors, `reset` / `update(outputs, targets)` / `compute()` and `part_class_to_shape_part_classes` are the reference's, so these
classes can stand in for `configs.train.meters[...]`.  MeterFrustumKitti.update is one launch (csrc/boxes.hip:
pvcnn_frustum_meter_update) where the reference decodes with torch, copies the corners to the host and clips them in Python.  Device buffers are allocated on the first `update` (on the outputs' device):
run one eager update before capturing a graph, and give `MeterShapeNet.reserve` the number of clouds a captured loop will add.
"""
import numpy as np
import torch

from .modules.functional import backend as _be

__all__ = ['MeterS3DIS', 'MeterShapeNet', 'MeterFrustumKitti', 'default_shape_name_to_part_classes']


default_shape_name_to_part_classes = {
    'Airplane': [0, 1, 2, 3],
    'Bag': [4, 5],
    'Cap': [6, 7],
    'Car': [8, 9, 10, 11],
    'Chair': [12, 13, 14, 15],
    'Earphone': [16, 17, 18],
    'Guitar': [19, 20, 21],
    'Knife': [22, 23],
    'Lamp': [24, 25, 26, 27],
    'Laptop': [28, 29],
    'Motorbike': [30, 31, 32, 33, 34, 35],
    'Mug': [36, 37],
    'Pistol': [38, 39, 40],
    'Rocket': [41, 42, 43],
    'Skateboard': [44, 45, 46],
    'Table': [47, 48, 49],
}


def _float_logits(outputs):
    return outputs if outputs.dtype == torch.float32 and outputs.is_contiguous() else outputs.float().contiguous()


def _long_targets(targets):
    return targets if targets.dtype == torch.int64 and targets.is_contiguous() else targets.long().contiguous()


def s3dis_meter_value(metric, num_classes, counts):
    """The reference's MeterS3DIS.compute on integer counts [seen C | positive C | correct C | numel | correct] (a list of ints)."""
    c = num_classes
    seen, positive, correct = counts[:c], counts[c:2 * c], counts[2 * c:3 * c]
    if metric == 'class':
        accuracy = 0
        for i in range(c):
            if seen[i] == 0:
                accuracy += 1
            else:
                accuracy += correct[i] / seen[i]
        return accuracy / c
    elif metric == 'iou':
        iou = 0
        for i in range(c):
            if seen[i] == 0:
                iou += 1
            else:
                iou += correct[i] / (seen[i] + positive[i] - correct[i])
        return iou / c
    else:
        return counts[3 * c + 1] / counts[3 * c]


def shapenet_meter_value(rows):
    """The reference's MeterShapeNet (update + compute) on per-cloud rows [(s, e), (intersection, union) per part class ...]."""
    iou_sum, shape_count = 0, 0
    for row in rows:
        start_class, end_class = row[0]
        if start_class >= end_class:
            raise IndexError('a cloud\'s first target is not a part class of the meter\'s table')
        iou = 0.0
        for intersection, union in row[1:1 + end_class - start_class]:
            if union == 0:
                iou += 1.0
            else:
                iou += intersection / union
        iou /= (end_class - start_class)
        iou_sum += iou
        shape_count += 1
    return iou_sum / shape_count


class MeterS3DIS:
    def __init__(self, metric='iou', num_classes=13):
        super().__init__()
        assert metric in ['overall', 'class', 'iou']
        self.metric = metric
        self.num_classes = num_classes
        self._counts = None                 # (3C + 2) int64 on the device of the first update
        self.reset()

    def reset(self):
        if self._counts is not None:
            self._counts.zero_()

    def update(self, outputs: torch.Tensor, targets: torch.Tensor):
        # outputs: B x num_classes x num_points, targets: B x num_points
        if self._counts is None or self._counts.device != outputs.device:
            self._counts = torch.zeros((3 * self.num_classes + 2,), dtype=torch.int64, device=outputs.device)
        _be._backend.seg_meter_update(_float_logits(outputs), _long_targets(targets), counts=self._counts)

    def counts(self):
        """[seen C | positive C | correct C | numel | correct] as Python ints (one device-to-host copy)."""
        if self._counts is None:
            return [0] * (3 * self.num_classes + 2)
        return self._counts.tolist()

    def compute(self):
        return s3dis_meter_value(self.metric, self.num_classes, self.counts())


class MeterShapeNet:
    def __init__(self, num_classes=50, num_shapes=16, shape_name_to_part_classes=None):
        super().__init__()
        self.num_classes = num_classes
        self.num_shapes = num_shapes

        self.shape_name_to_part_classes = default_shape_name_to_part_classes if shape_name_to_part_classes is None \
            else shape_name_to_part_classes
        part_class_to_shape_part_classes = []
        for shape_name, shape_part_classes in self.shape_name_to_part_classes.items():
            start_class, end_class = shape_part_classes[0], shape_part_classes[-1] + 1
            for _ in range(start_class, end_class):
                part_class_to_shape_part_classes.append((start_class, end_class))
        self.part_class_to_shape_part_classes = part_class_to_shape_part_classes
        self.max_parts = max(e - s for s, e in part_class_to_shape_part_classes)
        # device state: the part table, one row per cloud (kept until compute: the IoU is averaged per cloud, not pooled) and the
        # number of rows written, advanced on the device so that a replayed graph appends too
        self._ranges = self._rows = self._cursor = None
        self._host_count = 0                # rows added by eager updates (what the buffer must hold)
        self.reset()

    def reset(self):
        self._host_count = 0
        if self._cursor is not None:
            self._cursor.zero_()

    def _alloc(self, device, capacity):
        rows = torch.zeros((capacity, self.max_parts + 1, 2), dtype=torch.int32, device=device)
        if self._rows is not None and self._rows.device == device:
            rows[:self._rows.shape[0]] = self._rows
        else:
            self._ranges = torch.tensor(self.part_class_to_shape_part_classes, dtype=torch.int32, device=device).view(-1, 2)
            self._cursor = torch.zeros((1,), dtype=torch.int64, device=device)
            self._host_count = 0
        self._rows = rows

    def reserve(self, num_clouds, device):
        """Make room for num_clouds more clouds on `device` (call before capturing a graph of updates: a capture cannot grow it)."""
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        need = self._host_count + int(num_clouds)
        if self._rows is None or self._rows.device != device or need > self._rows.shape[0]:
            self._alloc(device, max(64, need, 2 * (self._rows.shape[0] if self._rows is not None else 0)))

    def update(self, outputs: torch.Tensor, targets: torch.Tensor):
        # outputs: B x num_classes x num_points, targets: B x num_points
        b = outputs.size(0)
        if not torch.cuda.is_current_stream_capturing():
            self.reserve(b, outputs.device)
        _be._backend.seg_meter_update(_float_logits(outputs), _long_targets(targets), part_ranges=self._ranges,
                                      max_parts=self.max_parts, rows=self._rows, row_cursor=self._cursor)
        self._cursor.add_(b)
        self._host_count += b

    def rows(self):
        """The per-cloud rows written so far as Python lists (one device-to-host copy)."""
        if self._rows is None:
            return []
        flat = torch.cat([self._cursor.to(torch.int32), self._rows.view(-1)]).tolist()
        n, width = flat[0], 2 * (self.max_parts + 1)
        if n > self._rows.shape[0]:
            raise RuntimeError(f'MeterShapeNet: {n} clouds updated but room for {self._rows.shape[0]}: reserve() more before capturing')
        return [[tuple(flat[1 + r * width + 2 * i: 3 + r * width + 2 * i]) for i in range(self.max_parts + 1)] for r in range(n)]

    def compute(self):
        return shapenet_meter_value(self.rows())


FRUSTUM_METRICS = ['iou_2d', 'iou_3d', 'accuracy', 'iou_3d_accuracy', 'iou_3d_class_accuracy']


def frustum_class_thresholds(class_name_to_class_id):
    """The per-class IoU threshold of the reference's update: 0.7 for 'Car', 0.5 for every other class (in the table's order)."""
    return [0.7 if cls == 'Car' else 0.5 for cls in class_name_to_class_id.keys()]


def frustum_meter_value(metric, class_names, sums, counts):
    """The reference's MeterFrustumKitti.compute on sums [iou_2d, iou_3d] (floats) and counts [seen, correct, iou_3d correct,
    correct per class K ..., seen per class K ...] (ints), classes in `class_names` order."""
    k = len(class_names)
    seen, correct, iou_3d_correct = counts[0], counts[1], counts[2]
    if metric == 'iou_3d':
        return sums[1] / seen
    elif metric == 'iou_2d':
        return sums[0] / seen
    elif metric == 'accuracy':
        return correct / seen
    elif metric == 'iou_3d_accuracy':
        return iou_3d_correct / seen
    elif metric == 'iou_3d_class_accuracy':
        return sum(counts[3 + i] / max(counts[3 + k + i], 1) for i in range(k)) / k
    else:
        raise KeyError


class MeterFrustumKitti:
    def __init__(self, num_heading_angle_bins, num_size_templates, size_templates, class_name_to_class_id,
                 metric='iou_3d'):
        super().__init__()
        assert metric in FRUSTUM_METRICS
        self.metric = metric
        self.num_heading_angle_bins = num_heading_angle_bins
        self.num_size_templates = num_size_templates
        self.size_templates = size_templates.view(self.num_size_templates, 3)
        # the reference's float32 arange (its values can differ from i * 2pi / NH by an ulp): uploaded, never recomputed
        self.heading_angle_bin_centers = torch.arange(0, 2 * np.pi, 2 * np.pi / self.num_heading_angle_bins)
        self.class_name_to_class_id = class_name_to_class_id
        self.class_thresholds = frustum_class_thresholds(class_name_to_class_id)
        # device state, allocated by the first eager update: sums (2) float64, counts (3 + 2K) int64 and the constant tables
        self._sums = self._counts = self._tables = None
        self.reset()

    def reset(self):
        if self._counts is not None:
            self._sums.zero_()
            self._counts.zero_()

    def _alloc(self, device):
        k = len(self.class_name_to_class_id)
        self._sums = torch.zeros((2,), dtype=torch.float64, device=device)
        self._counts = torch.zeros((3 + 2 * k,), dtype=torch.int64, device=device)
        self._tables = (self.heading_angle_bin_centers.to(device=device, dtype=torch.float32).contiguous(),
                        self.size_templates.to(device=device, dtype=torch.float32).contiguous(),
                        torch.tensor(list(self.class_name_to_class_id.values()), dtype=torch.int64, device=device),
                        torch.tensor(self.class_thresholds, dtype=torch.float64, device=device))

    def update(self, outputs, targets):
        ref = outputs['mask_logits'] if self.metric == 'accuracy' else outputs['center']
        if self._counts is None or self._counts.device != ref.device:
            self._alloc(ref.device)
        if self.metric == 'accuracy':
            _be._backend.frustum_meter_accuracy(_float_logits(outputs['mask_logits']), _long_targets(targets['mask_logits']),
                                                self._counts)
            return
        heads = tuple(_float_logits(outputs[k]) for k in
                      ('center', 'heading_scores', 'heading_residuals', 'size_scores', 'size_residuals'))
        tgt = (_float_logits(targets['center']), _long_targets(targets['heading_bin_id']),
               _float_logits(targets['heading_residual']), _long_targets(targets['size_template_id']),
               _float_logits(targets['size_residual']), _long_targets(targets['class_id']))
        bin_centers, templates, class_ids, thresholds = self._tables
        _be._backend.frustum_meter_update(heads, tgt, bin_centers, templates, class_ids, thresholds, self._sums, self._counts)

    def state(self):
        """(sums [iou_2d, iou_3d] as floats, counts as ints): one device-to-host copy."""
        k = len(self.class_name_to_class_id)
        if self._counts is None:
            return [0.0, 0.0], [0] * (3 + 2 * k)
        packed = torch.cat([self._sums.view(torch.int64), self._counts]).cpu()
        return packed[:2].view(torch.float64).tolist(), packed[2:].tolist()

    def compute(self):
        sums, counts = self.state()
        return frustum_meter_value(self.metric, list(self.class_name_to_class_id.keys()), sums, counts)
