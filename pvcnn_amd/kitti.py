"""KITTI box geometry on the device: the reference's get_box_iou_3d, the AP evaluation's overlaps and the --evaluate prediction table.

Reference: meters/kitti/utils.get_box_iou_3d clips on the host (Python + scipy); evaluate/kitti/utils/iou.py:rotate_iou_gpu_eval is
a numba.cuda kernel (it does not run on ROCm), and d3_box_overlap (evaluate/kitti/utils/eval.py:58-103) follows it with a host loop;
evaluate/kitti/frustum/eval.py:168-244 copies the decoded boxes to the host every batch and fills the table in a numba loop.  Here
all of them are launches of csrc/boxes.hip, one intersection routine for all (see include/pvcnn_hip.h, ABI v14).

`rotate_iou_gpu_eval` and `d3_box_overlap` keep the reference's signatures (numpy in, float32 numpy out), so they can be assigned over
`evaluate.kitti.utils.eval`'s module globals.
"""
import numpy as np
import torch

from .modules.functional import backend as _be

__all__ = ['box_iou_3d', 'rotate_iou_gpu_eval', 'd3_box_overlap', 'heading_angle_bin_centers', 'frustum_box_predictions']


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
