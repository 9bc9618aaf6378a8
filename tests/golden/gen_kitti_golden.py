#!/usr/bin/env python3
"""Generate tests/golden/kitti_boxes.pt from the REFERENCE ITSELF (Frustum-KITTI meter and box overlaps), run where the reference tree
is mounted.

Producers of the expected values:
  * meters/kitti/frustum.py   MeterFrustumKitti, all five metrics, over seeded batches of Car / Pedestrian / Cyclist boxes
  * meters/kitti/utils.py     get_box_iou_3d (on the corners of modules/frustum.get_box_corners_3d)
  * evaluate/kitti/utils/iou.py   dev_rotate_iou_eval per pair, as rotate_iou_kernel_eval calls it (criteria -1, 0, 1, 2)
  * evaluate/kitti/utils/eval.py  d3_box_overlap_kernel on the criterion-2 BEV matrix, as d3_box_overlap calls it (criteria -1, 0, 1, 2)
imported from the reference tree on the CPU.  numba is replaced by a stand-in whose jit / njit / cuda.jit return the function
unchanged and whose cuda.local.array is np.zeros; modules.functional is replaced by an empty module (get_box_corners_3d does not use
it, and importing it would build the reference's CUDA extension).  Generic cases only: no recorded IoU lies within 1e-4 of a
threshold (0.5, 0.7), and every box has a positive size.  Nothing of pvcnn_amd takes part in producing the expected values.
Run:  python tests/golden/gen_kitti_golden.py [reference root]     (rewrites kitti_boxes.pt)
"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
SEED = 1588147245
THRESHOLDS = (0.5, 0.7)
CLASSES = ('Car', 'Pedestrian', 'Cyclist')
NUM_HEADING_BINS = 12


def _stand_in_numba():
    fake = types.ModuleType('numba')

    def jit(*args, **kwargs):
        if len(args) == 1 and callable(args[0]) and not kwargs:
            return args[0]
        return lambda f: f
    fake.jit = fake.njit = jit
    fake.float32, fake.float64, fake.int32, fake.int64 = np.float32, np.float64, np.int32, np.int64
    cuda = types.ModuleType('numba.cuda')
    cuda.jit = jit
    cuda.local = types.SimpleNamespace(array=lambda shape, dtype: np.zeros(shape, dtype=dtype))
    cuda.shared = cuda.local
    fake.cuda = cuda
    return fake, cuda


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def load_reference():
    numba, cuda = _stand_in_numba()
    sys.modules['numba'], sys.modules['numba.cuda'] = numba, cuda
    pkg = types.ModuleType('modules')
    pkg.__path__ = [os.path.join(REF, 'modules')]
    sys.modules['modules'] = pkg
    sys.modules['modules.functional'] = types.ModuleType('modules.functional')
    frustum = _load('modules.frustum', os.path.join(REF, 'modules', 'frustum.py'))
    sys.path.insert(0, REF)
    try:
        meter = importlib.import_module('meters.kitti.frustum').MeterFrustumKitti
        box_utils = importlib.import_module('meters.kitti.utils')
        attributes = _load('ref_kitti_attributes', os.path.join(REF, 'datasets', 'kitti', 'attributes.py')).kitti_attributes
    finally:
        sys.path.remove(REF)
    iou = _load('ref_kitti_iou', os.path.join(REF, 'evaluate', 'kitti', 'utils', 'iou.py'))
    # eval.py imports `.iou` relatively: give it a parent package
    evpkg = types.ModuleType('ref_kitti_utils')
    evpkg.__path__ = [os.path.join(REF, 'evaluate', 'kitti', 'utils')]
    sys.modules['ref_kitti_utils'] = evpkg
    sys.modules['ref_kitti_utils.iou'] = iou
    ev = _load('ref_kitti_utils.eval', os.path.join(REF, 'evaluate', 'kitti', 'utils', 'eval.py'))
    return types.SimpleNamespace(meter=meter, get_box_corners_3d=frustum.get_box_corners_3d, get_box_iou_3d=box_utils.get_box_iou_3d,
                                 attributes=attributes, dev_rotate_iou_eval=iou.dev_rotate_iou_eval,
                                 d3_box_overlap_kernel=ev.d3_box_overlap_kernel)


def near_threshold(values):
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    return any(np.any(np.abs(v - t) < 1e-4) for t in THRESHOLDS)


def meter_batch(ref, rng, batch_size, num_points, size_templates, template_of_class):
    """Network outputs near the target boxes: the predicted bins / templates are mostly right, centers a few decimetres off."""
    ns, nh = size_templates.shape[0], NUM_HEADING_BINS
    class_id = rng.randint(0, len(CLASSES), size=batch_size)
    sid_t = np.array([template_of_class[c] for c in class_id])
    hid_t = rng.randint(0, nh, size=batch_size)
    bin_width = 2 * np.pi / nh
    center_t = np.stack([rng.uniform(-3, 3, batch_size), rng.uniform(-1, 2, batch_size), rng.uniform(5, 30, batch_size)], 1)
    heading_residual_t = rng.uniform(-bin_width / 2, bin_width / 2, batch_size)
    size_residual_t = rng.uniform(-0.15, 0.15, (batch_size, 3)) * size_templates[sid_t]
    heading_scores = rng.randn(batch_size, nh)
    right = rng.rand(batch_size) < 0.75
    heading_scores[np.arange(batch_size)[right], hid_t[right]] += 6.0
    heading_residuals = rng.uniform(-bin_width / 2, bin_width / 2, (batch_size, nh))
    heading_residuals[np.arange(batch_size), hid_t] = heading_residual_t + rng.randn(batch_size) * 0.1
    size_scores = rng.randn(batch_size, ns)
    right = rng.rand(batch_size) < 0.8
    size_scores[np.arange(batch_size)[right], sid_t[right]] += 6.0
    size_residuals = rng.uniform(-0.2, 0.2, (batch_size, ns, 3)) * size_templates[None]
    size_residuals[np.arange(batch_size), sid_t] = size_residual_t + rng.randn(batch_size, 3) * 0.05 * size_templates[sid_t]
    center = center_t + rng.randn(batch_size, 3) * np.array([0.4, 0.2, 0.6]) * rng.choice([0.3, 1.0, 3.0], size=(batch_size, 1))
    mask_logits = rng.randn(batch_size, 2, num_points)
    mask_target = rng.randint(0, 2, size=(batch_size, num_points))
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))            # noqa: E731
    i = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64))              # noqa: E731
    outputs = {'center': f(center), 'heading_scores': f(heading_scores), 'heading_residuals': f(heading_residuals),
               'size_scores': f(size_scores), 'size_residuals': f(size_residuals), 'mask_logits': f(mask_logits)}
    targets = {'center': f(center_t), 'heading_bin_id': i(hid_t), 'heading_residual': f(heading_residual_t),
               'size_template_id': i(sid_t), 'size_residual': f(size_residual_t), 'class_id': i(class_id),
               'mask_logits': i(mask_target)}
    return outputs, targets


def batch_corners(ref, outputs, targets, size_templates_t):
    """The corners the reference meter builds (meters/kitti/frustum.py:55-66), for the per-pair get_box_iou_3d record."""
    b = outputs['center'].shape[0]
    bid = torch.arange(b)
    centers = torch.arange(0, 2 * np.pi, 2 * np.pi / NUM_HEADING_BINS)
    hid = torch.argmax(outputs['heading_scores'], 1)
    heading = centers[hid] + outputs['heading_residuals'][bid, hid]
    sid = torch.argmax(outputs['size_scores'], 1)
    size = size_templates_t[sid] + outputs['size_residuals'][bid, sid]
    c1 = ref.get_box_corners_3d(centers=outputs['center'], headings=heading, sizes=size, with_flip=False)
    heading_t = centers[targets['heading_bin_id']] + targets['heading_residual']
    size_t = size_templates_t[targets['size_template_id']] + targets['size_residual']
    ct = ref.get_box_corners_3d(centers=targets['center'], headings=heading_t, sizes=size_t, with_flip=False)
    return c1, ct


def camera_boxes(rng, n):
    """KITTI camera-frame boxes (x, y, z, l, h, w, ry), clustered so that many pairs overlap."""
    anchors = np.stack([rng.uniform(-8, 8, 4), rng.uniform(1.0, 2.0, 4), rng.uniform(8, 25, 4)], 1)
    pos = anchors[rng.randint(0, 4, n)] + rng.randn(n, 3) * np.array([1.5, 0.3, 1.5])
    dims = np.stack([rng.uniform(1.0, 4.5, n), rng.uniform(1.3, 1.9, n), rng.uniform(0.6, 2.0, n)], 1)
    ry = rng.uniform(-np.pi, np.pi, n)
    return np.concatenate([pos, dims, ry[:, None]], 1)


def overlap_case(ref, rng, n, k):
    while True:
        boxes, qboxes = camera_boxes(rng, n), camera_boxes(rng, k)
        # half of the query boxes are near copies of boxes (the detections of a ground truth): IoUs up to ~0.9
        near = rng.choice(n, k // 2, replace=False)
        qboxes[:k // 2] = boxes[near] + rng.randn(k // 2, 7) * np.array([0.4, 0.1, 0.4, 0.2, 0.05, 0.1, 0.15])
        bev = boxes[:, [0, 2, 3, 5, 6]].astype(np.float32)                 # d3_box_overlap's BEV columns (z_axis = 1), as float32
        qbev = qboxes[:, [0, 2, 3, 5, 6]].astype(np.float32)
        rotate = {}
        for crit in (-1, 0, 1, 2):
            m = np.zeros((n, k), dtype=np.float32)
            for a in range(n):
                for b in range(k):
                    m[a, b] = ref.dev_rotate_iou_eval(qbev[b], bev[a], crit)     # rotate_iou_kernel_eval's argument order
            rotate[crit] = m
        d3 = {}
        for crit in (-1, 0, 1, 2):
            rinc = rotate[2].copy()
            ref.d3_box_overlap_kernel(boxes, qboxes, rinc, crit, 1, 1.0)
            d3[crit] = rinc
        if near_threshold(np.concatenate([m.ravel() for m in (*rotate.values(), *d3.values())])):
            continue
        if not all(np.isfinite(m).all() for m in (*rotate.values(), *d3.values())):
            continue
        return {'boxes': torch.from_numpy(boxes), 'query_boxes': torch.from_numpy(qboxes),
                'rotate': {c: torch.from_numpy(m) for c, m in rotate.items()},
                'd3': {c: torch.from_numpy(m) for c, m in d3.items()}}


def main():
    ref = load_reference()
    rng = np.random.RandomState(SEED)
    names = ref.attributes.class_names
    size_templates = np.stack([ref.attributes.class_name_to_size_template[c] for c in names]).astype(np.float32)
    size_templates_t = torch.from_numpy(size_templates)
    template_of_class = [names.index(c) for c in CLASSES]
    class_name_to_class_id = {c: i for i, c in enumerate(CLASSES)}

    metrics = ['iou_2d', 'iou_3d', 'accuracy', 'iou_3d_accuracy', 'iou_3d_class_accuracy']
    meters = {m: ref.meter(NUM_HEADING_BINS, len(names), size_templates_t, class_name_to_class_id, metric=m) for m in metrics}
    batches, pairs = [], []
    for batch_size in (32, 32, 29, 32):
        while True:
            outputs, targets = meter_batch(ref, rng, batch_size, 32, size_templates, template_of_class)
            c1, ct = batch_corners(ref, outputs, targets, size_templates_t)
            iou_3d, iou_2d = ref.get_box_iou_3d(c1.numpy(), ct.numpy())
            if not near_threshold(np.concatenate([iou_3d, iou_2d])) and np.isfinite(iou_3d).all() and np.isfinite(iou_2d).all():
                break
        for m in meters.values():
            m.update(outputs, targets)
        batches.append({'outputs': outputs, 'targets': targets})
        pairs.append({'corners_1': c1, 'corners_t': ct, 'iou_3d': torch.from_numpy(iou_3d), 'iou_2d': torch.from_numpy(iou_2d)})
    values = {m: float(meters[m].compute()) for m in metrics}
    box_iou = {k: torch.cat([p[k] for p in pairs]) for k in pairs[0]}
    golden = {
        'seed': SEED, 'num_heading_angle_bins': NUM_HEADING_BINS, 'size_templates': size_templates_t,
        'class_name_to_class_id': class_name_to_class_id,
        'meter': {'batches': batches, 'values': values,
                  'counts': {'iou_3d_corrent_num': int(meters['iou_3d'].iou_3d_corrent_num),
                             'total_seen_num': int(meters['iou_3d'].total_seen_num),
                             'total_correct_num': int(meters['accuracy'].total_correct_num),
                             'total_seen_points': int(meters['accuracy'].total_seen_num),
                             'correct_per_class': {c: int(v) for c, v in meters['iou_3d'].iou_3d_corrent_num_per_class.items()},
                             'seen_per_class': {c: int(v) for c, v in meters['iou_3d'].total_seen_num_per_class.items()}}},
        'box_iou_3d': box_iou,
        'overlaps': overlap_case(ref, rng, 24, 20),
    }
    path = os.path.join(HERE, 'kitti_boxes.pt')
    torch.save(golden, path)
    print(f'wrote {path} ({os.path.getsize(path)} bytes): {values}')


if __name__ == '__main__':
    main()
