"""Host side of the Frustum-KITTI meter (pvcnn_amd.meters.MeterFrustumKitti): the final arithmetic of compute() against the
reference's formulas (meters/kitti/frustum.py:76-89, restated here), the metric check, the per-class IoU thresholds and the layout of
tests/golden/kitti_boxes.pt.  No GPU needed."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'kitti_boxes.pt')
CLASSES = {'Car': 0, 'Pedestrian': 1, 'Cyclist': 2}


def _reference_compute(metric, class_names, state):
    """MeterFrustumKitti.compute as the reference writes it, on the reference's own attributes."""
    if metric == 'iou_3d':
        return state['iou_3d_sum'] / state['total_seen_num']
    elif metric == 'iou_2d':
        return state['iou_2d_sum'] / state['total_seen_num']
    elif metric == 'accuracy':
        return state['total_correct_num'] / state['total_seen_num']
    elif metric == 'iou_3d_accuracy':
        return state['iou_3d_corrent_num'] / state['total_seen_num']
    return sum(state['iou_3d_corrent_num_per_class'][cls] / max(state['total_seen_num_per_class'][cls], 1)
               for cls in class_names) / len(class_names)


@pytest.mark.parametrize('metric', ['iou_2d', 'iou_3d', 'accuracy', 'iou_3d_accuracy', 'iou_3d_class_accuracy'])
@pytest.mark.parametrize('per_class', [([5, 2, 0], [9, 7, 0]), ([0, 0, 0], [0, 0, 0]), ([3, 1, 4], [3, 5, 9])])
def test_compute_arithmetic_matches_the_reference(metric, per_class):
    from pvcnn_amd.meters import frustum_meter_value
    correct, seen = per_class
    sums = [17.123456789, 14.987654321]
    counts = [21, 13, 8] + correct + seen                         # [boxes, correct points, iou_3d >= 0.7, correct K, seen K]
    state = {'iou_2d_sum': sums[0], 'iou_3d_sum': sums[1], 'total_seen_num': counts[0], 'total_correct_num': counts[1],
             'iou_3d_corrent_num': counts[2], 'iou_3d_corrent_num_per_class': dict(zip(CLASSES, correct)),
             'total_seen_num_per_class': dict(zip(CLASSES, seen))}
    assert frustum_meter_value(metric, list(CLASSES), sums, counts) == _reference_compute(metric, list(CLASSES), state)


def test_metric_is_checked():
    from pvcnn_amd.meters import MeterFrustumKitti
    with pytest.raises(AssertionError):
        MeterFrustumKitti(12, 8, torch.zeros(8, 3), CLASSES, metric='iou_bev')
    for metric in ['iou_2d', 'iou_3d', 'accuracy', 'iou_3d_accuracy', 'iou_3d_class_accuracy']:
        MeterFrustumKitti(12, 8, torch.zeros(8, 3), CLASSES, metric=metric)       # no device touched before the first update


def test_car_threshold_mapping():
    from pvcnn_amd.meters import MeterFrustumKitti, frustum_class_thresholds
    assert frustum_class_thresholds(CLASSES) == [0.7, 0.5, 0.5]
    assert frustum_class_thresholds({'Pedestrian': 4, 'Van': 1, 'Car': 0}) == [0.5, 0.5, 0.7]
    assert frustum_class_thresholds({'car': 0, 'Cyclist': 1}) == [0.5, 0.5]             # the reference compares the name exactly
    m = MeterFrustumKitti(12, 8, torch.zeros(8, 3), CLASSES)
    assert m.class_thresholds == [0.7, 0.5, 0.5]
    # the heading bin centers are the reference's float32 arange, not i * 2pi / NH
    assert m.heading_angle_bin_centers.dtype == torch.float32
    assert torch.equal(m.heading_angle_bin_centers, torch.arange(0, 2 * np.pi, 2 * np.pi / 12))


def test_golden_file_structure():
    g = torch.load(GOLDEN, weights_only=False)
    assert g['class_name_to_class_id'] == CLASSES
    nh, templates = g['num_heading_angle_bins'], g['size_templates']
    assert nh == 12 and templates.dtype == torch.float32 and tuple(templates.shape) == (8, 3)
    meter = g['meter']
    assert set(meter['values']) == {'iou_2d', 'iou_3d', 'accuracy', 'iou_3d_accuracy', 'iou_3d_class_accuracy'}
    total = 0
    for batch in meter['batches']:
        o, t = batch['outputs'], batch['targets']
        b = o['center'].shape[0]
        total += b
        assert tuple(o['heading_scores'].shape) == (b, nh) and tuple(o['size_residuals'].shape) == (b, 8, 3)
        assert o['mask_logits'].dim() == 3 and tuple(t['mask_logits'].shape) == (b, o['mask_logits'].shape[2])
        for k in ('heading_bin_id', 'size_template_id', 'class_id', 'mask_logits'):
            assert t[k].dtype == torch.int64
        assert set(t['class_id'].tolist()) <= set(CLASSES.values())
    c = meter['counts']
    assert c['total_seen_num'] == total and sum(c['seen_per_class'].values()) == total
    assert all(v > 0 for v in c['seen_per_class'].values())          # every class is covered
    # the count metrics follow from the recorded counts with the reference's formulas
    from pvcnn_amd.meters import frustum_meter_value
    counts = [c['total_seen_num'], 0, c['iou_3d_corrent_num']] + list(c['correct_per_class'].values()) + list(c['seen_per_class'].values())
    assert frustum_meter_value('iou_3d_accuracy', list(CLASSES), [0.0, 0.0], counts) == meter['values']['iou_3d_accuracy']
    assert frustum_meter_value('iou_3d_class_accuracy', list(CLASSES), [0.0, 0.0], counts) == meter['values']['iou_3d_class_accuracy']
    assert c['total_correct_num'] / c['total_seen_points'] == meter['values']['accuracy']
    pairs = g['box_iou_3d']
    assert tuple(pairs['corners_1'].shape) == (total, 3, 8) and pairs['iou_3d'].dtype == torch.float64
    o = g['overlaps']
    n, k = o['boxes'].shape[0], o['query_boxes'].shape[0]
    assert o['boxes'].shape[1] == 7 and o['query_boxes'].shape[1] == 7
    for kind in ('rotate', 'd3'):
        assert set(o[kind]) == {-1, 0, 1, 2}
        for m in o[kind].values():
            assert m.dtype == torch.float32 and tuple(m.shape) == (n, k) and torch.isfinite(m).all()
    # generic cases only: nothing recorded sits on an AP / meter threshold
    vals = torch.cat([pairs['iou_3d'], pairs['iou_2d']] + [m.double().view(-1) for kind in ('rotate', 'd3') for m in o[kind].values()])
    for thr in (0.5, 0.7):
        assert ((vals - thr).abs() >= 1e-4).all()
