"""CPU: the sequential truth of the KITTI AP evaluation (tests/kitti_ap_truth.py) equals the reference's recorded run
(tests/golden/kitti_ap.pt, produced by tests/golden/gen_kitti_ap_golden.py from evaluate/kitti/utils/eval.py itself), and the new entry
points of the C ABI are declared, bound, exported and refuse bad arguments before any launch.  No GPU is needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import kitti_ap_truth as truth
from conftest import ROOT

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'kitti_ap.pt')
ENTRY_POINTS = ['pvcnn_image_box_overlap', 'pvcnn_kitti_ap_bbox_overlaps', 'pvcnn_kitti_ap_box_overlaps', 'pvcnn_kitti_ap_clean',
                'pvcnn_kitti_ap_match', 'pvcnn_kitti_ap_thresholds', 'pvcnn_kitti_ap_workspace_bytes', 'pvcnn_kitti_ap_stats']
METRICS = ('bbox', 'bev', '3d')


@pytest.fixture(scope='module')
def golden():
    return torch.load(GOLDEN, weights_only=False)


@pytest.fixture(scope='module')
def images(golden):
    return truth.images_from_golden(golden['gt'], golden['dt'], golden['names'])


@pytest.fixture(scope='module')
def evaluated(golden, images):
    """The truth's run over the golden's annotations and the golden's overlaps, once for the three metrics (AOS on)."""
    mo = golden['min_overlaps'].numpy()
    return {key: truth.evaluate(images, truth.split_overlaps(golden['overlaps'][key].numpy(), images), golden['classes'],
                                golden['difficulties'], metric, mo, compute_aos=True) for metric, key in enumerate(METRICS)}


def test_fixture_meets_its_conditions(golden):
    assert len(golden['gt']['counts']) >= 50
    counts = torch.stack([golden['metrics'][k]['counts'] for k in METRICS])
    assert (counts == 41).any() and ((counts > 0) & (counts < 41)).any()
    assert (golden['clean']['num_valid_gt'] == 0).any()
    assert golden['stuff'] > 0 and golden['ignored_assignments'] > 0
    scores = golden['dt']['score']
    assert len(torch.unique(scores)) < 10 < len(scores)                       # discrete scores: ties occur
    for key in ('bev', '3d'):
        ov = golden['overlaps'][key]
        assert ov.dtype == torch.float32
        assert not any(((ov.double() - t).abs() < 1e-4).any() for t in (0.5, 0.7))
    assert os.path.getsize(GOLDEN) < 300 * 1024


def test_clean_equals_the_reference(golden, evaluated):
    got = evaluated['bbox']
    for m in range(3):
        for l in range(3):
            assert got['ignored_gt'][m][l] == golden['clean']['ignored_gt'][m, l].tolist()
            assert got['ignored_det'][m][l] == golden['clean']['ignored_det'][m, l].tolist()
    assert np.array_equal(got['num_valid_gt'], golden['clean']['num_valid_gt'].numpy())


@pytest.mark.parametrize('key', METRICS)
def test_matching_thresholds_and_pr_equal_the_reference(golden, evaluated, key):
    want, got = golden['metrics'][key], evaluated[key]
    # pass 1: the true-positive scores of every (cell, image), in order
    flat = [s for m in range(3) for l in range(3) for per_image in got['tp_scores'][m][l][0] for s in per_image]
    lens = [len(per_image) for m in range(3) for l in range(3) for per_image in got['tp_scores'][m][l][0]]
    assert lens == want['tp_counts'].reshape(-1).tolist()
    assert np.array_equal(np.array(flat), want['tp_scores'].numpy())
    assert np.array_equal(got['counts'], want['counts'].numpy())
    assert np.array_equal(got['thresholds'], want['eval']['thresholds'].numpy())
    assert np.array_equal(got['pr'][..., :3], want['pr'][..., :3].numpy())
    np.testing.assert_allclose(got['pr'][..., 3], want['pr'][..., 3].numpy(), rtol=1e-12, atol=0)
    assert np.array_equal(got['precision'], want['eval']['precision'].numpy(), equal_nan=True)
    np.testing.assert_allclose(got['orientation'], want['eval']['orientation'].numpy(), rtol=1e-12, atol=0)


def test_mean_ap_equals_the_reference(golden, evaluated):
    for j, name in enumerate(('Car', 'Pedestrian', 'Cyclist')):
        for key in METRICS:
            assert np.array_equal(truth.mean_ap(evaluated[key]['precision'][j, :, 0]), golden['results'][name][key].numpy(), equal_nan=True)


def test_thresholds_skip_branch():
    """Many more true positives than 41: the scan skips scores; few: it takes every one."""
    scores = np.linspace(0.99, 0.01, 500)
    got = truth.thresholds(scores, 500)
    assert len(got) == 41 and got[0] == scores[0] and got[-1] == scores[-1]
    assert truth.thresholds(scores[:5], 5) == scores[:5].tolist()
    assert truth.thresholds([], 0) == []


# ---- the C ABI of the feature ---------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    from pvcnn_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'pvcnn_hip.h')).read()
    assert re.search(r'#define\s+PVCNN_ABI_VERSION\s+17\b', text) and _lib.ABI_VERSION == 17
    assert re.search(r'#define\s+PVCNN_KITTI_AP_MAX_BOXES\s+2048\b', text)
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = _lib.load()
    assert lib.pvcnn_version() == 17
    for name in ENTRY_POINTS:
        assert re.search(r'PVCNN_API\s+[\w\s\*]+?\b' + name + r'\s*\(', code), f'{name} not declared'
        assert name in _lib.SIGNATURES, f'{name} not bound'
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f'{name} not exported'


def _refused(lib, rc, text):
    assert rc != 0
    message = lib.pvcnn_last_error_string().decode()
    assert text in message, message


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Null pointers and over-limit images: a nonzero return and an error text; nothing is dereferenced or launched (no GPU here)."""
    from pvcnn_amd import _lib
    from pvcnn_amd.kitti import MAX_BOXES_PER_IMAGE
    lib = _lib.load()
    vp = ctypes.c_void_p
    p = vp(0x100000)                                    # any non-null address: the checks come before the launch
    null = vp(None)
    _refused(lib, lib.pvcnn_image_box_overlap(null, 4, p, 4, -1, p, null), 'null pointer')
    _refused(lib, lib.pvcnn_image_box_overlap(p, -1, p, 4, -1, p, null), 'bad sizes')
    _refused(lib, lib.pvcnn_kitti_ap_bbox_overlaps(p, p, p, null, p, 2, 10, p, null), 'null pointer')
    _refused(lib, lib.pvcnn_kitti_ap_box_overlaps(p, null, p, null, p, p, p, 2, 10, -1, 1, 1.0, null, null), 'null pointer')
    _refused(lib, lib.pvcnn_kitti_ap_box_overlaps(p, p, p, null, p, p, p, 2, 10, -1, 1, 1.0, p, null), 'go together')
    _refused(lib, lib.pvcnn_kitti_ap_box_overlaps(p, p, p, p, p, p, p, 2, 10, -1, 3, 1.0, p, null), 'z_axis')
    _refused(lib, lib.pvcnn_kitti_ap_clean(p, p, p, p, 5, p, p, 5, p, p, 2, null, 3, p, 3, p, p, p, p, null), 'null pointer')
    _refused(lib, lib.pvcnn_kitti_ap_clean(p, p, p, p, 5, p, p, 5, p, p, 2, p, 0, p, 3, p, p, p, p, null), 'classes * difficulties')
    _refused(lib, lib.pvcnn_kitti_ap_thresholds(p, 5, null, 9, 1, p, p, null), 'null pointer')
    _refused(lib, lib.pvcnn_kitti_ap_thresholds(p, 5, p, 9, 2, p, p, null), 'bad sizes')

    def matching(max_gt=5, max_dt=5, overlaps=p, min_overlaps=p):
        return [overlaps, p, p, p, p, 2, 5, 5, max_gt, max_dt] + [p] * 8 + [min_overlaps, 3, 3, 1]
    for args in (matching(max_gt=MAX_BOXES_PER_IMAGE + 1), matching(max_dt=MAX_BOXES_PER_IMAGE + 1)):
        _refused(lib, lib.pvcnn_kitti_ap_match(*args, p, null), 'more than 2048')
        _refused(lib, lib.pvcnn_kitti_ap_stats(*args, p, p, 0, 0, p, p, 1 << 20, null), 'more than 2048')
    _refused(lib, lib.pvcnn_kitti_ap_match(*matching(overlaps=null), p, null), 'null pointer')
    _refused(lib, lib.pvcnn_kitti_ap_match(*matching(), null, null), 'null pointer')
    _refused(lib, lib.pvcnn_kitti_ap_stats(*matching(min_overlaps=null), p, p, 0, 0, p, p, 1 << 20, null), 'null pointer')
    _refused(lib, lib.pvcnn_kitti_ap_stats(*matching(), p, p, 3, 0, p, p, 1 << 20, null), 'metric')
    _refused(lib, lib.pvcnn_kitti_ap_stats(*matching(), p, p, 0, 0, p, p, 8, null), 'workspace too small')
    assert lib.pvcnn_kitti_ap_workspace_bytes(2, 9) == 9 * 41 * 1 * 4 * 8
    assert lib.pvcnn_kitti_ap_workspace_bytes(3769, 9) == 9 * 41 * 472 * 4 * 8
    assert lib.pvcnn_kitti_ap_workspace_bytes(0, 9) == 0


def test_label_files_round_trip(tmp_path, golden, images):
    """get_label_annotations reads KITTI label lines: the fields, 'dimensions' reordered to (l, h, w), scores only for detections."""
    from pvcnn_amd import kitti
    gt, dt = truth.annotations(images[:3])
    for folder, annos, scored in (('gt', gt, False), ('dt', dt, True)):
        (tmp_path / folder).mkdir()
        for idx, a in enumerate(annos):
            lines = []
            for i in range(len(a['name'])):
                l, h, w = a['dimensions'][i]
                fields = [a['name'][i], repr(float(a['truncated'][i])), str(int(a['occluded'][i])), repr(float(a['alpha'][i]))]
                fields += [repr(float(v)) for v in a['bbox'][i]] + [repr(float(v)) for v in (h, w, l)]
                fields += [repr(float(v)) for v in a['location'][i]] + [repr(float(a['rotation_y'][i]))]
                if scored:
                    fields.append(repr(float(a['score'][i])))
                lines.append(' '.join(fields))
            (tmp_path / folder / f'{idx:06d}.txt').write_text('\n'.join(lines) + ('\n' if lines else ''))
        (tmp_path / folder / 'notes.txt').write_text('not a label file\n')
        back = kitti.get_label_annotations(tmp_path / folder)
        assert len(back) == 3
        for a, b in zip(annos, back):
            assert list(a['name']) == list(b['name'])
            for key in ('truncated', 'occluded', 'alpha', 'bbox', 'dimensions', 'location', 'rotation_y', 'score'):
                assert np.array_equal(np.asarray(a[key], dtype=np.float64).reshape(np.asarray(b[key]).shape), b[key]), key
    assert len(kitti.get_label_annotations(tmp_path / 'gt', image_ids=2)) == 2
    assert len(kitti.get_label_annotations(tmp_path / 'gt', image_ids=[2, 0])) == 2
