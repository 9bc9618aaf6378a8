#!/usr/bin/env python3
"""Generate tests/golden/kitti_ap.pt from the REFERENCE ITSELF (evaluate/kitti/utils/eval.py), run where the reference tree is mounted.

The reference's eval.py is loaded as gen_kitti_golden.py loads it: numba replaced by a stand-in whose jit returns the function
unchanged.  Its rotate_iou_gpu_eval (a numba.cuda launch) is replaced by a loop over the reference's own dev_rotate_iou_eval per pair,
in rotate_iou_kernel_eval's argument order.  Nothing of pvcnn_amd takes part in producing the expected values.

Input: IMAGES seeded synthetic images (>= 50: the reference raises below that).  Names from Car / Pedestrian / Cyclist / Van /
Person_sitting / Truck / DontCare, occlusion 0..3, truncation on both sides of 0.15 / 0.3 / 0.5, 2-D heights on both sides of 25 / 40;
detections are noisy copies of ground truths plus false positives, some of them inside DontCare regions; scores come from a small
discrete set, so ties occur.  Two variants: detections with an alpha (AOS on) and with alpha == -10 (AOS off).

Recorded for classes [0, 1, 2] from ONE run of the reference's eval_class per metric, through wrappers around its own functions: the
packed annotations, image_box_overlap at its four criteria, the per-image overlaps of the three metrics, clean_data's flags, the pass-1 true-positive scores per image,
get_thresholds' output, pr, the eval_class dicts, and get_official_eval_result's results / results_str.

Conditions on the fixture (an offending image is REDRAWN, nothing is dropped; the global ones are asserted):
  * no bev / 3d overlap within 1e-4 of 0.5 or 0.7;
  * no two non-identical detections overlap the same ground truth above 0.5 - 1e-4 with bev / 3d overlaps closer than 1e-4;
  * a cell with all 41 thresholds, a cell with fewer, a cell with num_valid_gt == 0;
  * the DontCare subtraction (nstuff > 0) and the assignment of a ground truth to an ignored_det == 1 detection each occur;
  * every recorded bev / 3d overlap is within REFERENCE_ERROR = 3e-6 of the same overlap evaluated in fp64 (tests/eval_truth.py on the
    fp32 box parameters).  The reference intersects edges in fp32 through cross products of ABSOLUTE coordinates, so its own error
    grows with the square of the distance from the origin and with 1 / sin of the angle between crossing edges: for a Pedestrian 28 m
    away whose detection is turned by 0.004 rad it returned 0.95700 where the geometry gives 0.95667 (3.3e-4), and 4e-5 at 16 m with
    0.1 rad.  A bound of PAIR_TOL = 1e-5 on |kernel - reference| presupposes a reference that is itself well inside it, hence this
    condition; it leaves 7e-6 for the fp32 corner rounding of the kernel under test (corners below 8 m: half an ulp is 2.4e-7, a
    Pedestrian's 0.5 m^2 moves by 0.7 m x that per corner, about 3e-7 of IoU each).  To keep such redraws rare the scene lies within
    4 m x 8 m of the camera and a detection is turned against its ground truth by at least MIN_TURN = 0.1 rad.
Run:  python tests/golden/gen_kitti_ap_golden.py [reference root]     (rewrites kitti_ap.pt)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import eval_truth                                      # noqa: E402  (tests/eval_truth.py: the fp64 geometry of an rbox pair)
SEED = 1588147245
IMAGES = 110
CLASSES = [0, 1, 2]
DIFFICULTIES = (0, 1, 2)
MARGIN = 1e-4
REFERENCE_ERROR = 3e-6                                # see the docstring: the reference's own fp32 rounding, per pair
BEV_AXES = [0, 2, 3, 5, 6]
MIN_TURN = 0.1                                        # radians between a detection and its ground truth, see the docstring
NAMES = ['Car', 'Pedestrian', 'Cyclist', 'Van', 'Person_sitting', 'Truck', 'DontCare']
NAME_P = [0.28, 0.24, 0.14, 0.08, 0.07, 0.07, 0.12]
SIZES = {'Car': (3.9, 1.5, 1.6), 'Van': (5.0, 2.2, 1.9), 'Truck': (10.0, 3.2, 2.6), 'Pedestrian': (0.8, 1.7, 0.6),
         'Person_sitting': (0.8, 1.3, 0.6), 'Cyclist': (1.8, 1.7, 0.6)}                                  # l, h, w
SCORES = [0.1, 0.3, 0.5, 0.5, 0.7, 0.9, 0.95]
KEYS = ('name', 'truncated', 'occluded', 'alpha', 'bbox', 'dimensions', 'location', 'rotation_y', 'score')


def load_reference():
    spec = importlib.util.spec_from_file_location('gen_kitti_golden', os.path.join(HERE, 'gen_kitti_golden.py'))
    base = importlib.util.module_from_spec(spec)
    argv, sys.argv = sys.argv, sys.argv[:2]
    try:
        spec.loader.exec_module(base)
        ref = base.load_reference()
    finally:
        sys.argv = argv
    ev = sys.modules['ref_kitti_utils.eval']
    cache = {}

    def rotate_iou(boxes, query_boxes, criterion=-1, device_id=0):
        boxes, query_boxes = boxes.astype(np.float32), query_boxes.astype(np.float32)
        out = np.zeros((boxes.shape[0], query_boxes.shape[0]), dtype=np.float32)
        for n in range(boxes.shape[0]):
            for k in range(query_boxes.shape[0]):
                key = (boxes[n].tobytes(), query_boxes[k].tobytes(), criterion)
                if key not in cache:
                    cache[key] = ref.dev_rotate_iou_eval(query_boxes[k], boxes[n], criterion)
                out[n, k] = cache[key]
        return out
    ev.rotate_iou_gpu_eval = rotate_iou
    return ev


def empty(n):
    return {'name': np.empty(n, dtype='<U16'), 'truncated': np.zeros(n), 'occluded': np.zeros(n, dtype=np.int64), 'alpha': np.zeros(n),
            'bbox': np.zeros((n, 4)), 'dimensions': np.zeros((n, 3)), 'location': np.zeros((n, 3)), 'rotation_y': np.zeros(n),
            'score': np.zeros(n)}


def draw_image(rng):
    n = rng.randint(0, 9)
    gt = empty(n)
    for i in range(n):
        name = rng.choice(NAMES, p=NAME_P)
        height = rng.choice([18.0, 24.0, 30.0, 38.0, 45.0, 80.0, 120.0]) + rng.rand()
        width = height * rng.uniform(0.5, 2.0)
        x0, y0 = rng.uniform(0, 1100), rng.uniform(100, 250)
        gt['name'][i] = name
        gt['bbox'][i] = [x0, y0, x0 + width, y0 + height]
        if name == 'DontCare':
            gt['truncated'][i], gt['occluded'][i], gt['alpha'][i], gt['rotation_y'][i] = -1, -1, -10, -10
            gt['dimensions'][i], gt['location'][i] = -1, -1000
            continue
        gt['truncated'][i] = rng.choice([0.0, 0.1, 0.2, 0.4, 0.6], p=[0.5, 0.2, 0.15, 0.1, 0.05])
        gt['occluded'][i] = rng.choice([0, 1, 2, 3], p=[0.55, 0.2, 0.15, 0.1])
        if name == 'Cyclist' and gt['occluded'][i] == 0:
            gt['occluded'][i] = 1                       # no Cyclist is 'easy': that cell has num_valid_gt == 0
        if name == 'Pedestrian':
            gt['truncated'][i], gt['occluded'][i] = rng.choice([0.0, 0.1]), 0     # every Pedestrian is detected: full recall, 41 thresholds
            gt['bbox'][i, 3] = y0 + 45.0 + rng.rand() * 60
        gt['alpha'][i] = rng.uniform(-np.pi, np.pi)
        gt['dimensions'][i] = np.array(SIZES[name]) * rng.uniform(0.9, 1.1, 3)
        gt['location'][i] = [rng.uniform(-4, 4), rng.uniform(1, 2), rng.uniform(2, 8)]
        gt['rotation_y'][i] = rng.uniform(-np.pi, np.pi)
    rows = []
    for i in range(n):
        name = str(gt['name'][i])
        copies = 1 if name == 'Pedestrian' else rng.choice([0, 1, 1, 1, 2])
        for _ in range(copies):
            noise = 0.01 if name == 'Pedestrian' else rng.choice([0.02, 0.08, 0.25])
            height = gt['bbox'][i, 3] - gt['bbox'][i, 1]
            bbox = gt['bbox'][i] + rng.randn(4) * noise * height * 0.5
            if 45.0 <= height < 46.0 and name != 'Pedestrian' and rng.rand() < 0.5:
                # a detection below 40 pixels on a ground truth above: ignored_det == 1 at difficulty 0, and it is assigned
                bbox = gt['bbox'][i] + np.array([0.0, 0.5, 0.0, -0.5]) * (height - 39.5)
            if name == 'DontCare':                      # a detection inside a DontCare region: "stuff" for the 2-D metric
                label = rng.choice(['Car', 'Pedestrian'])
                dims, loc, ry = np.array(SIZES[label]), np.array([rng.uniform(-4, 4), 1.5, rng.uniform(2, 8)]), rng.uniform(-3, 3)
                bbox = gt['bbox'][i] + np.array([1.0, 1.0, -1.0, -1.0]) * rng.uniform(0.5, 2.0)
            else:
                label = name if rng.rand() > 0.1 or name == 'Pedestrian' else rng.choice(['Car', 'Pedestrian', 'Cyclist'])
                dims = gt['dimensions'][i] * (1 + rng.randn(3) * noise)
                loc = gt['location'][i] + rng.randn(3) * noise * np.array([2.0, 0.3, 2.0])
                ry = gt['rotation_y'][i] + rng.choice([-1.0, 1.0]) * rng.uniform(MIN_TURN, MIN_TURN + 4 * noise)
            rows.append((label, gt['alpha'][i] + rng.randn() * 0.3, bbox, dims, loc, ry, rng.choice(SCORES)))
    for _ in range(rng.randint(0, 3)):                  # false positives
        label = rng.choice(['Car', 'Pedestrian', 'Cyclist'])
        x0, y0, height = rng.uniform(0, 1100), rng.uniform(100, 250), rng.uniform(15, 100)
        rows.append((label, rng.uniform(-3, 3), np.array([x0, y0, x0 + height, y0 + height]), np.array(SIZES[label]),
                     np.array([rng.uniform(-4, 4), 1.5, rng.uniform(2, 8)]), rng.uniform(-3, 3), rng.choice(SCORES[:5])))
    dt = empty(len(rows))
    for j, (label, alpha, bbox, dims, loc, ry, score) in enumerate(rows):
        dt['name'][j], dt['alpha'][j], dt['bbox'][j], dt['dimensions'][j] = label, alpha, bbox, dims
        dt['location'][j], dt['rotation_y'][j], dt['score'][j] = loc, ry, score
    return gt, dt


def boxes_7(anno):
    return np.concatenate([anno['location'], anno['dimensions'], anno['rotation_y'][:, None]], 1)


def image_is_generic(ev, gt, dt):
    if len(gt['name']) == 0 or len(dt['name']) == 0:
        return True
    g, d = boxes_7(gt), boxes_7(dt)
    bev = ev.bev_box_overlap(d[:, BEV_AXES], g[:, BEV_AXES]).astype(np.float64)
    d3 = ev.d3_box_overlap(d, g).astype(np.float64)
    geometry = eval_truth.pair_geometry_f64(d[:, BEV_AXES].astype(np.float32), g[:, BEV_AXES].astype(np.float32))
    exact = (eval_truth.rotate_iou_truth(geometry, -1), eval_truth.d3_overlap_truth(geometry, d, g, -1))
    for ov, ov_f64 in zip((bev, d3), exact):
        if not np.isfinite(ov).all() or any(np.any(np.abs(ov - t) < MARGIN) for t in (0.5, 0.7)):
            return False
        if np.abs(ov - ov_f64).max() > REFERENCE_ERROR:
            return False
        for col in range(ov.shape[1]):
            strong = np.nonzero(ov[:, col] > 0.5 - MARGIN)[0]
            for a in strong:
                for b in strong:
                    if a < b and abs(ov[a, col] - ov[b, col]) < MARGIN and not all(np.array_equal(dt[k][a], dt[k][b]) for k in KEYS):
                        return False
    return True


class Recorder:
    """Wraps the reference's compute_statistics_jit, get_thresholds and fused_compute_statistics while its eval_class runs."""

    def __init__(self, ev):
        self.ev = ev
        self.orig = {n: getattr(ev, n) for n in ('compute_statistics_jit', 'get_thresholds', 'fused_compute_statistics')}
        self.tp_scores, self.thresholds, self.pr, self.stuff, self.ignored_assignments = [], [], [], 0, 0

    def __enter__(self):
        ev, orig = self.ev, self.orig

        def compute_statistics_jit(overlaps, gt_datas, dt_datas, ignored_gt, ignored_det, dc_bboxes, metric, min_overlap, thresh=0,
                                   compute_fp=False, compute_aos=False):
            ret = orig['compute_statistics_jit'](overlaps, gt_datas, dt_datas, ignored_gt, ignored_det, dc_bboxes, metric, min_overlap,
                                                 thresh, compute_fp, compute_aos)
            if not compute_fp:
                self.tp_scores.append(np.array(ret[4], dtype=np.float64))
            else:
                self.ignored_assignments += int((np.asarray(ignored_gt) == 0).sum()) - ret[0] - ret[2]
                if metric == 0 and len(dc_bboxes):
                    bare = orig['compute_statistics_jit'](overlaps, gt_datas, dt_datas, ignored_gt, ignored_det, dc_bboxes[:0], metric,
                                                          min_overlap, thresh, compute_fp, compute_aos)
                    self.stuff += bare[1] - ret[1]
            return ret

        def get_thresholds(scores, num_gt, num_sample_pts=41):
            ret = orig['get_thresholds'](scores, num_gt, num_sample_pts)
            self.thresholds.append(np.array(ret, dtype=np.float64))
            return ret

        def fused_compute_statistics(overlaps, pr, *args, **kwargs):
            if not any(pr is seen for seen in self.pr):
                self.pr.append(pr)
            return orig['fused_compute_statistics'](overlaps, pr, *args, **kwargs)
        ev.compute_statistics_jit, ev.get_thresholds, ev.fused_compute_statistics = (compute_statistics_jit, get_thresholds,
                                                                                    fused_compute_statistics)
        return self

    def __exit__(self, *exc):
        for n, f in self.orig.items():
            setattr(self.ev, n, f)


def record_metric(ev, gt_annos, dt_annos, metric, min_overlaps, compute_aos):
    cells = len(CLASSES) * len(DIFFICULTIES) * min_overlaps.shape[0]
    images = len(gt_annos)
    with Recorder(ev) as rec, np.errstate(invalid='ignore', divide='ignore'):
        ret = ev.eval_class(gt_annos, dt_annos, CLASSES, DIFFICULTIES, metric, min_overlaps, compute_aos)
    assert len(rec.tp_scores) == cells * images and len(rec.thresholds) == cells and len(rec.pr) == cells
    pr = np.zeros((cells, 41, 4))
    counts = np.zeros(cells, dtype=np.int64)
    for c in range(cells):
        counts[c] = len(rec.thresholds[c])
        pr[c, :counts[c]] = rec.pr[c]
    shape = (len(CLASSES), len(DIFFICULTIES), min_overlaps.shape[0])
    # the true-positive scores of a cell, image after image (cell-major, as eval_class loops), with the per-image counts
    tp_counts = np.array([len(s) for s in rec.tp_scores], dtype=np.int64).reshape(shape + (images,))
    tp_scores = np.concatenate(rec.tp_scores) if rec.tp_scores else np.zeros(0)
    return {'tp_scores': torch.from_numpy(tp_scores), 'tp_counts': torch.from_numpy(tp_counts.astype(np.int16)),
            'counts': torch.from_numpy(counts.reshape(shape)), 'pr': torch.from_numpy(pr.reshape(shape + (41, 4))),
            'eval': {k: torch.from_numpy(np.asarray(v)) for k, v in ret.items()}}, rec


def main():
    ev = load_reference()
    rng = np.random.RandomState(SEED)
    gt_annos, dt_annos, redrawn = [], [], 0
    while len(gt_annos) < IMAGES:
        gt, dt = draw_image(rng)
        if not image_is_generic(ev, gt, dt):
            redrawn += 1
            continue
        gt_annos.append(gt)
        dt_annos.append(dt)
    dt_plain = [dict(d, alpha=np.full_like(d['alpha'], -10.0)) for d in dt_annos]

    names = sorted({str(n) for a in gt_annos + dt_annos for n in a['name']})

    def pack(annos):
        out = {'counts': torch.tensor([len(a['name']) for a in annos], dtype=torch.int16),
               'name': torch.tensor([names.index(str(n)) for a in annos for n in a['name']], dtype=torch.int8)}
        for k in KEYS[1:]:
            out[k] = torch.from_numpy(np.concatenate([a[k] for a in annos], 0))
        out['occluded'] = out['occluded'].to(torch.int8)
        return out

    overlaps = {}
    for metric, key in enumerate(('bbox', 'bev', '3d')):
        per_image = ev.calculate_iou_partly(dt_annos, gt_annos, metric, 50)[0]          # eval_class's call: overlaps[det, gt]
        flat = np.concatenate([o.reshape(-1) for o in per_image])
        if metric > 0:
            assert np.array_equal(flat, flat.astype(np.float32).astype(np.float64))
            flat = flat.astype(np.float32)
        overlaps[key] = torch.from_numpy(flat)

    # image_box_overlap itself, every criterion, on the first detections against the first ground truths
    some_dt = np.concatenate([a['bbox'] for a in dt_annos], 0)[:24]
    some_gt = np.concatenate([a['bbox'] for a in gt_annos], 0)[:20]
    box_overlap = {'boxes': torch.from_numpy(some_dt), 'query_boxes': torch.from_numpy(some_gt),
                   'out': {c: torch.from_numpy(ev.image_box_overlap(some_dt, some_gt, c)) for c in (-1, 0, 1, 2)}}
    assert all((o > 0).sum() >= 10 for o in box_overlap['out'].values())

    clean = {'ignored_gt': [], 'ignored_det': [], 'num_valid_gt': []}
    for cls in CLASSES:
        for diff in DIFFICULTIES:
            flags = [ev.clean_data(g, d, cls, diff) for g, d in zip(gt_annos, dt_annos)]
            clean['num_valid_gt'].append(sum(f[0] for f in flags))
            clean['ignored_gt'].append(np.concatenate([np.array(f[1], dtype=np.int8) for f in flags]))
            clean['ignored_det'].append(np.concatenate([np.array(f[2], dtype=np.int8) for f in flags]))
    shape = (len(CLASSES), len(DIFFICULTIES))
    clean = {'ignored_gt': torch.from_numpy(np.stack(clean['ignored_gt']).reshape(shape + (-1,))),
             'ignored_det': torch.from_numpy(np.stack(clean['ignored_det']).reshape(shape + (-1,))),
             'num_valid_gt': torch.tensor(clean['num_valid_gt'], dtype=torch.int64).reshape(shape)}

    official = np.array([[[0.7, 0.5, 0.5]] * 3])                                        # get_official_eval_result's, classes 0, 1, 2
    metrics, stuff, ignored_assignments = {}, 0, 0
    for metric, key in enumerate(('bbox', 'bev', '3d')):
        metrics[key], rec = record_metric(ev, gt_annos, dt_annos, metric, official, True)
        stuff += rec.stuff
        ignored_assignments += rec.ignored_assignments
    counts = torch.stack([metrics[k]['counts'] for k in metrics])
    assert (counts == 41).any() and ((counts < 41) & (counts > 0)).any(), counts
    assert (clean['num_valid_gt'] == 0).any() and stuff > 0 and ignored_assignments > 0, (clean['num_valid_gt'], stuff, ignored_assignments)

    with np.errstate(invalid='ignore', divide='ignore'):
        ref_metrics, results, results_str = ev.get_official_eval_result(gt_annos, dt_annos, CLASSES)
        plain_metrics, plain_results, plain_str = ev.get_official_eval_result(gt_annos, dt_plain, CLASSES)
    for key in metrics:
        for field in ('precision', 'orientation', 'thresholds'):
            assert np.array_equal(ref_metrics[key][field], metrics[key]['eval'][field].numpy(), equal_nan=True)
        # without alpha the same curves, and no orientation
        assert np.array_equal(plain_metrics[key]['precision'], ref_metrics[key]['precision'], equal_nan=True)
        assert np.array_equal(plain_metrics[key]['thresholds'], ref_metrics[key]['thresholds'])
        assert not plain_metrics[key]['orientation'].any()
    assert 'aos' in results_str and 'aos' not in plain_str

    def plain(results):
        return {c: {k: torch.from_numpy(np.asarray(v)) for k, v in r.items()} for c, r in results.items()}
    golden = {'seed': SEED, 'classes': CLASSES, 'difficulties': list(DIFFICULTIES), 'names': names, 'min_overlaps': torch.from_numpy(official),
              'gt': pack(gt_annos), 'dt': pack(dt_annos), 'overlaps': overlaps, 'image_box_overlap': box_overlap, 'clean': clean, 'metrics': metrics,
              'results': plain(results), 'results_str': results_str,
              # the alpha == -10 variant: the same detections, every alpha -10; its curves equal the ones above (asserted here)
              'plain_results': plain(plain_results), 'plain_results_str': plain_str,
              'stuff': int(stuff), 'ignored_assignments': int(ignored_assignments)}
    path = os.path.join(HERE, 'kitti_ap.pt')
    torch.save(golden, path)
    size = os.path.getsize(path)
    assert size < 300 * 1024, size
    print(f'wrote {path} ({size} bytes); redrawn {redrawn}; thresholds per cell {counts.reshape(3, -1).tolist()}; '
          f'num_valid_gt {clean["num_valid_gt"].tolist()}; stuff {stuff}; ignored-detection assignments {ignored_assignments}')
    print(results_str)


if __name__ == '__main__':
    main()
