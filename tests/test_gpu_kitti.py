"""Frustum-KITTI metrics on the device (csrc/boxes.hip, pvcnn_amd.meters.MeterFrustumKitti, pvcnn_amd.kitti) against
tests/golden/kitti_boxes.pt -- the reference's own meter, get_box_iou_3d, dev_rotate_iou_eval and d3_box_overlap_kernel -- and, for
degenerate geometry the reference cannot handle, against an fp64 truth written in this file.  Reads nothing outside the repository."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'kitti_boxes.pt')
PAIR_TOL = 1e-5          # absolute, per pair (the reference clips in fp32; the device clips the fp32 corners in fp64)
METRICS = ['iou_2d', 'iou_3d', 'accuracy', 'iou_3d_accuracy', 'iou_3d_class_accuracy']


@pytest.fixture(scope='module')
def golden():
    return torch.load(GOLDEN, weights_only=False)


def _to(d):
    return {k: v.to(DEV) for k, v in d.items()}


def _meter(golden, metric):
    from pvcnn_amd.meters import MeterFrustumKitti
    return MeterFrustumKitti(golden['num_heading_angle_bins'], golden['size_templates'].shape[0], golden['size_templates'],
                             golden['class_name_to_class_id'], metric=metric)


@pytest.mark.parametrize('metric', METRICS)
def test_meter_matches_reference(golden, metric):
    m = _meter(golden, metric)
    for batch in golden['meter']['batches']:
        m.update(_to(batch['outputs']), _to(batch['targets']))
    got, want = m.compute(), golden['meter']['values'][metric]
    if metric in ('iou_2d', 'iou_3d'):
        assert abs(got - want) <= PAIR_TOL, (got, want)
    else:
        assert got == want, (got, want)          # counts: exactly the reference's
    if metric == 'iou_3d_class_accuracy':
        c = golden['meter']['counts']
        _, counts = m.state()
        k = len(golden['class_name_to_class_id'])
        assert counts[0] == c['total_seen_num'] and counts[2] == c['iou_3d_corrent_num']
        assert counts[3:3 + k] == list(c['correct_per_class'].values()) and counts[3 + k:] == list(c['seen_per_class'].values())


def _clip_area_fp64(p, q):
    """Area of the intersection of two counter-clockwise convex polygons (Sutherland-Hodgman in fp64)."""
    out = p
    for i in range(len(q)):
        a, b = q[i], q[(i + 1) % len(q)]
        inp, out = out, []
        f = lambda v: (b[0] - a[0]) * (v[1] - a[1]) - (b[1] - a[1]) * (v[0] - a[0])      # noqa: E731
        for j in range(len(inp)):
            s_, e = inp[j - 1], inp[j]
            fs, fe = f(s_), f(e)
            if (fs < 0) != (fe < 0):
                t = fs / (fs - fe)
                out.append((s_[0] + t * (e[0] - s_[0]), s_[1] + t * (e[1] - s_[1])))
            if fe >= 0:
                out.append(e)
    return _area_fp64(out) if len(out) >= 3 else 0.0


def _area_fp64(poly):
    return 0.5 * sum(poly[i - 1][0] * poly[i][1] - poly[i][0] * poly[i - 1][1] for i in range(len(poly)))


def _box_iou_fp64(c1, ct):
    """get_box_iou_3d in fp64 on the fp32 corners (relative to the first corner), the truth both sides are measured against."""
    c1, ct = c1.astype(np.float64), ct.astype(np.float64)
    ox, oz = c1[0, 0], c1[2, 0]

    def quad(c):
        poly = [(c[0, i] - ox, c[2, i] - oz) for i in (3, 2, 1, 0)]
        return poly if _area_fp64(poly) >= 0 else poly[::-1]
    p, q = quad(c1), quad(ct)
    inter, a1, a2 = _clip_area_fp64(p, q), _area_fp64(p), _area_fp64(q)
    h = max(0.0, min(c1[1, 0], ct[1, 0]) - max(c1[1, 4], ct[1, 4]))
    v1, v2 = a1 * abs(c1[1, 0] - c1[1, 4]), a2 * abs(ct[1, 0] - ct[1, 4])
    return inter * h / (v1 + v2 - inter * h), inter / (a1 + a2 - inter)


def test_box_iou_3d_matches_reference(golden):
    """Measured: the device differs from the reference by up to 2.5e-5 (BEV) / 1.1e-5 (3-D), and the reference differs from an fp64
    truth by exactly as much: the reference clips in fp32 at absolute coordinates (products of ~26 m coordinates round at ~6e-5
    absolute; a 0.7 m^2 pedestrian box turns that into 2.5e-5 of IoU), the device clips the same fp32 corners in fp64 relative to a
    corner.  So the device is checked against the fp64 truth at 1e-9, and against the reference within the reference's own error."""
    from pvcnn_amd.kitti import box_iou_3d
    g = golden['box_iou_3d']
    iou_3d, iou_2d = (t.cpu().numpy() for t in box_iou_3d(g['corners_1'].to(DEV), g['corners_t'].to(DEV)))
    truth = np.array([_box_iou_fp64(a, b) for a, b in zip(g['corners_1'].numpy(), g['corners_t'].numpy())])
    ref3, ref2 = g['iou_3d'].numpy(), g['iou_2d'].numpy()
    err3, err2 = np.abs(iou_3d - ref3).max(), np.abs(iou_2d - ref2).max()
    ref_err3, ref_err2 = np.abs(ref3 - truth[:, 0]).max(), np.abs(ref2 - truth[:, 1]).max()
    print(f'box_iou_3d max |device - reference|: 3-D {err3:.3g}, BEV {err2:.3g}; |reference - fp64 truth|: {ref_err3:.3g}, {ref_err2:.3g}')
    assert np.abs(iou_3d - truth[:, 0]).max() <= 1e-9 and np.abs(iou_2d - truth[:, 1]).max() <= 1e-9
    assert err3 <= ref_err3 + 1e-9 and err2 <= ref_err2 + 1e-9
    assert ref_err3 <= 5e-5 and ref_err2 <= 5e-5


def _bev(boxes):
    return np.ascontiguousarray(boxes[:, [0, 2, 3, 5, 6]], dtype=np.float32)


@pytest.mark.parametrize('criterion', [-1, 0, 1, 2])
def test_rotate_iou_and_d3_overlap_match_reference(golden, criterion):
    from pvcnn_amd.kitti import d3_box_overlap, rotate_iou_gpu_eval
    o = golden['overlaps']
    boxes, qboxes = o['boxes'].numpy(), o['query_boxes'].numpy()
    got = rotate_iou_gpu_eval(_bev(boxes), _bev(qboxes), criterion)
    assert got.dtype == np.float32 and got.shape == (boxes.shape[0], qboxes.shape[0])
    err = np.abs(got.astype(np.float64) - o['rotate'][criterion].numpy()).max()
    got3 = d3_box_overlap(boxes, qboxes, criterion)
    assert got3.dtype == np.float32
    err3 = np.abs(got3.astype(np.float64) - o['d3'][criterion].numpy()).max()
    print(f'criterion {criterion}: rotate_iou max |error| {err:.3g}, d3_box_overlap {err3:.3g}')
    assert err <= PAIR_TOL and err3 <= PAIR_TOL


@pytest.mark.parametrize('n,k', [(1, 1), (63, 65), (300, 257), (0, 5), (5, 0), (0, 0)])
def test_overlap_shapes_and_edge_tiles(golden, n, k):
    """Every pair of an N x K launch is the pair's own value: rows / columns drawn from the golden boxes give exactly the entries of
    the golden-sized result (tiles of 64 with ragged edges included)."""
    from pvcnn_amd.modules.functional.backend import _backend as be
    o = golden['overlaps']
    boxes, qboxes = o['boxes'].numpy(), o['query_boxes'].numpy()
    rng = np.random.RandomState(n * 1000 + k)
    ri, ci = rng.randint(0, boxes.shape[0], n), rng.randint(0, qboxes.shape[0], k)
    for d3 in (False, True):
        def run(b, q):
            kw = {}
            if d3:
                kw = dict(boxes_3d=torch.from_numpy(np.ascontiguousarray(b)).to(DEV),
                          query_boxes_3d=torch.from_numpy(np.ascontiguousarray(q)).to(DEV))
            return be.rotate_iou(torch.from_numpy(_bev(b)).to(DEV), torch.from_numpy(_bev(q)).to(DEV), -1, **kw).cpu()
        full = run(boxes, qboxes)
        got = run(boxes[ri], qboxes[ci])
        assert tuple(got.shape) == (n, k)
        assert torch.equal(got, full[torch.from_numpy(ri)][:, torch.from_numpy(ci)])


# ---- degenerate geometry against an fp64 truth ---------------------------------------------------------------------------------------
def _corners(center, heading, size):
    """get_box_corners_3d in fp64 (corners (3, 8); sizes (l, w, h)), then fp32 as the meter holds them."""
    l, w, h = size
    x = np.array([l, l, -l, -l, l, l, -l, -l]) / 2
    y = np.array([h, h, h, h, -h, -h, -h, -h]) / 2
    z = np.array([w, -w, -w, w, w, -w, -w, w]) / 2
    c, s = math.cos(heading), math.sin(heading)
    r = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return (r @ np.stack([x, y, z]) + np.asarray(center, dtype=np.float64)[:, None]).astype(np.float32)


# (box 1, box 2, BEV IoU, 3-D IoU, exact): boxes as (center, heading, (l, w, h))
DEGENERATE = {
    'identical_axis_aligned': (((1, 0.5, 10), 0.0, (4, 2, 1.5)), ((1, 0.5, 10), 0.0, (4, 2, 1.5)), 1.0, 1.0, True),
    'identical_rotated': (((3.3, 1.1, 17.2), 0.7, (3.9, 1.6, 1.5)), ((3.3, 1.1, 17.2), 0.7, (3.9, 1.6, 1.5)), 1.0, 1.0, True),
    'touching': (((0, 0, 10), 0.0, (2, 2, 2)), ((2, 0, 10), 0.0, (2, 2, 2)), 0.0, 0.0, True),
    'touching_rotated': (((0, 0, 10), 0.5, (2, 2, 2)), ((2 * math.cos(0.5), 0, 10 - 2 * math.sin(0.5)), 0.5, (2, 2, 2)), 0.0, 0.0,
                         False),
    'inside_half_size': (((0, 0, 10), 0.0, (4, 2, 2)), ((0, 0, 10), 0.0, (2, 1, 1)), 0.25, 0.125, False),
    'half_length_shift': (((0, 0, 10), 0.0, (4, 2, 2)), ((2, 0, 10), 0.0, (4, 2, 2)), 1 / 3, 1 / 3, False),
    'disjoint': (((0, 0, 10), 0.3, (4, 2, 2)), ((9, 0, 20), 1.2, (4, 2, 2)), 0.0, 0.0, True),
    'zero_size': (((0, 0, 10), 0.0, (0, 0, 0)), ((0, 0, 10), 0.0, (4, 2, 2)), 0.0, 0.0, True),
    'both_zero_size': (((0, 0, 10), 0.0, (0, 2, 2)), ((0, 0, 10), 0.0, (0, 2, 2)), 0.0, 0.0, True),
}


def test_degenerate_box_iou_3d():
    from pvcnn_amd.kitti import box_iou_3d
    names = list(DEGENERATE)
    c1 = torch.from_numpy(np.stack([_corners(*DEGENERATE[n][0]) for n in names])).to(DEV)
    ct = torch.from_numpy(np.stack([_corners(*DEGENERATE[n][1]) for n in names])).to(DEV)
    for a, b in ((c1, ct), (ct, c1)):                                   # symmetric
        iou_3d, iou_2d = (t.cpu().tolist() for t in box_iou_3d(a, b))
        for i, name in enumerate(names):
            _, _, want2, want3, exact = DEGENERATE[name]
            assert math.isfinite(iou_2d[i]) and math.isfinite(iou_3d[i]), name
            if exact:
                assert (iou_2d[i], iou_3d[i]) == (want2, want3), (name, iou_2d[i], iou_3d[i])
            else:
                assert abs(iou_2d[i] - want2) <= 1e-6 and abs(iou_3d[i] - want3) <= 1e-6, (name, iou_2d[i], iou_3d[i])


def test_degenerate_rotate_iou_and_d3():
    from pvcnn_amd.kitti import d3_box_overlap, rotate_iou_gpu_eval
    # camera boxes (x, y, z, l, h, w, ry); BEV (x, z, l, w, ry)
    a = np.array([[1.0, 1.5, 10.0, 4.0, 1.5, 2.0, 0.0],          # 0
                  [3.3, 1.5, 17.2, 3.9, 1.5, 1.6, 0.7],          # 1
                  [0.0, 1.0, 30.0, 2.0, 2.0, 2.0, 0.0],          # 2
                  [0.0, 1.0, 40.0, 4.0, 2.0, 2.0, 0.0],          # 3
                  [0.0, 1.0, 50.0, 0.0, 2.0, 2.0, 0.0]])         # 4: zero length
    q = np.array([a[0], a[1],
                  [2.0, 1.0, 30.0, 2.0, 2.0, 2.0, 0.0],          # touches 2
                  [0.0, 0.5, 40.0, 2.0, 1.0, 1.0, 0.0],          # inside 3, half size (height range inside too)
                  a[4]])
    iou = rotate_iou_gpu_eval(_bev(a), _bev(q), -1)
    assert np.isfinite(iou).all()
    want = np.zeros((5, 5))
    want[0, 0] = want[1, 1] = 1.0
    want[3, 3] = 0.25
    assert np.abs(iou - want).max() <= 1e-6 and iou[0, 0] == 1.0 and iou[1, 1] == 1.0 and iou[2, 2] == 0.0
    crit0 = rotate_iou_gpu_eval(_bev(a), _bev(q), 0)               # inter / area(query): 0 for the zero-size query, not NaN
    assert np.isfinite(crit0).all() and crit0[4, 4] == 0.0 and abs(crit0[3, 3] - 1.0) <= 1e-6
    d3 = d3_box_overlap(a, q, -1)
    want[3, 3] = 0.125
    assert np.isfinite(d3).all() and np.abs(d3 - want).max() <= 1e-6 and d3[0, 0] == 1.0 and d3[2, 2] == 0.0


# ---- graph capture and reproducibility ----------------------------------------------------------------------------------------------
def _capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    return graph


def test_configured_meters_capture_into_a_graph_and_are_reproducible(golden):
    """The four meters of configs/kitti/frustum: several updates captured and replayed equal the eager run; two eager runs are
    bit-identical (fp64 sums in a fixed order, integer counts)."""
    configured = ['iou_3d', 'accuracy', 'iou_3d_accuracy', 'iou_3d_class_accuracy']
    batches = [(_to(b['outputs']), _to(b['targets'])) for b in golden['meter']['batches']]

    def eager_run():
        ms = {m: _meter(golden, m) for m in configured}
        for o, t in batches:
            for m in ms.values():
                m.update(o, t)
        return {k: (m.state(), m.compute()) for k, m in ms.items()}
    first, second = eager_run(), eager_run()
    assert first == second
    captured = {m: _meter(golden, m) for m in configured}
    for m in captured.values():
        m.update(*batches[0])                                       # allocates the device state
        m.reset()
    graph = _capture(lambda: [m.update(o, t) for o, t in batches for m in captured.values()])
    for m in captured.values():
        m.reset()
    graph.replay()
    torch.cuda.synchronize()
    assert {k: (m.state(), m.compute()) for k, m in captured.items()} == first
    graph.replay()                                                  # accumulates: twice the counts
    _, counts = captured['iou_3d_accuracy'].state()
    assert counts[0] == 2 * first['iou_3d_accuracy'][0][1][0] and counts[2] == 2 * first['iou_3d_accuracy'][0][1][2]


# ---- --evaluate predictions ---------------------------------------------------------------------------------------------------------
def _update_predictions_fp64(predictions, outputs, rotation_angle, rgb_score, bin_centers, templates, step):
    """evaluate/kitti/frustum/eval.py:180-185 (fp32 decode, as torch) + update_predictions (fp64), restated in numpy."""
    center = outputs['center'].numpy()
    b = center.shape[0]
    hid = outputs['heading_scores'].numpy().argmax(1)
    heading = bin_centers[hid] + outputs['heading_residuals'].numpy()[np.arange(b), hid]           # float32
    sid = outputs['size_scores'].numpy().argmax(1)
    size = templates[sid] + outputs['size_residuals'].numpy()[np.arange(b), sid]                   # float32
    for i in range(b):
        l, w, h = (float(v) for v in size[i])
        x, y, z = (float(v) for v in center[i])
        r = float(rotation_angle[i])
        cx = math.cos(r) * x + math.sin(r) * z
        cy = y + h / 2.0
        cz = math.cos(r) * z - math.sin(r) * x
        r = r + float(heading[i])
        while r > np.pi:
            r = r - 2 * np.pi
        while r < -np.pi:
            r = r + 2 * np.pi
        predictions[step + i] = [h, w, l, cx, cy, cz, r, float(rgb_score[i])]


def test_frustum_box_predictions(golden):
    from pvcnn_amd.kitti import frustum_box_predictions, heading_angle_bin_centers
    nh = golden['num_heading_angle_bins']
    templates = golden['size_templates']
    bin_centers = heading_angle_bin_centers(nh, DEV)
    rng = np.random.RandomState(7)
    batches = golden['meter']['batches']
    total = sum(b['outputs']['center'].shape[0] for b in batches)
    table = torch.zeros((total + 3, 8), dtype=torch.float64, device=DEV)
    want = np.zeros((total + 3, 8))
    step = 0
    for b in batches:
        n = b['outputs']['center'].shape[0]
        targets = {'rotation_angle': torch.from_numpy(rng.uniform(-4, 4, n).astype(np.float32)),
                   'rgb_score': torch.from_numpy(rng.rand(n).astype(np.float32))}
        _update_predictions_fp64(want, b['outputs'], targets['rotation_angle'].numpy(), targets['rgb_score'].numpy(),
                                 bin_centers.cpu().numpy(), templates.numpy(), step)
        step = frustum_box_predictions(table, _to(b['outputs']), targets, step, templates.to(DEV), bin_centers)
    assert step == total
    got = table.cpu().numpy()
    assert np.abs(got - want).max() <= 1e-6
    assert not got[total:].any()                                    # rows past the batches are untouched
    assert (np.abs(got[:total, 6]) <= np.pi).all()
