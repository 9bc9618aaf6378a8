"""The box-overlap kernels (csrc/boxes.hip) against truths that do not share their failure class: box_iou_3d against an exact rational
Sutherland-Hodgman (fractions.Fraction on the fp32 corners), the N x K overlaps and the Frustum-KITTI meter against fp64 / exact
truths on corners decoded in fp64, on seeded families built where clipping code goes wrong (tests/fuzz_cases.py): near-parallel
edges, a vertex on an edge, shared partial edges, nested boxes touching from inside, quarter turns of equal extents, slivers,
clockwise against counter-clockwise corners, touching heights.  Reads nothing outside the repository."""
import math
import time

import numpy as np
import pytest
import torch

import eval_truth as T
import fuzz_cases as F
from test_gpu_kitti import PAIR_TOL, _update_predictions_fp64

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BOX_THREADS, BOX_TILE, MASK_GRID_CAP = 256, 64, 1024


def _be():
    from pvcnn_amd.modules.functional.backend import _backend
    return _backend


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def test_box_iou_3d_against_the_exact_truth():
    """3020 pairs of every family against the exact rational intersection of the same fp32 corners, at the project's bar of 1e-9
    absolute (valid for areas >= 0.01 m^2 and offsets <= 100 m; the generator stays inside, checked on the CPU).  Also: symmetric
    under swapping the arguments, finite and inside [0, 1], exactly 1.0 for bit-identical boxes, exactly 0.0 where the exact
    intersection is empty, a point or a segment.
    Measured on an MI355X: worst |device - exact| 1.6e-13 (slivers) and 1.1e-13 (mirrored slivers), every other family <= 9e-16;
    451 of the pairs have an empty intersection and all give exactly 0.  The exact truth of all pairs takes ~1 s (3.4 s on a slow
    host)."""
    from pvcnn_amd.kitti import box_iou_3d
    names, c1, ct = F.box_iou_pairs()
    t0 = time.time()
    truth = [T.box_iou_exact(a, b) for a, b in zip(c1, ct)]
    print(f'exact truth of {len(names)} pairs: {time.time() - t0:.1f} s')
    want3, want2 = np.array([t[0] for t in truth]), np.array([t[1] for t in truth])
    empty = np.array([t[2] == 0 for t in truth])
    g3, g2 = (t.cpu().numpy() for t in box_iou_3d(_dev(c1), _dev(ct)))
    s3, s2 = (t.cpu().numpy() for t in box_iou_3d(_dev(ct), _dev(c1)))
    names = np.array(names)
    for fam in sorted(set(names)):
        m = names == fam
        print(f'{fam:20s} {m.sum():5d} pairs: max |error| BEV {np.abs(g2 - want2)[m].max():.3g}, 3-D {np.abs(g3 - want3)[m].max():.3g}; '
              f'{int(empty[m].sum())} with an empty intersection')
    assert empty.sum() >= 40 and (~empty).sum() >= 2000
    for got in (g3, g2, s3, s2):
        assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
    assert (g2[empty] == 0).all() and (g3[empty] == 0).all() and (s2[empty] == 0).all() and (s3[empty] == 0).all()
    same = names == 'identical'
    assert same.sum() >= 50 and (g2[same] == 1.0).all() and (g3[same] == 1.0).all()
    assert np.abs(g2 - want2).max() <= 1e-9 and np.abs(g3 - want3).max() <= 1e-9
    assert np.abs(s2 - want2).max() <= 1e-9 and np.abs(s3 - want3).max() <= 1e-9
    assert np.abs(g2 - s2).max() <= 1e-9 and np.abs(g3 - s3).max() <= 1e-9               # symmetric


def _overlaps(boxes, qboxes, criterion, d3):
    kw = {}
    if d3:
        kw = dict(boxes_3d=_dev(boxes, np.float64), query_boxes_3d=_dev(qboxes, np.float64))
    return _be().rotate_iou(_dev(F.bev(boxes)), _dev(F.bev(qboxes)), criterion, **kw)


@pytest.fixture(scope='module')
def overlap_case():
    boxes, qboxes = F.overlap_boxes()
    return boxes, qboxes, T.pair_geometry_f64(F.bev(boxes), F.bev(qboxes))


@pytest.mark.parametrize('criterion', [-1, 0, 1, 2])
def test_rotate_iou_and_d3_against_the_fp64_truth(overlap_case, criterion):
    """The N x K overlaps (N = K > 64: several ragged 64-box tiles; the designed pair of every family on the diagonal) against the
    fp64 truth on corners formed in fp64.  The device forms its corners in fp32 with cosf / sinf, so the bar is per pair and derived
    (eval_truth.pair_bound): 2 * delta * 2 * (perim_a + perim_b) / max(area_a, area_b) + 2^-23, delta = 8 fp32 ulps of the pair's
    largest |corner coordinate|.  The 3-D form carries the same bound over (see the comment below).
    Measured on an MI355X: worst |error| / bound 0.004 (BEV) and 0.005 (3-D) over the four criteria; the largest absolute errors are
    3.0e-5 (BEV) and 3.8e-5 (3-D), on slivers -- above PAIR_TOL, which holds against the reference's fp32 corners, not against
    corners formed in fp64."""
    boxes, qboxes, geo = overlap_case
    assert boxes.shape[0] > BOX_TILE and boxes.shape[0] % BOX_TILE != 0
    bound = T.pair_bound(geo, criterion)
    got = _overlaps(boxes, qboxes, criterion, False).cpu().numpy().astype(np.float64)
    want = T.rotate_iou_truth(geo, criterion)
    ratio = np.abs(got - want) / bound
    diag = np.abs(np.diag(got) - np.diag(want))
    print(f'criterion {criterion}: rotate_iou worst |error| / bound {ratio.max():.3f} (max |error| {np.abs(got - want).max():.3g}; '
          f'designed pairs {diag.max():.3g}; PAIR_TOL {PAIR_TOL})')
    assert np.isfinite(got).all() and (got >= 0).all() and ratio.max() <= 1.0
    if criterion != 2:
        assert (got <= 1).all()
    got3 = _overlaps(boxes, qboxes, criterion, True).cpu().numpy().astype(np.float64)
    want3 = T.d3_overlap_truth(geo, boxes, qboxes, criterion)
    # d3 value = iw * I / ua: the sizes and heights are fp64 on both sides, so only the BEV intersection I differs.  ua >= the volume
    # of either box >= iw * its BEV area, so the value moves by no more than the BEV ratio of the same denominator would: criterion -1
    # keeps its bound; criterion 0 divides by the BOX's volume and 1 by the QUERY's (the BEV form has them the other way round);
    # criterion 2 is iw * I.  The 2^-23 term covers the float32 BEV intersection and the float32 store.
    iw = np.maximum(np.minimum(boxes[:, 1][:, None], qboxes[:, 1][None, :]) -
                    np.maximum((boxes[:, 1] - boxes[:, 4])[:, None], (qboxes[:, 1] - qboxes[:, 4])[None, :]), 0.0)
    bound3 = {-1: bound, 0: T.pair_bound(geo, 1), 1: T.pair_bound(geo, 0), 2: bound * np.maximum(iw, 1.0)}[criterion]
    ratio3 = np.abs(got3 - want3) / bound3
    print(f'criterion {criterion}: d3_box_overlap worst |error| / bound {ratio3.max():.3f} (max |error| {np.abs(got3 - want3).max():.3g})')
    assert np.isfinite(got3).all() and (got3 >= 0).all() and ratio3.max() <= 1.0


def test_every_entry_equals_its_own_1x1_launch():
    """Each entry of a 70 x 67 launch (two ragged tiles each way) is bit-equal to the same pair computed alone."""
    boxes, qboxes = F.overlap_boxes()
    boxes, qboxes = boxes[:70], qboxes[-67:]
    for d3 in (False, True):
        for criterion in (-1, 2):
            full = _overlaps(boxes, qboxes, criterion, d3)
            bb, qq = _dev(F.bev(boxes)), _dev(F.bev(qboxes))
            b3, q3 = _dev(boxes, np.float64), _dev(qboxes, np.float64)
            singles = []
            for i in range(boxes.shape[0]):
                for j in range(qboxes.shape[0]):
                    kw = dict(boxes_3d=b3[i:i + 1], query_boxes_3d=q3[j:j + 1]) if d3 else {}
                    singles.append(_be().rotate_iou(bb[i:i + 1], qq[j:j + 1], criterion, **kw))
            singles = torch.cat(singles).view(full.shape)
            assert torch.equal(singles.view(torch.int32), full.view(torch.int32)), (d3, criterion)


NH, NS = 12, 8
TEMPLATES = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73], [5.0, 1.9, 2.2], [10.0, 2.5, 3.2], [0.8, 0.5, 1.1],
                      [12.0, 2.6, 3.5], [2.0, 1.0, 1.5]], dtype=np.float32)


def _frustum_batch(rng, b):
    """Heads and targets of B boxes: the target near the prediction (so IoUs spread over (0, 1)); NaN head scores (the NaN wins the
    argmax); target ids outside their tables (IoU 0); a class id absent from class_ids."""
    o = dict(center=np.c_[rng.uniform(-20, 20, b), rng.uniform(0, 2, b), rng.uniform(5, 60, b)].astype(np.float32),
             heading_scores=rng.standard_normal((b, NH)).astype(np.float32),
             heading_residuals=rng.uniform(-0.25, 0.25, (b, NH)).astype(np.float32),
             size_scores=rng.standard_normal((b, NS)).astype(np.float32),
             size_residuals=rng.uniform(-0.2, 0.2, (b, NS, 3)).astype(np.float32))
    o['heading_scores'][rng.random((b, NH)) < 0.02] = np.nan
    o['size_scores'][rng.random((b, NS)) < 0.02] = np.nan
    hid, sid = T.first_argmax(o['heading_scores'], 1), T.first_argmax(o['size_scores'], 1)
    hid_t = np.where(rng.random(b) < 0.8, hid, rng.integers(0, NH, b)).astype(np.int64)
    sid_t = np.where(rng.random(b) < 0.8, sid, rng.integers(0, NS, b)).astype(np.int64)
    bad = np.arange(b) % 50 == 7
    hid_t[bad] = np.array([-1, NH, NH + 3], dtype=np.int64)[np.arange(bad.sum()) % 3]
    bad2 = np.arange(b) % 50 == 23
    sid_t[bad2] = np.array([NS, -2, NS + 1], dtype=np.int64)[np.arange(bad2.sum()) % 3]
    t = dict(center=(o['center'] + rng.normal(0, 0.15, (b, 3))).astype(np.float32), heading_bin_id=hid_t,
             heading_residual=(o['heading_residuals'][np.arange(b), hid] + rng.normal(0, 0.05, b)).astype(np.float32),
             size_template_id=sid_t,
             size_residual=(o['size_residuals'][np.arange(b), sid] + rng.normal(0, 0.05, (b, 3))).astype(np.float32),
             class_id=rng.integers(0, 4, b).astype(np.int64))                            # class 3 is absent from class_ids
    return o, t, bad | bad2


def _decoded_corners(center, heading32, size32):
    """make_corners in fp64 on the fp32 decode: (3, 8) fp64 corners."""
    return T.box_corners_f64([float(v) for v in center], float(heading32), [float(v) for v in size32])


@pytest.mark.parametrize('b', [1, 255, 256, 257, 1000])
def test_frustum_meter_update_boxes(b):
    """One workgroup striding over B by 256.  Counts are exact; the IoU sums match an fp64 truth built from box_iou_exact on corners
    decoded in fp64, within the sum of the per-box derived corner bounds.  Boxes whose exact 3-D IoU lies within its bound of a
    threshold (0.5 / 0.7) may be counted either way; they are counted as the device did only if the truth is that close.  The tables
    are views between sentinel entries: `hid >= 0 && hid < NH && sid >= 0 && sid < NS` is tested before either table is read.
    Measured on an MI355X: |sum error| 1.4e-7 (B = 1) to 4.6e-6 (B = 1000) against bounds of 1.1e-3 to 0.61: ratio < 1e-4."""
    rng = np.random.default_rng(90 + b)
    o, t, bad = _frustum_batch(rng, b)
    bins_all = np.r_[[7.0] * 8, np.arange(0, 2 * np.pi, 2 * np.pi / NH, dtype=np.float32), [7.0] * 8].astype(np.float32)
    tmpl_all = np.r_[np.full((8, 3), 2.0, dtype=np.float32), TEMPLATES, np.full((8, 3), 2.0, dtype=np.float32)]
    bins_dev, tmpl_dev = _dev(bins_all), _dev(tmpl_all)
    bins, tmpl = bins_dev[8:8 + NH], tmpl_dev[8:8 + NS]
    bin_centers = bins_all[8:8 + NH]
    class_ids = torch.tensor([0, 1, 2], dtype=torch.int64, device=DEV)
    thresholds = np.array([0.7, 0.5, 0.5])
    sums = torch.tensor([1.5, 2.5], dtype=torch.float64, device=DEV)                     # accumulates into a non-zero state
    counts = torch.arange(9, dtype=torch.int64, device=DEV)
    heads = tuple(_dev(o[k]) for k in ('center', 'heading_scores', 'heading_residuals', 'size_scores', 'size_residuals'))
    tgt = tuple(_dev(t[k]) for k in ('center', 'heading_bin_id', 'heading_residual', 'size_template_id', 'size_residual', 'class_id'))
    _be().frustum_meter_update(heads, tgt, bins, tmpl, class_ids, _dev(thresholds), sums, counts)

    hid, sid = T.first_argmax(o['heading_scores'], 1), T.first_argmax(o['size_scores'], 1)
    heading = bin_centers[hid] + o['heading_residuals'][np.arange(b), hid]               # fp32, as torch adds them
    size = TEMPLATES[sid] + o['size_residuals'][np.arange(b), sid]
    iou3, iou2, bnd = np.zeros(b), np.zeros(b), np.zeros(b)
    for i in range(b):
        if bad[i]:
            continue                                                                     # a target id outside its table: IoU 0
        heading_t = bin_centers[t['heading_bin_id'][i]] + t['heading_residual'][i]
        size_t = TEMPLATES[t['size_template_id'][i]] + t['size_residual'][i]
        cp, cq = _decoded_corners(o['center'][i], heading[i], size[i]), _decoded_corners(t['center'][i], heading_t, size_t)
        iou3[i], iou2[i], _ = T.box_iou_exact(cp, cq)
        delta = float(T.corner_delta(max(np.abs(cp).max(), np.abs(cq).max())))
        perim = 2 * (abs(size[i][0]) + abs(size[i][1]) + abs(size_t[0]) + abs(size_t[1]))
        area = max(abs(size[i][0] * size[i][1]), abs(size_t[0] * size_t[1]))
        bnd[i] = 2 * delta * 2 * perim / area + 2 * 3 * 2 * delta / min(abs(size[i][2]), abs(size_t[2]))   # BEV, and the heights
    got_sums, got_counts = sums.cpu().numpy() - [1.5, 2.5], counts.cpu().numpy() - np.arange(9)
    err2, err3 = abs(got_sums[0] - iou2.sum()), abs(got_sums[1] - iou3.sum())
    print(f'B={b}: |sum error| BEV {err2:.3g}, 3-D {err3:.3g}; bound {bnd.sum():.3g}; ratio {max(err2, err3) / bnd.sum():.3f}')
    assert (size > 0.05).all() and bad.sum() == (np.arange(b) % 50 == 7).sum() + (np.arange(b) % 50 == 23).sum()
    assert max(err2, err3) <= bnd.sum()
    assert got_counts[0] == b and got_counts[1] == 0
    cls = t['class_id']
    seen = [int((cls == k).sum()) for k in range(3)]
    assert got_counts[6:9].tolist() == seen
    if b >= 255:
        assert sum(seen) < b                                                             # class 3 is seen nowhere

    def count_range(thr, mask):
        sure = int(((iou3 >= thr + bnd) & mask).sum())
        return sure, sure + int(((np.abs(iou3 - thr) < bnd) & mask).sum())
    lo, hi = count_range(0.7, np.ones(b, dtype=bool))
    assert lo <= got_counts[2] <= hi and hi - lo <= max(2, b // 50)
    for k in range(3):
        lo, hi = count_range(thresholds[k], cls == k)
        assert lo <= got_counts[3 + k] <= hi and hi - lo <= max(2, b // 50)


def test_frustum_meter_target_ids_outside_their_tables_give_iou_0():
    """Every box of the batch has a target id outside its table, and the target geometry is the prediction's own: with the guard the
    sums stay exactly 0; without it the sentinel table entries (a 2 x 2 x 2 m box at heading 7) would overlap the prediction."""
    rng = np.random.default_rng(95)
    b = 300
    o, t, _ = _frustum_batch(rng, b)
    t['center'] = o['center'].copy()
    t['heading_bin_id'] = np.array([-1, NH, NH + 3, -8], dtype=np.int64)[np.arange(b) % 4]
    t['size_template_id'] = np.array([NS, -2, NS + 7, 0, 3], dtype=np.int64)[np.arange(b) % 5]
    t['size_template_id'][(np.arange(b) % 4 == 3) & (np.arange(b) % 5 >= 3)] = -1
    bins_all = np.r_[[7.0] * 8, np.arange(0, 2 * np.pi, 2 * np.pi / NH, dtype=np.float32), [7.0] * 8].astype(np.float32)
    tmpl_all = np.r_[np.full((8, 3), 2.0, dtype=np.float32), TEMPLATES, np.full((8, 3), 2.0, dtype=np.float32)]
    bins_dev, tmpl_dev = _dev(bins_all), _dev(tmpl_all)
    sums = torch.zeros(2, dtype=torch.float64, device=DEV)
    counts = torch.zeros(9, dtype=torch.int64, device=DEV)
    heads = tuple(_dev(o[k]) for k in ('center', 'heading_scores', 'heading_residuals', 'size_scores', 'size_residuals'))
    tgt = tuple(_dev(t[k]) for k in ('center', 'heading_bin_id', 'heading_residual', 'size_template_id', 'size_residual', 'class_id'))
    _be().frustum_meter_update(heads, tgt, bins_dev[8:8 + NH], tmpl_dev[8:8 + NS], torch.tensor([0, 1, 2], dtype=torch.int64, device=DEV),
                               _dev(np.array([0.7, 0.5, 0.5])), sums, counts)
    cls = t['class_id']
    assert sums.tolist() == [0.0, 0.0]
    assert counts.tolist() == [b, 0, 0, 0, 0, 0] + [int((cls == k).sum()) for k in range(3)]


def test_frustum_meter_mask_accuracy_at_scale():
    """B * N = 300,033 > 1024 * 256 (the grid cap): NaN logits (the NaN wins), exact counts, accumulation across two updates."""
    b, c, n = 3, 2, 100011
    assert b * n > MASK_GRID_CAP * BOX_THREADS
    rng = np.random.default_rng(97)
    x = (rng.integers(-2, 3, size=(b, c, n)) * 0.5).astype(np.float32)
    x[rng.random((b, c, n)) < 0.02] = np.nan
    t = rng.integers(-1, 3, size=(b, n), dtype=np.int64)
    hits = int((T.first_argmax(x, 1) == t).sum())
    counts = torch.zeros(9, dtype=torch.int64, device=DEV)
    for k in (1, 2):
        _be().frustum_meter_accuracy(_dev(x), _dev(t), counts)
        assert counts.tolist() == [k * b * n, k * hits] + [0] * 7
    assert 0 < hits < b * n


def test_frustum_predictions_angle_wrap():
    """Sums of rotation angle and heading that land exactly on +-pi (the inequalities are strict: they stay), one ulp beyond (they
    wrap), and tens of turns away (inside the 64-step cap).  Bar: 1e-6, the existing one."""
    from pvcnn_amd.kitti import frustum_box_predictions, heading_angle_bin_centers
    rng = np.random.default_rng(101)
    b = 300
    o, _, _ = _frustum_batch(rng, b)
    o['heading_scores'] = np.nan_to_num(o['heading_scores'])
    o['size_scores'] = np.nan_to_num(o['size_scores'])
    bin_centers = heading_angle_bin_centers(NH, DEV)
    bc = bin_centers.cpu().numpy()
    kinds = np.arange(b) % 6
    o['heading_scores'][(kinds == 1) | (kinds == 3), 0] = 10.0                           # a heading near 0: |-pi - heading| < 4, see below
    hid = o['heading_scores'].argmax(1)
    heading = (bc[hid] + o['heading_residuals'][np.arange(b), hid]).astype(np.float64)   # the fp32 decode, as a double
    rot = rng.uniform(-4, 4, b)
    for i in range(b):
        target = [math.pi, -math.pi, np.nextafter(math.pi, 4), np.nextafter(-math.pi, -4), None, None][kinds[i]]
        if target is not None:
            r = target - heading[i]
            for _ in range(4):                                                           # make the fp64 sum land on the target exactly
                if r + heading[i] == target:                                             # (|r| < 4: r is as fine-grained as pi)
                    break
                r = np.nextafter(r, math.copysign(np.inf, target - (r + heading[i])))
            rot[i] = r
        else:
            rot[i] = rng.uniform(-3, 3) + 2 * math.pi * rng.integers(-29, 30)            # up to 29 turns: |angle| < 190 rad
    exact = np.array([rot[i] + heading[i] for i in range(b)])
    assert (exact[kinds == 0] == math.pi).all() and (exact[kinds == 1] == -math.pi).all()
    assert (exact[kinds == 2] > math.pi).all() and (exact[kinds == 3] < -math.pi).all() and np.abs(exact).max() > 150
    rgb = rng.random(b)
    table = torch.full((b + 5, 8), -3.0, dtype=torch.float64, device=DEV)
    want = np.full((b + 5, 8), -3.0)
    outputs = {k: torch.from_numpy(v) for k, v in o.items()}
    _update_predictions_fp64(want, outputs, rot, rgb, bc, TEMPLATES, 2)
    step = frustum_box_predictions(table, {k: v.to(DEV) for k, v in outputs.items()},
                                   {'rotation_angle': torch.from_numpy(rot), 'rgb_score': torch.from_numpy(rgb)}, 2,
                                   torch.from_numpy(TEMPLATES).to(DEV), bin_centers)
    got = table.cpu().numpy()
    assert step == b + 2 and (got[:2] == -3.0).all() and (got[b + 2:] == -3.0).all()
    assert np.abs(got - want).max() <= 1e-6
    ang = got[2:b + 2, 6]
    assert (ang[kinds == 0] == math.pi).all() and (ang[kinds == 1] == -math.pi).all()     # exactly on +-pi: not wrapped
    assert (ang[kinds == 2] < 0).all() and (ang[kinds == 3] > 0).all()                    # one ulp beyond: wrapped once
    assert (np.abs(ang) <= math.pi).all()
