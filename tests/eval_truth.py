"""Plain references for the evaluation and box-overlap kernels (csrc/evaluate.hip, csrc/boxes.hip): numpy and `fractions` only -- no
torch device code, no oracle, nothing of pvcnn_amd.  tests/test_eval_truth_host.py proves these against the golden files (the
reference's own outputs) before tests/test_gpu_eval_fuzz.py and tests/test_gpu_boxes_fuzz.py judge the kernels by them.

Conventions follow the kernels' stated contracts:
  * a vote is dropped when its confidence is <= 0 or NaN, its shuffled index is outside [0, map_stride) (with a mapping) or its
    target is outside [0, P);
  * argmax is the first maximum and a NaN beats every number (torch.argmax);
  * a box of zero area intersects nothing and a ratio with a zero denominator is 0.
"""
import math
from fractions import Fraction

import numpy as np

# ---- vote merge ------------------------------------------------------------------------------------------------------------------


def vote_targets(shuffled, mapping, num_points):
    """-> (targets (B*V) int64, valid (B*V) bool) of the votes in (b, p) order."""
    shuffled = np.asarray(shuffled, dtype=np.int64)
    shuffled = shuffled.reshape(1, -1) if shuffled.ndim == 1 else shuffled
    b, v = shuffled.shape
    idx = shuffled.reshape(-1)
    if mapping is None:
        t, ok = idx, np.ones(idx.shape, dtype=bool)
    else:
        mapping = np.asarray(mapping, dtype=np.int64)
        m = mapping.shape[1]
        ok = (idx >= 0) & (idx < m)
        rows = np.repeat(np.arange(b, dtype=np.int64), v)
        t = np.where(ok, mapping[rows, np.where(ok, idx, 0)], -1)
    return t, ok & (t >= 0) & (t < num_points)


def merge_serial(state_conf, state_pred, conf, pred, shuffled, mapping=None):
    """update_scene_predictions / update_shape_predictions, literally: for b, for p: if conf > state[t]: replace.  In place on
    state_conf (P) float32 and state_pred (P) int64."""
    shuffled = np.asarray(shuffled, dtype=np.int64)
    shuffled = shuffled.reshape(1, -1) if shuffled.ndim == 1 else shuffled
    b, v = shuffled.shape
    conf = np.asarray(conf, dtype=np.float32).reshape(b, v)
    pred = np.asarray(pred).reshape(b, v)
    num_points = state_conf.shape[0]
    for i in range(b):
        for p in range(v):
            idx = int(shuffled[i, p])
            if mapping is not None:
                if idx < 0 or idx >= mapping.shape[1]:
                    continue
                t = int(mapping[i, idx])
            else:
                t = idx
            if t < 0 or t >= num_points:
                continue
            c = conf[i, p]
            if not c > 0:                                  # conf <= 0, -0.0 or NaN: dropped
                continue
            if c > state_conf[t]:
                state_conf[t] = c
                state_pred[t] = pred[i, p]


def merge_vectorised(state_conf, state_pred, conf, pred, shuffled, mapping=None):
    """The same rule at millions of votes: per target the largest confidence of the call, among equal ones the first vote in (b, p)
    order; it replaces the state only where strictly greater.  In place."""
    t, valid = vote_targets(shuffled, mapping, state_conf.shape[0])
    c = np.asarray(conf, dtype=np.float32).reshape(-1)
    q = np.asarray(pred).reshape(-1)
    with np.errstate(invalid='ignore'):
        valid = valid & (c > 0)
    sel = np.flatnonzero(valid)                            # ascending vote order
    if sel.size == 0:
        return
    order = np.argsort(t[sel], kind='stable')              # groups of one target, vote order kept inside a group
    sel = sel[order]
    ts, cs = t[sel], c[sel]
    starts = np.flatnonzero(np.r_[True, ts[1:] != ts[:-1]])
    seg_max = np.maximum.reduceat(cs, starts)
    seg_id = np.cumsum(np.r_[True, ts[1:] != ts[:-1]]) - 1
    pos = np.where(cs == seg_max[seg_id], np.arange(cs.size), cs.size)
    first = np.minimum.reduceat(pos, starts)               # the first vote holding the group's maximum
    tw, cw, pw = ts[starts], cs[first], q[sel[first]]
    upd = cw > state_conf[tw]
    state_conf[tw[upd]] = cw[upd]
    state_pred[tw[upd]] = pw[upd]


# ---- histograms and meters -------------------------------------------------------------------------------------------------------


def class_slots(values, num_classes, wrap_negative):
    """-> (slot, counted): numpy indexing when wrap_negative (a value in [-C, 0) counts for value + C); anything else outside
    [0, C) is counted nowhere."""
    v = np.asarray(values, dtype=np.int64).copy()
    if wrap_negative:
        neg = (v < 0) & (v >= -num_classes)
        v[neg] += num_classes
    ok = (v >= 0) & (v < num_classes)
    return v, ok


def seg_counts_truth(gt, pred, num_classes, wrap_negative=True):
    """(3, C) int64 [seen; positive; correct] of update_stats: correct counts a point whose raw values are equal, for gt's class."""
    gt, pred = np.asarray(gt, dtype=np.int64).reshape(-1), np.asarray(pred, dtype=np.int64).reshape(-1)
    gs, gok = class_slots(gt, num_classes, wrap_negative)
    ps, pok = class_slots(pred, num_classes, wrap_negative)
    out = np.zeros((3, num_classes), dtype=np.int64)
    out[0] = np.bincount(gs[gok], minlength=num_classes)
    out[1] = np.bincount(ps[pok], minlength=num_classes)
    hit = gok & (gt == pred)
    out[2] = np.bincount(gs[hit], minlength=num_classes)
    return out


def first_argmax(x, axis):
    """torch.argmax: the first maximum along `axis`; the first NaN where there is one."""
    x = np.asarray(x)
    nan = np.isnan(x)
    with np.errstate(invalid='ignore'):
        k = np.argmax(np.where(nan, -np.inf, x), axis=axis)
    return np.where(nan.any(axis=axis), np.argmax(nan, axis=axis), k)


def meter_s3dis_truth(logits, targets, num_classes):
    """(3C + 2) int64 [seen C | positive C | correct C | numel | correct] of one MeterS3DIS.update; a target outside [0, C) is seen
    nowhere and never correct."""
    logits, targets = np.asarray(logits), np.asarray(targets, dtype=np.int64)
    c = num_classes
    k = first_argmax(logits, 1).reshape(-1)
    t = targets.reshape(-1)
    ok = (t >= 0) & (t < c)
    out = np.zeros(3 * c + 2, dtype=np.int64)
    out[:c] = np.bincount(t[ok], minlength=c)
    out[c:2 * c] = np.bincount(k, minlength=c)
    hit = ok & (t == k)
    out[2 * c:3 * c] = np.bincount(t[hit], minlength=c)
    out[3 * c] = t.size
    out[3 * c + 1] = int(hit.sum())
    return out


def meter_shapenet_rows_truth(logits, targets, ranges, max_parts):
    """Rows (B, max_parts + 1, 2) int32 of one MeterShapeNet.update: [(s, e), (intersection, union) of part classes s .. e-1, zeros].
    The range is ranges[targets[b, 0]]; a label outside the table or a bad row (s < 0, e > C, s >= e, e - s > max_parts) gives
    (0, 0) and no counts."""
    logits, targets = np.asarray(logits), np.asarray(targets, dtype=np.int64)
    ranges = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    b, c, n = logits.shape
    rows = np.zeros((b, max_parts + 1, 2), dtype=np.int32)
    for i in range(b):
        label = int(targets[i, 0])
        s = e = 0
        if 0 <= label < ranges.shape[0]:
            s, e = int(ranges[label, 0]), int(ranges[label, 1])
            if s < 0 or e > c or s >= e or e - s > max_parts:
                s = e = 0
        rows[i, 0] = (s, e)
        if s >= e:
            continue
        k = first_argmax(logits[i, s:e], 0) + s
        t = targets[i]
        for j in range(s, e):
            it, ip = t == j, k == j
            rows[i, 1 + j - s] = (int((it & ip).sum()), int((it | ip).sum()))
    return rows


# ---- softmax confidence ----------------------------------------------------------------------------------------------------------


def vote_confidence_truth(logits, lo, hi):
    """softmax(x, 1)[:, lo:hi].max(1) in fp64 on fp32 logits (B, C, N); lo / hi ints or per-cloud arrays (clamped to [0, C]; an empty
    range gives conf 0, pred -1).  -> dict(conf, pred, second (the runner-up probability inside the range; -inf for a
    one-class range, whose prediction cannot be anything else),
    dist (m - x_pred), dist2 (m - x_runner_up)), arrays (B, N)."""
    x = np.asarray(logits)
    b, c, n = x.shape
    los = np.broadcast_to(np.asarray(lo, dtype=np.int64), (b,))
    his = np.broadcast_to(np.asarray(hi, dtype=np.int64), (b,))
    out = {k: np.zeros((b, n)) for k in ('conf', 'second', 'dist', 'dist2')}
    out['pred'] = np.full((b, n), -1, dtype=np.int64)
    for i in range(b):
        l, h = max(int(los[i]), 0), min(int(his[i]), c)
        if l >= h:
            continue
        xi = x[i].astype(np.float64)
        m = xi.max(0)
        with np.errstate(under='ignore'):
            e = np.exp(xi - m)
            p = e / e.sum(0)
        pr = p[l:h]
        k = np.argmax(pr, 0)                               # the first maximum
        cols = np.arange(n)
        out['conf'][i] = pr[k, cols]
        out['pred'][i] = k + l
        d1 = m - xi[k + l, cols]
        out['dist'][i] = np.where(np.isfinite(d1), d1, 0.0)               # a probability of exactly 0 has no rounding
        if h - l > 1:
            rest = pr.copy()
            rest[k, cols] = -1.0
            k2 = np.argmax(rest, 0)
            out['second'][i] = rest[k2, cols]
            d2 = m - xi[k2 + l, cols]
            out['dist2'][i] = np.where(np.isfinite(d2), d2, 0.0)
        else:
            out['second'][i] = -np.inf
    return out


FLT_MIN = 2.0 ** -126       # below it fp32 has absolute, not relative, precision (and a flushed denormal is 0)


def confidence_rel_bound(num_classes, dist):
    """2 * ((C + 3) + |x_k - m|) * 2^-24: the serial fp32 sum of C terms, one expf each, one division; the rounding of x_k - m
    magnified by the exponential; the factor 2 is margin for expf's last bits."""
    return 2.0 * ((num_classes + 3) + np.abs(dist)) * 2.0 ** -24


def confidence_excluded(truth, num_classes):
    """Points whose in-range fp64 top-two gap does not exceed the rounding bounds of the two probabilities (each at its own
    distance from the maximum, plus the fp32 underflow floor): their class cannot be told in fp32."""
    b1 = confidence_rel_bound(num_classes, truth['dist']) * truth['conf']
    b2 = confidence_rel_bound(num_classes, truth['dist2']) * np.maximum(truth['second'], 0.0)
    return (truth['pred'] >= 0) & ~(truth['conf'] - truth['second'] > b1 + b2 + 2 * FLT_MIN)


# ---- boxes -----------------------------------------------------------------------------------------------------------------------


def _area2(poly):
    return sum(poly[i - 1][0] * poly[i][1] - poly[i][0] * poly[i - 1][1] for i in range(len(poly)))


def _ccw(poly):
    return poly if _area2(poly) >= 0 else poly[::-1]


def _clip(p, q):
    """Sutherland-Hodgman: polygon p clipped by the closed half-planes of the counter-clockwise convex polygon q, in the number type
    of the coordinates (Fraction: no rounding at all)."""
    out = list(p)
    for i in range(len(q)):
        a, b = q[i], q[(i + 1) % len(q)]
        ex, ey = b[0] - a[0], b[1] - a[1]
        inp, out = out, []
        if not inp:
            break
        f = [ex * (v[1] - a[1]) - ey * (v[0] - a[0]) for v in inp]
        for j in range(len(inp)):
            s_, e_, fs, fe = inp[j - 1], inp[j], f[j - 1], f[j]
            if (fs < 0) != (fe < 0):
                t = fs / (fs - fe)
                out.append((s_[0] + t * (e_[0] - s_[0]), s_[1] + t * (e_[1] - s_[1])))
            if fe >= 0:
                out.append(e_)
    return out


def quad_intersection(p, q):
    """Area of the intersection of two convex quads (lists of 4 (x, y)) given in either orientation, in their number type."""
    p, q = _ccw(list(p)), _ccw(list(q))
    if _area2(p) == 0 or _area2(q) == 0:
        return _area2(p) * 0
    out = _clip(p, q)
    return _area2(out) / 2 if len(out) >= 3 else _area2(p) * 0


def quad_intersection_exact(p, q):
    """quad_intersection over the rationals: the coordinates (fp32 or fp64 values) are converted exactly.  -> Fraction."""
    fr = lambda poly: [(Fraction(float(x)), Fraction(float(y))) for x, y in poly]      # noqa: E731
    return quad_intersection(fr(p), fr(q)) + Fraction(0)


def _ratio(num, den):
    return num / den if den > 0 else num * 0


def box_iou_exact(c1, ct):
    """get_box_iou_3d on (3, 8) corner sets, exactly: BEV quads are (x, z) of corners 3, 2, 1, 0; heights from y of corners 0 and 4;
    a volume is BEV area times |y0 - y4|.  -> (iou_3d, iou_2d, intersection area) as (float, float, Fraction)."""
    c1, ct = np.asarray(c1), np.asarray(ct)
    fr = lambda v: Fraction(float(v))                                                   # noqa: E731
    quad = lambda c: [(fr(c[0, i]), fr(c[2, i])) for i in (3, 2, 1, 0)]                # noqa: E731
    p, q = quad(c1), quad(ct)
    a1, a2 = abs(_area2(p)) / 2, abs(_area2(q)) / 2
    inter = quad_intersection(p, q) + Fraction(0)
    iou_2d = _ratio(inter, a1 + a2 - inter)
    h = max(Fraction(0), min(fr(c1[1, 0]), fr(ct[1, 0])) - max(fr(c1[1, 4]), fr(ct[1, 4])))
    v1, v2 = a1 * abs(fr(c1[1, 0]) - fr(c1[1, 4])), a2 * abs(fr(ct[1, 0]) - fr(ct[1, 4]))
    iou_3d = _ratio(inter * h, v1 + v2 - inter * h)
    return float(iou_3d), float(iou_2d), inter


def box_corners_f64(center, heading, size):
    """get_box_corners_3d (with_flip=False) in fp64: (3, 8) corners of a box (center (x, y, z), heading, size (l, w, h))."""
    l, w, h = (float(v) for v in size)
    x = np.array([l, l, -l, -l, l, l, -l, -l]) / 2
    y = np.array([h, h, h, h, -h, -h, -h, -h]) / 2
    z = np.array([w, -w, -w, w, w, -w, -w, w]) / 2
    c, s = math.cos(float(heading)), math.sin(float(heading))
    r = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return r @ np.stack([x, y, z]) + np.asarray(center, dtype=np.float64)[:, None]


def rbox_corners_f64(box):
    """rbbox_to_corners of an rbox (x, y, dx, dy, angle), the fp32 parameters taken to fp64 first: corners (-dx/2, -dy/2),
    (-dx/2, dy/2), (dx/2, dy/2), (dx/2, -dy/2) turned by the angle, x = cos*cx + sin*cy + x0, y = -sin*cx + cos*cy + y0."""
    x0, y0, dx, dy, a = (float(np.float32(v)) for v in box)
    c, s = math.cos(a), math.sin(a)
    hx, hy = dx / 2, dy / 2
    return [(c * cx + s * cy + x0, -s * cx + c * cy + y0) for cx, cy in ((-hx, -hy), (-hx, hy), (hx, hy), (hx, -hy))]


def criterion_value(inter, area_box, area_query, criterion):
    """rotate_iou_gpu_eval's criteria: -1 IoU, 0 inter / area(query box), 1 inter / area(box), other the intersection."""
    if criterion == -1:
        return _ratio(inter, area_box + area_query - inter)
    if criterion == 0:
        return _ratio(inter, area_query)
    if criterion == 1:
        return _ratio(inter, area_box)
    return inter


def pair_geometry_f64(boxes, query_boxes):
    """-> (inter, area_box, area_query, perimeter_box, perimeter_query, max |corner coordinate|): (N, K) / (N) / (K) fp64 arrays of
    the rboxes' fp64 corners."""
    cb = [_ccw(rbox_corners_f64(b)) for b in boxes]
    cq = [_ccw(rbox_corners_f64(b)) for b in query_boxes]
    area = lambda poly: _area2(poly) / 2                                                # noqa: E731
    perim = lambda poly: sum(math.hypot(poly[i][0] - poly[i - 1][0], poly[i][1] - poly[i - 1][1]) for i in range(4))   # noqa: E731
    big = lambda poly: max(max(abs(x), abs(y)) for x, y in poly)                        # noqa: E731
    inter = np.zeros((len(cb), len(cq)))
    for i, p in enumerate(cb):
        for j, q in enumerate(cq):
            inter[i, j] = quad_intersection(q, p)
    return (inter, np.array([area(p) for p in cb]), np.array([area(p) for p in cq]), np.array([perim(p) for p in cb]),
            np.array([perim(p) for p in cq]), np.array([big(p) for p in cb]), np.array([big(p) for p in cq]))


def rotate_iou_truth(geometry, criterion):
    inter, ab, aq = geometry[:3]
    out = np.zeros_like(inter)
    for i in range(inter.shape[0]):
        for j in range(inter.shape[1]):
            out[i, j] = criterion_value(inter[i, j], ab[i], aq[j], criterion)
    return out


def d3_overlap_truth(geometry, boxes, query_boxes, criterion, z_axis=1, z_center=1.0):
    """d3_box_overlap_kernel in fp64 on the fp64 BEV intersection: boxes (N, 7), query_boxes (K, 7) fp64."""
    inter = geometry[0]
    out = np.zeros_like(inter)
    for i in range(inter.shape[0]):
        for j in range(inter.shape[1]):
            if not inter[i, j] > 0:
                continue
            b, q = boxes[i], query_boxes[j]
            min_z = min(b[z_axis] + b[z_axis + 3] * (1 - z_center), q[z_axis] + q[z_axis + 3] * (1 - z_center))
            max_z = max(b[z_axis] - b[z_axis + 3] * z_center, q[z_axis] - q[z_axis + 3] * z_center)
            iw = min_z - max_z
            if iw > 0:
                area1, area2 = b[3] * b[4] * b[5], q[3] * q[4] * q[5]
                inc = iw * inter[i, j]
                ua = area1 + area2 - inc if criterion == -1 else area1 if criterion == 0 else area2 if criterion == 1 else 1.0
                out[i, j] = inc / ua if ua > 0 else 0.0
    return out


def corner_delta(max_abs_coordinate):
    """8 fp32 ulps of the largest |corner coordinate|: what cosf / sinf, two products, a sum and the offset can move a corner by."""
    return 8.0 * np.spacing(np.asarray(max_abs_coordinate, dtype=np.float64).astype(np.float32)).astype(np.float64)


def pair_bound(geometry, criterion=-1):
    """The derived per-pair bar of an N x K overlap whose corners the device forms in fp32:
        |dIoU| <= 2 * delta * 2 * (perim_a + perim_b) / max(area_a, area_b) + 2^-23
    delta = corner_delta(largest |corner coordinate| of the pair); a corner that moves by delta changes an area by at most delta times
    the perimeter, the intersection by at most that of both, and IoU = I / U with U >= max(area); 2^-23 is the float32 store (and the
    float32 BEV intersection of the 3-D form); the leading 2 is margin.  For the other criteria the same reasoning with the
    criterion's own denominator (query area, box area, 1) in place of max(area), and the store relative to the value."""
    inter, ab, aq, pb, pq, mb, mq = geometry
    delta = corner_delta(np.maximum(mb[:, None], mq[None, :]))
    num = 2.0 * delta * 2.0 * (pb[:, None] + pq[None, :])
    if criterion == -1:
        return num / np.maximum(ab[:, None], aq[None, :]) + 2.0 ** -23
    if criterion == 0:
        return num / np.broadcast_to(aq[None, :], inter.shape) + 2.0 ** -23
    if criterion == 1:
        return num / np.broadcast_to(ab[:, None], inter.shape) + 2.0 ** -23
    return num + 2.0 ** -23 * np.maximum(inter, 1.0)
