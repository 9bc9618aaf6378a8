"""A plain sequential truth for the KITTI AP evaluation: clean / matching pass 1 / thresholds / matching pass 2 / precision / mAP.

Written from the algorithm, one Python loop per rule, for ONE image at a time; it takes the overlaps as input (overlaps[det, gt]), so
no IoU rounding can separate it from what it checks.  tests/test_kitti_ap_truth_host.py proves it equal to the reference's recorded
run (tests/golden/kitti_ap.pt); tests/test_gpu_kitti_ap.py fuzzes the device kernels against it.

An image is a dict: gt_name, dt_name (lists of str), gt_bbox (G, 4), dt_bbox (D, 4), gt_occluded, gt_truncated, gt_alpha (G), dt_alpha,
dt_score (D).
"""
import math

import numpy as np

CLASS_NAMES = ['car', 'pedestrian', 'cyclist', 'van', 'person_sitting', 'car', 'tractor', 'trailer']
MIN_HEIGHT = [40, 25, 25]
MAX_OCCLUSION = [0, 1, 2]
MAX_TRUNCATION = [0.15, 0.3, 0.5]
SAMPLE_POINTS = 41
NO_SCORE = -10000000          # a detection scoring at or below this is never matched in pass 1


def clean(image, current_class, difficulty):
    """-> (ignored_gt, ignored_det in {-1, 0, 1}, the positions of the DontCare ground truths, the number of valid ground truths)."""
    wanted = CLASS_NAMES[current_class]
    neighbour = {'pedestrian': 'person_sitting', 'car': 'van'}.get(wanted)
    ignored_gt, dontcare = [], []
    for i, name in enumerate(image['gt_name']):
        lower = str(name).lower()
        height = image['gt_bbox'][i][3] - image['gt_bbox'][i][1]
        too_hard = (image['gt_occluded'][i] > MAX_OCCLUSION[difficulty] or image['gt_truncated'][i] > MAX_TRUNCATION[difficulty]
                    or height <= MIN_HEIGHT[difficulty])
        if lower == wanted:
            ignored_gt.append(1 if too_hard else 0)
        elif neighbour is not None and lower == neighbour:
            ignored_gt.append(1)
        else:
            ignored_gt.append(-1)
        if str(name) == 'DontCare':
            dontcare.append(i)
    ignored_det = []
    for j, name in enumerate(image['dt_name']):
        height = abs(image['dt_bbox'][j][3] - image['dt_bbox'][j][1])
        if height < MIN_HEIGHT[difficulty]:
            ignored_det.append(1)
        else:
            ignored_det.append(0 if str(name).lower() == wanted else -1)
    return ignored_gt, ignored_det, dontcare, sum(1 for f in ignored_gt if f == 0)


def match_scores(overlaps, ignored_gt, ignored_det, scores, min_overlap):
    """Pass 1: the scores of the true positives, in ground-truth order."""
    taken = [False] * len(ignored_det)
    out = []
    for g, flag_gt in enumerate(ignored_gt):
        if flag_gt == -1:
            continue
        chosen, best = None, NO_SCORE
        for j, flag_det in enumerate(ignored_det):
            if flag_det == -1 or taken[j] or not overlaps[j][g] > min_overlap:
                continue
            if scores[j] > best:
                chosen, best = j, scores[j]
        if chosen is None:
            continue
        taken[chosen] = True
        if flag_gt == 0 and ignored_det[chosen] == 0:
            out.append(float(scores[chosen]))
    return out


def thresholds(tp_scores, num_gt):
    """The scores at which the recall passes 0, 1/40, 2/40, ...: at most 41."""
    ordered = sorted((float(s) for s in tp_scores), reverse=True)
    out, recall_wanted = [], 0.0
    for i, score in enumerate(ordered):
        last = i == len(ordered) - 1
        here = (i + 1) / num_gt
        after = here if last else (i + 2) / num_gt
        if not last and (after - recall_wanted) < (recall_wanted - here):
            continue                                    # the next score lies nearer to the wanted recall
        out.append(score)
        recall_wanted += 1 / (SAMPLE_POINTS - 1.0)
    return out


def box_fraction(box, region):
    """Intersection of two (x1, y1, x2, y2) boxes over the area of `box`."""
    w = min(box[2], region[2]) - max(box[0], region[0])
    h = min(box[3], region[3]) - max(box[1], region[1])
    if not (w > 0 and h > 0):
        return 0.0
    return w * h / ((box[2] - box[0]) * (box[3] - box[1]))


def match_stats(image, overlaps, ignored_gt, ignored_det, dontcare, metric, min_overlap, thresh, compute_aos):
    """Pass 2 at one score threshold: (tp, fp, fn, similarity) with similarity None where nothing was found at all."""
    scores = image['dt_score']
    num_det = len(ignored_det)
    taken = [False] * num_det
    low = [bool(scores[j] < thresh) for j in range(num_det)]
    tp = fn = 0
    deltas = []
    for g, flag_gt in enumerate(ignored_gt):
        if flag_gt == -1:
            continue
        # the reference's scan, state by state: nothing / an ignored detection / a counted detection chosen so far
        chosen, chosen_overlap, chosen_is_ignored = None, 0, False
        for j in range(num_det):
            if ignored_det[j] == -1 or taken[j] or low[j]:
                continue
            overlap = overlaps[j][g]
            if not overlap > min_overlap:
                continue
            if ignored_det[j] == 0 and (overlap > chosen_overlap or chosen_is_ignored):
                chosen, chosen_overlap, chosen_is_ignored = j, overlap, False
            elif ignored_det[j] == 1 and chosen is None:
                chosen, chosen_is_ignored = j, True
        if chosen is None:
            if flag_gt == 0:
                fn += 1
            continue
        taken[chosen] = True
        if flag_gt == 1 or ignored_det[chosen] == 1:
            continue
        tp += 1
        if compute_aos:
            deltas.append(image['gt_alpha'][g] - image['dt_alpha'][chosen])
    fp = 0
    for j in range(num_det):
        if taken[j] or low[j] or ignored_det[j] != 0:
            continue
        in_dontcare = metric == 0 and any(box_fraction(image['dt_bbox'][j], image['gt_bbox'][d]) > min_overlap for d in dontcare)
        if not in_dontcare:
            fp += 1
    similarity = None
    if compute_aos and (tp > 0 or fp > 0):
        similarity = math.fsum((1.0 + math.cos(d)) / 2.0 for d in deltas)
    return tp, fp, fn, similarity


def evaluate(images, overlaps, current_classes, difficulties, metric, min_overlaps, compute_aos=False):
    """eval_class over `images` with the given per-image overlaps (a list of (D_i, G_i) arrays).  min_overlaps (K, 3, M).
    -> dict: ignored_gt / ignored_det [m][l] (flat over the images), num_valid_gt (M, L), tp_scores [m][l][k] (a list per image),
    thresholds (M, L, K, 41), counts (M, L, K), pr (M, L, K, 41, 4), precision, orientation (M, L, K, 41)."""
    M, L, K = len(current_classes), len(difficulties), len(min_overlaps)
    out = {'ignored_gt': [[None] * L for _ in range(M)], 'ignored_det': [[None] * L for _ in range(M)],
           'num_valid_gt': np.zeros((M, L), dtype=np.int64), 'tp_scores': [[[None] * K for _ in range(L)] for _ in range(M)],
           'thresholds': np.zeros((M, L, K, SAMPLE_POINTS)), 'counts': np.zeros((M, L, K), dtype=np.int64),
           'pr': np.zeros((M, L, K, SAMPLE_POINTS, 4)), 'precision': np.zeros((M, L, K, SAMPLE_POINTS)),
           'orientation': np.zeros((M, L, K, SAMPLE_POINTS))}
    for m, cls in enumerate(current_classes):
        for l, diff in enumerate(difficulties):
            cleaned = [clean(image, cls, diff) for image in images]
            out['ignored_gt'][m][l] = [f for c in cleaned for f in c[0]]
            out['ignored_det'][m][l] = [f for c in cleaned for f in c[1]]
            num_gt = sum(c[3] for c in cleaned)
            out['num_valid_gt'][m, l] = num_gt
            for k in range(K):
                min_overlap = min_overlaps[k][metric][m]
                per_image = [match_scores(ov, c[0], c[1], image['dt_score'], min_overlap)
                             for image, ov, c in zip(images, overlaps, cleaned)]
                out['tp_scores'][m][l][k] = per_image
                chosen = thresholds([s for scores in per_image for s in scores], num_gt)
                n = len(chosen)
                out['counts'][m, l, k] = n
                out['thresholds'][m, l, k, :n] = chosen
                pr = out['pr'][m, l, k]
                for t, thresh in enumerate(chosen):
                    for image, ov, c in zip(images, overlaps, cleaned):
                        tp, fp, fn, similarity = match_stats(image, ov, c[0], c[1], c[2], metric, min_overlap, thresh, compute_aos)
                        pr[t, 0] += tp
                        pr[t, 1] += fp
                        pr[t, 2] += fn
                        if similarity is not None:
                            pr[t, 3] += similarity
                out['precision'][m, l, k], out['orientation'][m, l, k] = curves(pr, n, compute_aos)
    return out


def curves(pr, n, compute_aos):
    """precision and orientation over the 41 recall positions: tp / (tp + fp) and similarity / (tp + fp) in the first n, each then
    raised to the maximum of everything behind it."""
    precision, orientation = np.zeros(SAMPLE_POINTS), np.zeros(SAMPLE_POINTS)
    with np.errstate(invalid='ignore', divide='ignore'):
        for i in range(n):
            precision[i] = pr[i, 0] / (pr[i, 0] + pr[i, 1])
            if compute_aos:
                orientation[i] = pr[i, 3] / (pr[i, 0] + pr[i, 1])
        for i in range(n):
            precision[i] = np.max(precision[i:])
            if compute_aos:
                orientation[i] = np.max(orientation[i:])
    return precision, orientation


def mean_ap(curve):
    """11-point AP in percent: every fourth of the 41 positions (last axis)."""
    total = 0
    for i in range(0, curve.shape[-1], 4):
        total = total + curve[..., i]
    return total / 11 * 100


def images_from_golden(packed_gt, packed_dt, names):
    """The per-image dicts from the packed annotations of tests/golden/kitti_ap.pt."""
    images, g0, d0 = [], 0, 0
    for ng, nd in zip(packed_gt['counts'].tolist(), packed_dt['counts'].tolist()):
        gs, ds = slice(g0, g0 + ng), slice(d0, d0 + nd)
        images.append({'gt_name': [names[c] for c in packed_gt['name'][gs].tolist()],
                       'dt_name': [names[c] for c in packed_dt['name'][ds].tolist()],
                       'gt_bbox': packed_gt['bbox'][gs].numpy(), 'dt_bbox': packed_dt['bbox'][ds].numpy(),
                       'gt_occluded': packed_gt['occluded'][gs].numpy().astype(np.int64), 'gt_truncated': packed_gt['truncated'][gs].numpy(),
                       'gt_alpha': packed_gt['alpha'][gs].numpy(), 'dt_alpha': packed_dt['alpha'][ds].numpy(),
                       'dt_score': packed_dt['score'][ds].numpy(),
                       'gt_dimensions': packed_gt['dimensions'][gs].numpy(), 'gt_location': packed_gt['location'][gs].numpy(),
                       'gt_rotation_y': packed_gt['rotation_y'][gs].numpy(), 'dt_dimensions': packed_dt['dimensions'][ds].numpy(),
                       'dt_location': packed_dt['location'][ds].numpy(), 'dt_rotation_y': packed_dt['rotation_y'][ds].numpy()})
        g0, d0 = g0 + ng, d0 + nd
    return images


def annotations(images):
    """(gt_annos, dt_annos) in the evaluation's format from per-image dicts that carry the 3-D fields."""
    gt = [{'name': np.array(im['gt_name'], dtype='<U16'), 'truncated': np.asarray(im['gt_truncated'], dtype=np.float64),
           'occluded': np.asarray(im['gt_occluded']), 'alpha': np.asarray(im['gt_alpha'], dtype=np.float64),
           'bbox': np.asarray(im['gt_bbox'], dtype=np.float64).reshape(-1, 4), 'dimensions': np.asarray(im['gt_dimensions']).reshape(-1, 3),
           'location': np.asarray(im['gt_location']).reshape(-1, 3), 'rotation_y': np.asarray(im['gt_rotation_y']),
           'score': np.zeros(len(im['gt_name']))} for im in images]
    dt = [{'name': np.array(im['dt_name'], dtype='<U16'), 'truncated': np.zeros(len(im['dt_name'])),
           'occluded': np.zeros(len(im['dt_name']), dtype=np.int64), 'alpha': np.asarray(im['dt_alpha'], dtype=np.float64),
           'bbox': np.asarray(im['dt_bbox'], dtype=np.float64).reshape(-1, 4), 'dimensions': np.asarray(im['dt_dimensions']).reshape(-1, 3),
           'location': np.asarray(im['dt_location']).reshape(-1, 3), 'rotation_y': np.asarray(im['dt_rotation_y']),
           'score': np.asarray(im['dt_score'], dtype=np.float64)} for im in images]
    return gt, dt


def split_overlaps(flat, images):
    """The flat per-image blocks -> a list of (D_i, G_i) float64 arrays."""
    out, at = [], 0
    flat = np.asarray(flat, dtype=np.float64)
    for im in images:
        nd, ng = len(im['dt_name']), len(im['gt_name'])
        out.append(flat[at:at + nd * ng].reshape(nd, ng))
        at += nd * ng
    return out
