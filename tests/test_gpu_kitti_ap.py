"""GPU: the KITTI AP evaluation on the device (pvcnn_amd/kitti.py, csrc/kitti_ap.hip, csrc/boxes.hip).

Against the golden (tests/golden/kitti_ap.pt: the reference's own run): image_box_overlap and the per-image 2-D overlaps bit-equal,
bev / 3d overlaps within PAIR_TOL; the matching kernels FED THE GOLDEN'S OVERLAPS give the reference's clean flags, pass-1
true-positive scores, thresholds, counts and tp / fp / fn exactly and its similarity sums to rtol 1e-10 (n * 2^-53 for a reordered fp64
sum of n <= 1e5 terms in [0, 1], plus a few ulp of cos); end to end from the annotations the curves and the AP table are the reference's.

Fuzz against the sequential truth (tests/kitti_ap_truth.py, proven equal to the golden on the CPU), fed the device's own overlaps so
that IoU rounding cannot matter: per-image sizes around the 64 lanes of a wave, image counts around the reference's 50-image parts
and the 8 images of a wave, true-positive totals around the 41 sample points."""
import os

import numpy as np
import pytest
import torch

import kitti_ap_truth as truth
from conftest import ROOT

pytestmark = pytest.mark.gpu

PAIR_TOL = 1e-5                                       # tests/test_gpu_kitti.py's bound for one fp32 overlap
METRICS = ('bbox', 'bev', '3d')
SIM_RTOL = 1e-10
NAMES = ['Car', 'Pedestrian', 'Cyclist', 'Van', 'Person_sitting', 'Truck', 'DontCare', 'tractor', 'trailer', 'car']
SIZES = {'Car': (3.9, 1.5, 1.6), 'Pedestrian': (0.8, 1.7, 0.6), 'Cyclist': (1.8, 1.7, 0.6)}


@pytest.fixture(scope='module')
def golden():
    return torch.load(os.path.join(ROOT, 'tests', 'golden', 'kitti_ap.pt'), weights_only=False)


@pytest.fixture(scope='module')
def golden_images(golden):
    return truth.images_from_golden(golden['gt'], golden['dt'], golden['names'])


@pytest.fixture(scope='module')
def golden_annos(golden_images):
    return truth.annotations(golden_images)


@pytest.fixture(scope='module')
def kitti():
    from pvcnn_amd import kitti
    return kitti


def run(kitti, gt_annos, dt_annos, classes, difficulties, metric, min_overlaps, compute_aos, overlaps=None):
    packed = kitti._Packed(gt_annos, dt_annos)
    if overlaps is not None:
        overlaps = torch.as_tensor(np.asarray(overlaps)).to(packed.device)
    return kitti._eval_class_packed(packed, classes, difficulties, metric, min_overlaps, compute_aos, 1, 1.0, overlaps=overlaps,
                                    details=True)


# ---- against the golden ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('criterion', [-1, 0, 1, 2])
def test_image_box_overlap_is_bit_equal(kitti, golden, criterion):
    rec = golden['image_box_overlap']
    got = kitti.image_box_overlap(rec['boxes'].numpy(), rec['query_boxes'].numpy(), criterion)
    assert got.dtype == np.float64 and np.array_equal(got, rec['out'][criterion].numpy())
    assert kitti.image_box_overlap(np.zeros((0, 4)), rec['query_boxes'].numpy(), criterion).shape == (0, 20)


def test_per_image_overlaps(kitti, golden, golden_annos):
    from pvcnn_amd.modules.functional import backend as be
    packed = kitti._Packed(*golden_annos)
    got = {key: be._backend.kitti_ap_overlaps(packed, metric).cpu().numpy() for metric, key in enumerate(METRICS)}
    assert got['bbox'].dtype == np.float64 and np.array_equal(got['bbox'], golden['overlaps']['bbox'].numpy())
    for key in ('bev', '3d'):
        want = golden['overlaps'][key].numpy()
        assert got[key].dtype == np.float32 and got[key].shape == want.shape
        err = np.abs(got[key].astype(np.float64) - want.astype(np.float64)).max()
        print(f'{key}: max |overlap - reference| = {err:.3e} over {want.size} pairs ({(want > 0).sum()} positive)')
        assert err <= PAIR_TOL


@pytest.mark.parametrize('key', METRICS)
def test_matching_on_the_goldens_overlaps(kitti, golden, golden_annos, key):
    want = golden['metrics'][key]
    got = run(kitti, *golden_annos, golden['classes'], golden['difficulties'], METRICS.index(key), golden['min_overlaps'].numpy(), True,
              overlaps=golden['overlaps'][key].numpy())
    d = got['details']
    assert np.array_equal(d['ignored_gt'], golden['clean']['ignored_gt'].numpy())
    assert np.array_equal(d['ignored_det'], golden['clean']['ignored_det'].numpy())
    assert np.array_equal(d['num_valid_gt'], golden['clean']['num_valid_gt'].numpy())
    # pass 1: the true-positive scores of every cell as a multiset
    counts, scores, at = want['tp_counts'].numpy().astype(np.int64), want['tp_scores'].numpy(), 0
    for cell in np.ndindex(3, 3, 1):
        n = int(counts[cell].sum())
        mine = d['tp_scores'][cell]
        assert np.array_equal(np.sort(mine[np.isfinite(mine)]), np.sort(scores[at:at + n])), cell
        at += n
    assert np.array_equal(d['counts'], want['counts'].numpy())
    assert np.array_equal(got['thresholds'], want['eval']['thresholds'].numpy())
    assert np.array_equal(d['pr'][..., :3], want['pr'][..., :3].numpy())
    np.testing.assert_allclose(d['pr'][..., 3], want['pr'][..., 3].numpy(), rtol=SIM_RTOL, atol=0)


@pytest.mark.parametrize('with_alpha', [True, False])
def test_end_to_end_equals_the_reference(kitti, golden, golden_annos, with_alpha):
    gt_annos, dt_annos = golden_annos
    if not with_alpha:
        dt_annos = [dict(a, alpha=np.full_like(a['alpha'], -10.0)) for a in dt_annos]
    metrics, results, results_str = kitti.get_official_eval_result(gt_annos, dt_annos, golden['classes'])
    for key in METRICS:
        want = golden['metrics'][key]['eval']
        assert np.array_equal(metrics[key]['precision'], want['precision'].numpy(), equal_nan=True)
        assert np.array_equal(metrics[key]['thresholds'], want['thresholds'].numpy())
        if with_alpha:
            np.testing.assert_allclose(metrics[key]['orientation'], want['orientation'].numpy(), rtol=SIM_RTOL, atol=0)
        else:
            assert not metrics[key]['orientation'].any()
        assert metrics[key]['precision'].shape == (3, 3, 1, 41)
    want_results = golden['results' if with_alpha else 'plain_results']
    want_str = golden['results_str' if with_alpha else 'plain_results_str']
    assert sorted(results) == sorted(want_results)
    for name, per_metric in want_results.items():
        for key in METRICS:
            assert np.array_equal(results[name][key], per_metric[key].numpy(), equal_nan=True)
    got_lines, want_lines = results_str.splitlines(), want_str.splitlines()
    assert len(got_lines) == len(want_lines) and ('aos' in results_str) == with_alpha
    for a, b in zip(got_lines, want_lines):
        if a.startswith('aos'):
            np.testing.assert_allclose([float(v) for v in a[8:].split(', ')], [float(v) for v in b[8:].split(', ')], atol=0.011)
            assert a[:8] == b[:8]
        else:
            assert a == b
    assert results_str.endswith('\n')


# ---- fuzz against the sequential truth -------------------------------------------------------------------------------------------------
def fuzz_image(rng, num_gt, num_dt, names=NAMES, scores=(0.2, 0.4, 0.4, 0.6, 0.9), spots=4):
    """Ground truths clustered on a few spots and detections that are noisy copies of them (several per ground truth where num_dt >
    num_gt), so that detections contend for ground truths and ground truths for detections."""
    centre = np.stack([rng.uniform(50, 1000, spots), rng.uniform(120, 220, spots)], 1)
    place = np.stack([rng.uniform(-8, 8, spots), rng.uniform(1.2, 1.8, spots), rng.uniform(8, 30, spots)], 1)
    spot = rng.randint(0, spots, num_gt)
    height = rng.choice([22.0, 30.0, 39.0, 42.0, 60.0, 90.0], num_gt) + rng.rand(num_gt)
    width = height * rng.uniform(0.8, 1.2, num_gt)
    c = centre[spot] + rng.randn(num_gt, 2) * 25
    g_bbox = np.stack([c[:, 0] - width / 2, c[:, 1] - height / 2, c[:, 0] + width / 2, c[:, 1] + height / 2], 1).reshape(-1, 4)
    g_loc = (place[spot] + rng.randn(num_gt, 3) * np.array([1.5, 0.1, 1.5])).reshape(-1, 3)
    g_dims = (np.array(SIZES['Car'])[None] * rng.uniform(0.9, 1.1, (num_gt, 3))).reshape(-1, 3)
    g_ry = rng.uniform(-3, 3, num_gt)
    g_name = [str(n) for n in rng.choice(names, num_gt)]
    if num_gt:
        src = rng.randint(0, num_gt, num_dt)
        noise = rng.choice([0.01, 0.05, 0.2], num_dt)
        d_bbox = g_bbox[src] + rng.randn(num_dt, 4) * (noise * height[src])[:, None]
        d_loc = g_loc[src] + rng.randn(num_dt, 3) * noise[:, None] * np.array([1.0, 0.2, 1.0])
        d_dims = g_dims[src] * (1 + rng.randn(num_dt, 3) * noise[:, None] * 0.5)
        d_ry = g_ry[src] + rng.randn(num_dt) * noise
        d_name = [g_name[i] if g_name[i] in names[:3] and rng.rand() < 0.8 else str(rng.choice(names[:3])) for i in src]
    else:
        x0, y0, side = rng.uniform(0, 1000, num_dt), rng.uniform(100, 250, num_dt), rng.uniform(20, 90, num_dt)
        d_bbox = np.stack([x0, y0, x0 + side, y0 + side], 1).reshape(-1, 4)
        d_loc = np.stack([rng.uniform(-8, 8, num_dt), np.full(num_dt, 1.5), rng.uniform(8, 30, num_dt)], 1).reshape(-1, 3)
        d_dims = np.tile(np.array(SIZES['Car']), (num_dt, 1)).reshape(-1, 3)
        d_ry = rng.uniform(-3, 3, num_dt)
        d_name = [str(n) for n in rng.choice(names[:3], num_dt)]
    return {'gt_name': g_name, 'dt_name': d_name, 'gt_bbox': g_bbox, 'dt_bbox': d_bbox,
            'gt_occluded': rng.choice([0, 0, 0, 1, 2, 3], num_gt), 'gt_truncated': rng.choice([0.0, 0.0, 0.0, 0.2, 0.4, 0.6], num_gt),
            'gt_alpha': rng.uniform(-3, 3, num_gt), 'dt_alpha': rng.uniform(-3, 3, num_dt),
            'dt_score': rng.choice(scores, num_dt).astype(np.float64), 'gt_dimensions': g_dims, 'gt_location': g_loc, 'gt_rotation_y': g_ry,
            'dt_dimensions': d_dims, 'dt_location': d_loc, 'dt_rotation_y': d_ry}


def exact_image(rng, n, detected=True, name='Car'):
    """n easy, well separated ground truths and, if `detected`, their exact detections: n true positives."""
    im = fuzz_image(rng, n, n, names=[name], spots=1)
    im['gt_bbox'] = np.array([[100.0 + 100 * i, 100.0, 180.0 + 100 * i, 180.0] for i in range(n)]).reshape(-1, 4)
    im['gt_location'] = np.array([[-20.0 + 6 * i, 1.5, 20.0] for i in range(n)]).reshape(-1, 3)
    im['gt_occluded'], im['gt_truncated'] = np.zeros(n, dtype=np.int64), np.zeros(n)
    im['dt_name'] = [name if detected else 'Cyclist'] * n
    for k in ('bbox', 'dimensions', 'location', 'rotation_y'):
        im['dt_' + k] = np.array(im['gt_' + k], dtype=np.float64)
    im['dt_score'] = rng.choice([0.3, 0.5, 0.8], n).astype(np.float64)
    return im


def check_against_truth(kitti, images, classes, difficulties, metric, min_overlaps, compute_aos, class_ints=None):
    gt_annos, dt_annos = truth.annotations(images)
    got = run(kitti, gt_annos, dt_annos, classes, difficulties, metric, min_overlaps, compute_aos)
    d = got['details']
    want = truth.evaluate(images, truth.split_overlaps(d['overlaps'], images), class_ints or classes, difficulties, metric, min_overlaps,
                          compute_aos)
    M, L, K = len(classes), len(difficulties), len(min_overlaps)
    for m in range(M):
        for l in range(L):
            assert d['ignored_gt'][m, l].tolist() == want['ignored_gt'][m][l]
            assert d['ignored_det'][m, l].tolist() == want['ignored_det'][m][l]
            for k in range(K):
                mine = d['tp_scores'][m, l, k]
                theirs = [s for per_image in want['tp_scores'][m][l][k] for s in per_image]
                assert np.array_equal(np.sort(mine[np.isfinite(mine)]), np.sort(np.array(theirs, dtype=np.float64)))
    assert np.array_equal(d['num_valid_gt'], want['num_valid_gt'])
    assert np.array_equal(d['counts'], want['counts'])
    assert np.array_equal(got['thresholds'], want['thresholds'])
    assert np.array_equal(d['pr'][..., :3], want['pr'][..., :3])
    np.testing.assert_allclose(d['pr'][..., 3], want['pr'][..., 3], rtol=SIM_RTOL, atol=0)
    assert np.array_equal(got['precision'], want['precision'], equal_nan=True)
    np.testing.assert_allclose(got['orientation'], want['orientation'], rtol=SIM_RTOL, atol=0)
    assert got['precision'].shape == (M, L, K, 41)
    return got, want


TWO_ROWS = np.array([[[0.7, 0.5, 0.5]] * 3, [[0.5, 0.25, 0.25]] * 3])
CROWD = ['Car', 'Car', 'Pedestrian', 'Van', 'Person_sitting', 'DontCare']
SHAPES = [(0, 0), (0, 3), (3, 0), (1, 1), (7, 63), (7, 64), (7, 65), (70, 130), (5, 257)]


@pytest.mark.parametrize('metric', [0, 1, 2])
def test_fuzz_sizes_around_the_wave(kitti, metric):
    """Every per-image (gt, dt) size in one evaluation: empty sides, one pair, 63 / 64 / 65 detections (one and two rounds of the
    lanes), more ground truths than lanes, five rounds; two min_overlap rows; AOS."""
    rng = np.random.RandomState(100 + metric)
    images = [fuzz_image(rng, g, d, names=CROWD) for g, d in SHAPES]
    got, want = check_against_truth(kitti, images, [0, 1], [0, 2], metric, TWO_ROWS[:, :, :2], True)
    print('tp / fp / fn maxima', want['pr'][..., :3].max(axis=(0, 1, 2, 3)), 'thresholds per cell', want['counts'].tolist())
    assert want['counts'].max() > 0


@pytest.mark.parametrize('count', [1, 2, 49, 50, 51, 130])
def test_fuzz_image_counts(kitti, count):
    """Ragged offsets over any number of images, below the reference's 50 included; 520 true positives at 130 images: the
    threshold scan skips scores."""
    rng = np.random.RandomState(count)
    images = [exact_image(rng, 8) if count == 130 and i % 2 == 0 else fuzz_image(rng, rng.randint(0, 7), rng.randint(0, 9), spots=2)
              for i in range(count)]
    got, want = check_against_truth(kitti, images, [0], [0, 2], 0, TWO_ROWS[:, :, :1], True)
    if count == 130:
        assert want['pr'][0, 0, 0, 0, 0] + want['pr'][0, 0, 0, 0, 2] >= 520 and want['counts'].max() == 41


@pytest.mark.parametrize('total', [0, 1, 40, 41])
def test_fuzz_true_positive_totals(kitti, total):
    """0, 1, 40 and 41 true positives in a cell: no threshold, one, and the edge of the 41 sample points.  Among 52 ground truths the
    recall steps of 1/52 are finer than the samples' 1/40, so the scan skips scores (fewer thresholds than true positives, the last one
    admitting them all); with every ground truth detected, `total` of `total`, each score is a sample point up to the 41st."""
    rng = np.random.RandomState(7 + total)
    for count in {52, max(total, 2)}:
        images = [exact_image(rng, 1, i < total) for i in range(count)]
        got, want = check_against_truth(kitti, images, [0], [0, 1], 1, TWO_ROWS[:, :, :1], False)
        n = int(want['counts'][0, 0, 0])
        assert np.isfinite(got['details']['tp_scores'][0, 0, 0]).sum() == total and want['num_valid_gt'][0, 0] == count
        assert n == min(total, 41) if count == total or total < 2 else 1 < n < total
        assert n == 0 or (want['pr'][0, 0, 0, n - 1, 0] == total and want['pr'][0, 0, 0, n - 1, 2] == count - total)
        assert not got['orientation'].any()


def test_fuzz_equal_scores_and_a_threshold_above_every_score(kitti):
    """All scores equal: every choice is a tie, the lowest index wins.  Then every detection below the score threshold of pass 2:
    the thresholds of a run with high scores applied to the same boxes with low scores (through the kernels directly)."""
    from pvcnn_amd.modules.functional import backend as be
    rng = np.random.RandomState(11)
    images = [fuzz_image(rng, g, d, names=CROWD, scores=(0.5,)) for g, d in [(7, 65), (5, 20), (0, 2), (9, 9)]]
    check_against_truth(kitti, images, [0, 1], [0, 1, 2], 0, TWO_ROWS[:, :, :2], True)
    check_against_truth(kitti, images, [0, 1], [0, 1, 2], 2, TWO_ROWS[:, :, :2], True)
    gt_annos, dt_annos = truth.annotations(images)
    high = run(kitti, gt_annos, dt_annos, [0], [2], 0, TWO_ROWS[:1, :, :1], True)
    assert high['details']['counts'][0, 0, 0] > 0
    low_images = [dict(im, dt_score=np.full(len(im['dt_name']), 0.25)) for im in images]
    packed = kitti._Packed(*truth.annotations(low_images))
    b, dev = be._backend, packed.device
    overlaps = b.kitti_ap_overlaps(packed, 0)
    clean = b.kitti_ap_clean(packed, torch.tensor([0], dtype=torch.int32, device=dev), torch.tensor([2], dtype=torch.int32, device=dev))
    rows = torch.tensor([[0.7]], dtype=torch.float64, device=dev)
    pr = b.kitti_ap_stats(packed, overlaps, clean, rows, torch.from_numpy(high['thresholds']).to(dev),
                          torch.from_numpy(high['details']['counts']).to(dev), 0, True).cpu().numpy()
    n = int(high['details']['counts'][0, 0, 0])
    valid = int(clean[3].item())
    assert (pr[0, 0, 0, :n, 0] == 0).all() and (pr[0, 0, 0, :n, 1] == 0).all() and (pr[0, 0, 0, :n, 2] == valid).all()
    assert not pr[0, 0, 0, n:].any() and not pr[..., 3].any()


def test_fuzz_class_forms(kitti):
    """Classes as names and as ints 0..7 (5 is 'car' again; 3 / 4 have no neighbour rule); a class absent from all ground truths."""
    rng = np.random.RandomState(13)
    images = [fuzz_image(rng, rng.randint(0, 12), rng.randint(0, 14), spots=2) for _ in range(20)]
    for im in images:
        im['dt_name'] = [g if rng.rand() < 0.7 else str(rng.choice(NAMES)) for g in rng.choice(im['gt_name'] or NAMES, len(im['dt_name']))]
        im['gt_name'] = [n if n != 'Cyclist' else 'Car' for n in im['gt_name']]          # no Cyclist ground truth anywhere
    mo = np.array([[[0.5] * 8] * 3])
    by_int, want = check_against_truth(kitti, images, list(range(8)), [0, 1, 2], 0, mo, True)
    assert want['num_valid_gt'][2].sum() == 0 and want['counts'][2].sum() == 0 and not by_int['precision'][2].any()
    assert np.array_equal(by_int['precision'][0], by_int['precision'][5], equal_nan=True)
    print('num_valid_gt', want['num_valid_gt'].tolist(), 'thresholds', want['counts'][..., 0].tolist())
    assert want['num_valid_gt'][[0, 1, 3, 4, 6, 7]].sum(1).min() > 0
    names = ['Car', 'Pedestrian', 'Cyclist', 'Van', 'Person_sitting', 'car', 'tractor', 'trailer']
    by_name, _ = check_against_truth(kitti, images, names, [0, 1, 2], 0, mo, True, class_ints=list(range(8)))
    for key in ('precision', 'orientation', 'thresholds'):
        assert np.array_equal(by_int[key], by_name[key], equal_nan=True)


def test_over_limit_images_raise(kitti):
    rng = np.random.RandomState(17)
    mo = TWO_ROWS[:1, :, :1]
    for g, d in ((1, kitti.MAX_BOXES_PER_IMAGE + 1), (kitti.MAX_BOXES_PER_IMAGE + 1, 1)):
        annos = truth.annotations([fuzz_image(rng, 2, 2), fuzz_image(rng, g, d)])
        with pytest.raises(RuntimeError, match='more than 2048'):
            kitti.eval_class(*annos, [0], [0], 0, mo)
    annos = truth.annotations([fuzz_image(rng, 3, kitti.MAX_BOXES_PER_IMAGE)])                 # the limit itself is served
    assert kitti.eval_class(*annos, [0], [0], 0, mo)['precision'].shape == (1, 1, 1, 41)
    with pytest.raises(ValueError):
        kitti.eval_class([], [], [0], [0], 0, mo)


def test_two_runs_are_bit_identical(kitti):
    rng = np.random.RandomState(19)
    images = [fuzz_image(rng, rng.randint(0, 20), rng.randint(0, 80), names=CROWD) for _ in range(40)]
    annos = truth.annotations(images)
    for metric in (0, 2):
        a = run(kitti, *annos, [0, 1, 2], [0, 1, 2], metric, TWO_ROWS, True)
        b = run(kitti, *annos, [0, 1, 2], [0, 1, 2], metric, TWO_ROWS, True)
        for key in ('precision', 'orientation', 'thresholds'):
            assert a[key].tobytes() == b[key].tobytes()
        assert a['details']['pr'].tobytes() == b['details']['pr'].tobytes() and a['details']['pr'][..., 3].max() > 0
