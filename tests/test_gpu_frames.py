"""KITTI frames on the device (csrc/frames.hip, pvcnn_amd.frames, DeviceFrustumKitti.from_frustums) against tests/frames_truth.py, the
numpy definition: zero tolerance on everything the definition fixes.  Synthetic frames from a seeded generator: a 1242 x 375 image, a
KITTI-like calibration, N = 5003 scan points (78 full point tiles of 64 and a ragged one of 11) and six boxes -- the whole image, two
that overlap, one that holds no point, one 24 px high, one whose 3-D box holds no point; N = 1 and N = 64 with one box; N = 20011,
where the tile prefix of a box takes more than one pass of its workgroup (313 tiles > 256).  Reads nothing outside the repository."""
import functools

import numpy as np
import pytest
import torch

from conftest import SEED
import frames_truth as ft

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SIZE = (1242, 375)
P = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
R0 = np.array([[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459], [0.007402527, 0.004351614, 0.9999631]])
V2C = np.array([[0.007533745, -0.9999714, -0.000616602, -0.004069766], [0.01480249, 0.0007280733, -0.9998902, -0.07631618],
                [0.9998621, 0.00752379, 0.01480755, -0.2717806]])
BOXES = np.array([[0, 0, 1242, 375], [400, 120, 700, 300], [550, 100, 800, 280], [60.5, 40.25, 140.5, 120.75], [300, 150, 500, 174],
                  [800, 150, 1000, 250]], dtype=np.float64)
CLASSES = ['Car', 'Pedestrian', 'Cyclist', 'Car', 'Pedestrian', 'Cyclist']
CLASS_IDS = [0, 1, 2, 0, 1, 2]
NAMES = ('Car', 'Pedestrian', 'Cyclist')


def calibration():
    from pvcnn_amd.frames import Calibration
    return Calibration(P, R0, V2C)


@functools.lru_cache(maxsize=None)
def frame(seed=0, n=5003, m=6):
    """(scan (n, 4) fp32, boxes_2d (m, 4), boxes_3d (m, 7), scores (m,)): see the module docstring."""
    rng = np.random.RandomState(SEED + seed)
    scan = (rng.rand(n, 4) * [65, 50, 3.5, 1] + [-5, -25, -2.5, 0]).astype(np.float32)
    if n <= 64:                                             # the corner sizes: every point in front of the camera, in the image
        scan[:, 0] = np.abs(scan[:, 0]) + 6
        scan[:, 1:3] *= np.float32(0.125)
    boxes = BOXES[:m].copy()
    if m > 3:                                               # box 3 holds no point: what projects into it moves inside the clip distance
        _, uv, seen = ft.project(scan, P, R0, V2C, SIZE)
        scan[ft.in_box(uv, seen, boxes[3]), 0] = 1.5
    rows, uv, seen = ft.project(scan, P, R0, V2C, SIZE)
    boxes_3d = np.zeros((m, 7))
    for i in range(m):                                      # a 3-D box around one of the box's points (box 5: far from every point)
        sel = np.nonzero(ft.in_box(uv, seen, boxes[i]))[0]
        centre = rows[sel[len(sel) // 2], :3].astype(np.float64) if len(sel) and i != 5 else np.array([300.0, 0.0, 300.0])
        boxes_3d[i] = [1.6, 1.7 + 0.1 * i, 4.0, centre[0], centre[1] + 0.8, centre[2], rng.uniform(-np.pi, np.pi)]
    return scan, boxes, boxes_3d, rng.rand(m)


@functools.lru_cache(maxsize=None)
def truth(seed=0, n=5003, m=6, with_3d=True, min_points=5):
    scan, boxes, boxes_3d, _ = frame(seed, n, m)
    return ft.extract(scan, P, R0, V2C, boxes, SIZE, boxes_3d=boxes_3d if with_3d else None, min_points=min_points)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def same(a, b):
    a, b = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------------------------ 1: extraction
@pytest.mark.parametrize('n,m,min_points,with_3d', [(5003, 6, 5, True), (5003, 6, 5, False), (1, 1, 5, True), (1, 1, 5, False),
                                                    (1, 1, 1, False), (64, 1, 5, True), (64, 1, 5, False), (20011, 6, 5, True),
                                                    (20011, 6, 5, False)])
def test_extract_frustums_equals_the_truth(hip, n, m, min_points, with_3d):
    from pvcnn_amd import frames
    scan, boxes, boxes_3d, scores = frame(0, n, m)
    want = truth(0, n, m, with_3d, min_points)
    calib = calibration()
    rows, uv, in_image = frames.project_scan(scan, calib, SIZE)
    assert same(rows, want['all_rows']) and same(uv, want['uv']) and same(in_image, want['in_image'].astype(np.uint8))
    before = frames.copies_made()
    options = dict(boxes_3d=boxes_3d) if with_3d else dict(scores=scores, min_points=min_points)
    got = frames.extract_frustums(torch.from_numpy(scan).to(DEV), calib, boxes, SIZE, classes=CLASSES[:m], **options)
    assert frames.copies_made() == before + 1
    assert same(got.kept, want['kept']) and same(got.offsets, want['offsets'])
    for c in range(4):
        assert same(got.rows[:, c], want['rows'][:, c]), f'column {c}'
    assert got.rows.shape == want['rows'].shape
    if with_3d:
        assert same(got.labels, want['labels'])
        assert len(want['kept']) and same(got.boxes_3d, np.stack([ft.corners(boxes_3d[i]) for i in want['kept']]))
    else:
        assert got.labels is None and same(got.scores, scores[want['kept']])
    assert same(got.frustum_angles, want['frustum_angles']) and got.class_names == [CLASSES[i] for i in want['kept']]
    assert same(got.counts, want['counts'][want['kept'], 0])
    if n == 5003:                                           # the frame is what the docstring says it is
        assert want['counts'][3, 0] == 0 and want['counts'][4, 0] > 5 and want['counts'][5, 0] > 5
        assert want['kept'].tolist() == ([0, 1, 2] if with_3d else [0, 1, 2, 5])
        overlap = ft.in_box(want['uv'], want['in_image'], boxes[1]) & ft.in_box(want['uv'], want['in_image'], boxes[2])
        assert overlap.any() and (not with_3d or (want['counts'][:3, 1] > 0).all() and want['counts'][5, 1] == 0)


# ------------------------------------------------------------------------------------------------------------------ 2: parity batch
def numpy_choices(counts, num_points, seed=1):
    rng = np.random.RandomState(SEED + seed)
    return np.stack([rng.choice(k, num_points, replace=True) if k > 0 else np.zeros(num_points, dtype=np.int64) for k in counts]).astype(np.int32)


def batch_equals(got, want):
    inputs, targets, valid = got
    f, hot, rot, score, ok = want
    return (same(inputs['features'], f) and same(inputs['one_hot_vectors'], hot) and same(targets['rotation_angle'], rot)
            and same(targets['rgb_score'], score) and same(valid, ok))


@pytest.mark.parametrize('n,m', [(5003, 6), (1, 1), (64, 1)])
@pytest.mark.parametrize('rotate', [True, False])
def test_frame_batch_in_parity_mode_equals_the_truth(hip, n, m, rotate):
    from pvcnn_amd import frames
    scan, boxes, _, scores = frame(0, n, m)
    counts = truth(0, n, m, False)['counts'][:, 0]
    num_points = 1024 if n > 64 else 96
    ch = numpy_choices(counts, num_points)
    calib = calibration()
    before = frames.copies_made()
    want = ft.batch(scan, P, R0, V2C, boxes, SIZE, CLASS_IDS[:m], scores, ch, num_points, frustum_rotate=rotate)
    got = frames.frame_batch(scan, calib, boxes, SIZE, CLASS_IDS[:m], scores=scores, num_points=num_points, frustum_rotate=rotate, choices=ch)
    assert batch_equals(got, want)
    if n == 5003:
        assert want[4].tolist() == [1, 1, 1, 0, 0, 1]
    # out= of Bmax = 8 rows, poisoned; the scan in a larger buffer, read through count=
    want8 = ft.batch(scan, P, R0, V2C, boxes, SIZE, CLASS_IDS[:m], scores, ch, num_points, frustum_rotate=rotate, bmax=8)
    out = ({'features': torch.full((8, 4, num_points), 7.0, device=DEV), 'one_hot_vectors': torch.full((8, 3), 7.0, device=DEV)},
           {'rotation_angle': torch.full((8,), 7.0, device=DEV), 'rgb_score': torch.full((8,), 7.0, dtype=torch.float64, device=DEV)},
           torch.full((8,), 7, dtype=torch.uint8, device=DEV))
    buffer = torch.full((n + 333, 4), 9.0, device=DEV)      # rows beyond count would all project into the image
    buffer[:n] = torch.from_numpy(scan)
    got8 = frames.frame_batch(buffer, calib, boxes, SIZE, CLASS_IDS[:m], scores=scores, num_points=num_points, frustum_rotate=rotate,
                              choices=ch, out=out, count=torch.tensor([n], dtype=torch.int32, device=DEV))
    assert got8[2] is out[2] and batch_equals(got8, want8)
    dead = (got8[2] == 0).cpu()
    assert dead.sum() >= 8 - m and not got8[0]['features'].cpu()[dead].any() and not got8[0]['one_hot_vectors'].cpu()[dead].any()
    assert not got8[1]['rotation_angle'].cpu()[dead].any() and not got8[1]['rgb_score'].cpu()[dead].any()
    assert frames.copies_made() == before


# ------------------------------------------------------------------------------------------------------------------ 3: device draws
def seed_words(a, b):
    return torch.tensor([a, b], dtype=torch.int64, device=DEV)


def row_set(rows):
    return set(np.ascontiguousarray(rows).view(np.int32).reshape(len(rows), 4).view([('', np.int32)] * 4).reshape(-1).tolist())


def test_frame_batch_in_device_mode(hip):
    from pvcnn_amd import frames
    scan, boxes, _, scores = frame(0)
    calib = calibration()
    kw = dict(scores=scores, num_points=1024, frustum_rotate=True)
    a = frames.frame_batch(scan, calib, boxes, SIZE, CLASS_IDS, seed=seed_words(11, 5), **kw)
    b = frames.frame_batch(scan, calib, boxes, SIZE, CLASS_IDS, seed=seed_words(11, 5), **kw)
    c = frames.frame_batch(scan, calib, boxes, SIZE, CLASS_IDS, seed=seed_words(12, 5), **kw)
    d = frames.frame_batch(scan, calib, boxes, SIZE, CLASS_IDS, seed=seed_words(11, 6), **kw)
    fa = a[0]['features'].cpu().numpy()
    assert same(fa, b[0]['features']) and not same(fa, c[0]['features']) and not same(fa, d[0]['features'])
    assert a[2].tolist() == [1, 1, 1, 0, 0, 1]
    want = truth(0, 5003, 6, False)
    for w, m in enumerate(want['kept']):
        cloud = want['rows'][want['offsets'][w]:want['offsets'][w + 1]]
        allowed = row_set(ft.rotate_rows(cloud, np.pi / 2.0 + ft.frustum_angle(P, boxes[m])))
        drawn = row_set(fa[m].T)
        assert drawn <= allowed and len(drawn) > min(len(allowed), 1024) // 4       # rows of this box, and not a handful of them
    e = frames.frame_batch(scan, calib, boxes, SIZE, CLASS_IDS, scores=scores, num_points=64)      # torch's device generator
    assert e[2].tolist() == [1, 1, 1, 0, 0, 1]


def test_frame_batch_replays_in_a_graph(hip):
    from pvcnn_amd import frames
    scan, boxes, _, scores = frame(0)
    scan2 = frame(1, 4507)[0]
    calib = calibration()
    table = torch.from_numpy(frames.box_table(calib, boxes, CLASS_IDS, scores)).to(DEV)
    buffer = torch.zeros((5200, 4), device=DEV)
    count = torch.zeros((1,), dtype=torch.int32, device=DEV)
    seed = seed_words(21, 4)
    kw = dict(num_points=512, frustum_rotate=True, seed=seed)

    def load(s):
        buffer[:len(s)] = torch.from_numpy(s).to(DEV)
        count.fill_(len(s))
    load(scan)
    out = frames.frame_batch(buffer, calib, table, SIZE, count=count, **kw)             # eager once: everything cached is cached
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        frames.frame_batch(buffer, calib, table, SIZE, count=count, out=out, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        frames.frame_batch(buffer, calib, table, SIZE, count=count, out=out, **kw)
    load(scan2)
    graph.replay()
    torch.cuda.synchronize()
    eager = frames.frame_batch(scan2, calib, boxes, SIZE, CLASS_IDS, scores=scores, **kw)
    assert same(out[0]['features'], eager[0]['features']) and same(out[0]['one_hot_vectors'], eager[0]['one_hot_vectors'])
    assert same(out[1]['rotation_angle'], eager[1]['rotation_angle']) and same(out[1]['rgb_score'], eager[1]['rgb_score'])
    assert same(out[2], eager[2]) and out[2].sum().item() >= 3
    first = frames.frame_batch(scan, calib, boxes, SIZE, CLASS_IDS, scores=scores, **kw)
    assert not same(first[0]['features'], eager[0]['features'])


# ------------------------------------------------------------------------------------------------------------------ 4: the store
TEMPLATES = {'Car': np.array([3.9, 1.6, 1.56]), 'Pedestrian': np.array([0.8, 0.6, 1.73]), 'Cyclist': np.array([1.76, 0.6, 1.73])}
TEMPLATE_IDS = {'Car': 0, 'Pedestrian': 3, 'Cyclist': 5}


def one_ulp(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


@pytest.mark.parametrize('with_3d', [True, False])
def test_a_store_from_frustums_equals_the_constructor_on_the_downloaded_frustums(hip, with_3d):
    from pvcnn_amd import frames
    from pvcnn_amd.data import DeviceFrustumKitti
    calib = calibration()
    got = []
    for s in range(3):
        scan, boxes, boxes_3d, scores = frame(s)
        options = dict(boxes_3d=boxes_3d) if with_3d else dict(scores=scores)
        got.append(frames.extract_frustums(scan, calib, boxes, SIZE, classes=CLASSES, **options))
    clouds = [f.item(w)[0].cpu().numpy() for f in got for w in range(len(f))]
    names = [n for f in got for n in f.class_names]
    angles = [a for f in got for a in f.frustum_angles]
    assert len(clouds) == (9 if with_3d else 12)
    for rotate in (False, True):
        common = dict(classes=NAMES, frustum_rotate=rotate)
        if with_3d:
            truth_options = dict(num_heading_angle_bins=12, class_name_to_size_template_id=TEMPLATE_IDS, size_templates=TEMPLATES,
                                 random_flip=True, random_shift=True)
            want = DeviceFrustumKitti(clouds, [f.item(w)[1].cpu().numpy() for f in got for w in range(len(f))],
                                      [c for f in got for c in f.boxes_3d], [h for f in got for h in f.heading_angles],
                                      [z for f in got for z in f.sizes], names, angles, 1024, device=DEV, **truth_options, **common)
            store = DeviceFrustumKitti.from_frustums(got, 1024, **truth_options, **common)
            assert same(store.labels, want.labels) and same(store.item_i64, want.item_i64)
        else:
            want = DeviceFrustumKitti.from_rgb_detection(clouds, names, angles, [p for f in got for p in f.scores], 1024, device=DEV, **common)
            store = DeviceFrustumKitti.from_frustums(got, 1024, **common)
            assert store.labels is None and store.item_i64 is None and store.rgb_detection
        assert same(store.offsets, want.offsets) and same(store.item_f64, want.item_f64) and same(store.item_f32, want.item_f32)
        assert store.max_n == want.max_n and len(store) == len(want) and store.nbytes == want.nbytes
        if not rotate:
            assert same(store.rows, want.rows)
        else:
            exact = np.concatenate([ft.rotate_rows(c, np.pi / 2.0 + a) for c, a in zip(clouds, angles)])
            assert same(store.rows, exact)
            assert one_ulp(store.rows.cpu().numpy(), want.rows.cpu().numpy()).all()
        idx = list(range(len(store)))[::-1][:8]
        counts = (store.offsets[1:] - store.offsets[:-1]).cpu().numpy()
        ch = torch.from_numpy(numpy_choices([counts[i] for i in idx], 1024, seed=2))
        rng = np.random.RandomState(SEED)
        draws = dict(flip=torch.from_numpy(rng.random_sample(8)), shift=torch.from_numpy(rng.randn(8))) if with_3d else {}
        a, b = store.assemble(idx, choices=ch, **draws), store.to('cpu').assemble_reference(idx, choices=ch, **draws)
        for x, y in zip(a, b):
            assert x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)


# ------------------------------------------------------------------------------------------------------------------ 5: detection
def test_detect_frame_equals_the_steps_by_hand_and_its_lines_parse_back(hip, tmp_path):
    from pvcnn_amd import frames, kitti, workload
    scan, boxes, _, scores = frame(0)
    calib = calibration()
    templates = workload.frustum_size_templates()
    torch.manual_seed(SEED)
    model = workload.FrustumPVCNNE(3, 12, 8, 128, templates, 1, 0.25).to(DEV).eval()
    ch = numpy_choices(truth(0, 5003, 6, False)['counts'][:, 0], 1024, seed=3)
    before = frames.copies_made()
    torch.manual_seed(7)
    table, valid = frames.detect_frame(model, scan, calib, boxes, SIZE, CLASS_IDS, scores, templates.to(DEV), choices=ch)
    assert frames.copies_made() == before + 1
    torch.manual_seed(7)
    inputs, targets, ok = frames.frame_batch(scan, calib, boxes, SIZE, CLASS_IDS, scores=scores, choices=ch)
    with torch.no_grad():
        outputs = model(inputs)
    want = torch.zeros((6, 8), dtype=torch.float64, device=DEV)
    kitti.frustum_box_predictions(want, outputs, targets, 0, templates.to(DEV), kitti.heading_angle_bin_centers(12, DEV))
    assert table.shape == (6, 8) and table.dtype == np.float64 and same(table, want)
    assert valid.tolist() == [True, True, True, False, False, True] and same(valid, ok.cpu().numpy() != 0)
    assert np.isfinite(table[valid]).all() and same(table[:, 7], np.where(valid, scores, 0.0))
    lines = frames.kitti_label_lines(CLASSES, boxes, table, valid)
    assert len(lines) == 4 and all(line.endswith('\n') for line in lines)
    path = tmp_path / '000000.txt'
    path.write_text(''.join(lines))
    anno = kitti.get_label_annotation(str(path))
    live = np.nonzero(valid)[0]
    assert anno['name'].tolist() == [CLASSES[i] for i in live] and np.array_equal(anno['bbox'], boxes[live])
    shown = np.array([[float(f'{v:f}') for v in table[i]] for i in live])
    assert np.array_equal(anno['dimensions'], shown[:, [2, 0, 1]]) and np.array_equal(anno['location'], shown[:, 3:6])
    assert np.array_equal(anno['rotation_y'], shown[:, 6]) and np.array_equal(anno['score'], shown[:, 7])
