"""The KITTI frame store (csrc/frame_store.hip, pvcnn_amd.frame_store.DeviceKittiFrames) against tests/frame_store_truth.py, the numpy
definition: zero tolerance in parity mode.  Synthetic frames as tests/test_gpu_frames.py makes them (the same image, calibration and
point distribution), cut so that their in-image point counts are 1, 63, 64, 65 (the edges of a 64-point tile) and 5003 (79 tiles: five
trips of the sixteen waves' walk), with 1, 2, 3, 4 and 6 objects; one device-mode test adds a frame of 66003 points (1032 tiles: a
second trip of the 1024-thread prefix scan, whose carry it needs).  The last of the five frames holds the three hand-made cases of the
acceptance rule: an object whose box is 26 px high (u2 = 0 makes it 23.4), and one whose only positive point lies 2 px inside the left
edge of its box (u0 ~ 1 moves the box 8 px to the right).  Reads nothing outside the repository."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import SEED
import frames_truth as ft
import frame_store_truth as fst

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SIZE = (1242, 375)
P = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
R0 = np.array([[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459], [0.007402527, 0.004351614, 0.9999631]])
V2C = np.array([[0.007533745, -0.9999714, -0.000616602, -0.004069766], [0.01480249, 0.0007280733, -0.9998902, -0.07631618],
                [0.9998621, 0.00752379, 0.01480755, -0.2717806]])
NAMES = ('Car', 'Pedestrian', 'Cyclist')
TEMPLATES = {'Car': np.array([3.9, 1.6, 1.56]), 'Pedestrian': np.array([0.8, 0.6, 1.73]), 'Cyclist': np.array([1.76, 0.6, 1.73])}
TEMPLATE_IDS = {'Car': 0, 'Pedestrian': 3, 'Cyclist': 5}
FRAMES = ((1, 1), (63, 2), (64, 3), (65, 4), (5003, 6))       # (in-image points, objects)
LOW, EDGE = 2, 3                                              # the hand-made objects of the last frame
KEYS = ('mask_logits', 'center', 'heading_bin_id', 'heading_residual', 'size_template_id', 'size_residual', 'class_id')


def calibration():
    from pvcnn_amd.frames import Calibration
    return Calibration(P, R0, V2C)


@functools.lru_cache(maxsize=None)
def frame(index, n_in=None, m=None):
    """(scan (n, 4) fp32 with exactly n_in in-image points among others, boxes_2d (m, 4), boxes_3d (m, 7), class names)."""
    if n_in is None:
        n_in, m = FRAMES[index]
    rng = np.random.RandomState(SEED + 100 + index)
    cloud = (rng.rand(4 * n_in + 64, 4) * [65, 50, 3.5, 1] + [-5, -25, -2.5, 0]).astype(np.float32)
    seen = ft.project(cloud, P, R0, V2C, SIZE)[2]
    inside, outside = np.nonzero(seen)[0][:n_in], np.nonzero(~seen)[0][:n_in // 3 + 1]
    assert len(inside) == n_in
    scan = cloud[np.sort(np.concatenate([inside, outside]))]
    rows, uv = fst.frame_points(scan, P, R0, V2C, SIZE)
    assert len(rows) == n_in
    boxes, boxes_3d = np.zeros((m, 4)), np.zeros((m, 7))
    for i in range(m):                                       # an object around one of the frame's points
        j = (i * n_in) // m
        u, v = uv[j]
        x, y, z = rows[j, :3].astype(np.float64)
        boxes[i] = [u - 40 - i, v - 30, u + 40, v + 30 + i]
        boxes_3d[i] = [1.6, 1.7 + 0.1 * i, 4.0, x, y + 0.8, z, rng.uniform(-np.pi, np.pi)]
        if index == len(FRAMES) - 1 and i == LOW:
            boxes[i] = [u - 40, v - 13, u + 40, v + 13]
        if index == len(FRAMES) - 1 and i == EDGE:           # a 3-D box so small that it holds this point alone
            boxes[i] = [u - 2, v - 30, u + 78, v + 30]
            boxes_3d[i] = [0.02, 0.02, 0.02, x, y + 0.01, z, 0.3]
    return scan, boxes, boxes_3d, [NAMES[(i + index) % 3] for i in range(m)]


@functools.lru_cache(maxsize=None)
def world():
    """The truth's view of the five frames: their stored points, and one item dict per object, in store order."""
    points, items = [], []
    for f in range(len(FRAMES)):
        scan, boxes, boxes_3d, names = frame(f)
        points.append(fst.frame_points(scan, P, R0, V2C, SIZE))
        for i in range(len(boxes)):
            assert fst.admitted(points[f], boxes[i], boxes_3d[i])
            hot = np.zeros(3, dtype=np.float32)
            hot[NAMES.index(names[i])] = 1
            items.append(dict(frame=f, box=boxes[i], box_3d=boxes_3d[i], one_hot=hot, class_id=NAMES.index(names[i]),
                              size_template_id=TEMPLATE_IDS[names[i]],
                              size_residual=(boxes_3d[i][[2, 1, 0]] - TEMPLATES[names[i]]).astype(np.float32)))
    return points, items


@functools.lru_cache(maxsize=None)
def make_store(num_points, rotate, flip_shift, shift_ratio=0.1, frames=tuple(range(len(FRAMES)))):
    from pvcnn_amd.frame_store import DeviceKittiFrames
    calib = calibration()
    return DeviceKittiFrames([(frame(f)[0], calib, SIZE) + frame(f)[1:] for f in frames], num_points,
                             class_name_to_size_template_id=TEMPLATE_IDS, size_templates=TEMPLATES, random_flip=flip_shift,
                             random_shift=flip_shift, frustum_rotate=rotate, shift_ratio=shift_ratio)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def same(a, b):
    a, b = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def seed_words(a, b):
    return torch.tensor([a, b], dtype=torch.int64, device=DEV)


PAD = 3


def poisoned(shape, dtype):
    """A contiguous tensor of `shape` that starts PAD elements inside a larger allocation full of NaN / -1 -> (the slice, the allocation)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * PAD,), float('nan') if dtype.is_floating_point else -1, dtype=dtype, device=DEV)
    return whole[PAD:PAD + n].view(shape), whole


def intact(whole):
    edge = torch.cat([whole[:PAD], whole[-PAD:]])
    return bool(edge.isnan().all()) if whole.dtype.is_floating_point else bool((edge == -1).all())


def poisoned_batch(store, b):
    from pvcnn_amd.data import _build
    pairs = _build(store._describe(b), lambda sd: poisoned(*sd))
    out = tuple({k: v[0] for k, v in part.items()} for part in pairs)
    return out, [v[1] for part in pairs for v in part.values()]


def poisoned_draws(store, b):
    pairs = {k: poisoned(tuple(t.shape), t.dtype) for k, t in store.empty_draws(b).items()}
    return {k: v[0] for k, v in pairs.items()}, [v[1] for v in pairs.values()]


def hand_rows(indices, rng):
    """params rows for the samples of `indices`: the hand-made draws for the three special items of the last frame, random ones else."""
    points, items = world()
    first = len(items) - FRAMES[-1][1]
    rows = []
    for i in indices:
        u = rng.random_sample(4)
        if i == first:
            u = np.array([0.5, 0.5, 0.5, 0.5])
        elif i == first + LOW:
            u[2] = 0.0
        elif i == first + EDGE:
            u[0], u[2] = 0.9990234375, 0.5
        rows.append(fst.params_row(P, items[i]['box'], u))
    return np.stack(rows)


def truth_batch(indices, rows, choices, flip, shift, num_points, rotate, flip_shift, shift_ratio=0.1):
    points, items = world()
    return fst.batch([fst.sample(points[items[i]['frame']], P, items[i], None if rows is None else rows[s], choices[s], flip[s],
                                 shift[s], frustum_rotate=rotate, random_flip=flip_shift, random_shift=flip_shift, shift_ratio=shift_ratio)
                      for s, i in enumerate(indices)])


def draw_choices(indices, rows, num_points, rng, shift_ratio=0.1):
    """-> (positions among the selected points of the box each sample uses (numpy's draws), with a few beyond both ends for the clamp;
    the number of those points per sample)."""
    points, items = world()
    out, counts = [], []
    for s, i in enumerate(indices):
        box = fst.box_used(points[items[i]['frame']], P, items[i]['box'], items[i]['box_3d'], None if rows is None else rows[s], shift_ratio)[1]
        k = int(fst.select(points[items[i]['frame']], box, items[i]['box_3d'])[0].sum())
        ch = rng.choice(k, num_points, replace=True)
        if num_points >= 64:
            ch[5], ch[17] = -3, k + 4
        out.append(ch)
        counts.append(k)
    return np.stack(out).astype(np.int32), np.asarray(counts)


def check(got, want, draws=None):
    x, y = got
    assert same(x['features'], want['features']) and same(x['one_hot_vectors'], want['one_hot_vectors'])
    for k in KEYS:
        assert same(y[k], want[k]), k
    if draws is not None:
        assert same(draws['used'], want['used'])


# -------------------------------------------------------------------------------------------------------------------- 1: parity
FIRST = sum(m for _, m in FRAMES) - FRAMES[-1][1]              # the first item of the last frame
BATCHES = {1: [[FIRST], [FIRST + LOW], [FIRST + EDGE]],        # one launch per branch of the rule
           7: [[FIRST, FIRST + LOW, FIRST + EDGE, FIRST + 1, 0, 4, 7]]}         # four samples of one frame and three other frames


@pytest.mark.parametrize('b', [1, 7])
@pytest.mark.parametrize('num_points', [1, 64, 1024])
@pytest.mark.parametrize('rotate', [True, False])
@pytest.mark.parametrize('flip_shift', [True, False])
def test_parity_mode_equals_the_truth(hip, b, num_points, rotate, flip_shift):
    points, items = world()
    assert len(items) == 16 and [len(p[0]) for p in points] == [n for n, _ in FRAMES]
    store = make_store(num_points, rotate, flip_shift)
    assert len(store) == 16 and store.num_frames == 5 and store.largest_frame == 5003 and store.out_channels == 4
    rng = np.random.RandomState(SEED + num_points + 2 * rotate + flip_shift)
    why = []
    for indices in BATCHES[b]:
        rows = hand_rows(indices, rng)
        choices, counts = draw_choices(indices, rows, num_points, rng)
        flip, shift = rng.random_sample(b), rng.randn(b)
        want = truth_batch(indices, rows, choices, flip, shift, num_points, rotate, flip_shift)
        why += [fst.box_used(points[items[i]['frame']], P, items[i]['box'], items[i]['box_3d'], rows[s])[5] for s, i in enumerate(indices)]
        out, allocations = poisoned_batch(store, b)
        draws, draw_allocations = poisoned_draws(store, b)
        parity = dict(choices=torch.from_numpy(choices), params=torch.from_numpy(rows))
        if flip_shift:
            parity.update(flip=torch.from_numpy(flip), shift=torch.from_numpy(shift))
        got = store.assemble(indices, out, draws_out=draws, **parity)
        assert got is out
        check(got, want, draws)
        assert same(draws['params'], rows) and same(draws['choices'], np.clip(choices, 0, counts[:, None] - 1).astype(np.int32))
        assert all(intact(a) for a in allocations + draw_allocations)
        again = store.assemble(indices, **parity)                                    # fresh tensors; the store's own draws
        check(again, want)
        assert same(store.draws(b)[0], rows) and same(store.draws(b)[1], want['used'])
    assert why[:3] == ['accepted', 'low', 'lost'] and {'accepted', 'low', 'lost'} <= set(why)
    if flip_shift and num_points == 1024 and b == 7:                                # the draws did flip some and not others
        assert 0 < (flip > 0.5).sum() < b


# -------------------------------------------------------------------------------------------------------------------- 2: anchor
@pytest.mark.parametrize('rotate', [True, False])
def test_without_perturbation_it_is_the_packed_store(hip, rotate):
    from pvcnn_amd import frames
    from pvcnn_amd.data import DeviceFrustumKitti
    calib = calibration()
    options = dict(num_heading_angle_bins=12, class_name_to_size_template_id=TEMPLATE_IDS, size_templates=TEMPLATES, random_flip=True,
                   random_shift=True, frustum_rotate=rotate)
    packed = DeviceFrustumKitti.from_frustums([frames.extract_frustums(frame(f)[0], calib, frame(f)[1], SIZE, classes=frame(f)[3],
                                                                       boxes_3d=frame(f)[2]) for f in range(len(FRAMES))], 1024,
                                              classes=NAMES, **options)
    store = make_store(1024, rotate, True, 0.0)
    assert len(packed) == len(store) == 16
    indices = list(range(16))
    rng = np.random.RandomState(SEED + 7)
    choices = torch.from_numpy(draw_choices(indices, None, 1024, rng, shift_ratio=0)[0])
    flip, shift = torch.from_numpy(rng.random_sample(16)), torch.from_numpy(rng.randn(16))
    want = packed.assemble(indices, choices=choices, flip=flip, shift=shift)
    got = store.assemble(indices, choices=choices, flip=flip, shift=shift)
    assert same(got[0]['features'], want[0]['features']) and same(got[0]['one_hot_vectors'], want[0]['one_hot_vectors'])
    for k in KEYS:
        if k != 'center':
            assert same(got[1][k], want[1][k]), k
    a, b = got[1]['center'].cpu().numpy(), want[1]['center'].cpu().numpy()      # the packed store rotates the centre with a BLAS product
    assert (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)).all()
    assert not store.draws(16)[1].any()                                         # no perturbation: every sample is its own box
    check(got, truth_batch(indices, None, choices.numpy(), flip.numpy(), shift.numpy(), 1024, rotate, True, 0))


# -------------------------------------------------------------------------------------------------------------------- 3: device mode
def test_device_mode_records_its_draws_and_parity_mode_reproduces_them(hip):
    from pvcnn_amd import frames
    store = make_store(1024, True, True)
    points, items = world()
    indices = [FIRST + i for i in range(6)] * 16 + [0, 2, 5, 8]
    b = len(indices)
    draws = store.empty_draws(b)
    got = store.assemble(indices, seed=seed_words(31, 4), draws_out=draws)
    back = store.assemble(indices, choices=draws['choices'], params=draws['params'], flip=draws['flip'], shift=draws['shift'])
    for x, y in zip(got, back):
        assert all(same(x[k], y[k]) for k in x)
    assert same(store.draws(b)[0], draws['params']) and same(store.draws(b)[1], draws['used'])
    rows, used = draws['params'].cpu().numpy(), draws['used'].cpu().numpy()
    assert set(used.tolist()) == {0, 1}                                          # some accepted, some fallen back (the 26 px box, often)
    boxes = np.stack([items[i]['box'] for i in indices])
    assert same(rows[:, 4:8], frames.random_shift_box2d(boxes, rows[:, 0:4]))
    angle = np.array([fst.rotation_angle(P, r[4:8]) for r in rows])
    err = max(np.abs(rows[:, 8] - angle).max(), np.abs(rows[:, 9] - np.cos(angle)).max(), np.abs(rows[:, 10] - np.sin(angle)).max())
    print(f'rotation angle, cos, sin of the device against numpy: max |difference| {err:.3e}')
    assert err <= 1e-14
    assert not rows[:, 11].any() and ((rows[:, :4] >= 0) & (rows[:, :4] < 1)).all()
    # and the truth, given the recorded draws, agrees on which box was used and on everything that needs no device trigonometry
    want = truth_batch(indices, rows, draws['choices'].cpu().numpy(), draws['flip'].cpu().numpy(), draws['shift'].cpu().numpy(), 1024, True, True)
    assert same(used, want['used']) and same(got[1]['mask_logits'], want['mask_logits']) and same(got[1]['class_id'], want['class_id'])
    # one seed repeats, another seed or stream differs
    again, other, third = store.empty_draws(b), store.empty_draws(b), store.empty_draws(b)
    store.assemble(indices, seed=seed_words(31, 4), draws_out=again)
    store.assemble(indices, seed=seed_words(32, 4), draws_out=other)
    store.assemble(indices, seed=seed_words(31, 5), draws_out=third)
    assert all(same(again[k], draws[k]) for k in draws)
    assert not same(other['params'], draws['params']) and not same(other['choices'], draws['choices'])
    assert not same(third['params'], draws['params']) and not same(third['choices'], draws['choices'])


def test_device_mode_on_a_frame_of_1032_tiles(hip):
    """66003 in-image points: the 1024-thread scan of the tile counts makes a second trip and carries the first one's total."""
    from pvcnn_amd.frame_store import DeviceKittiFrames
    scan, boxes, boxes_3d, names = frame(8, 66003, 3)
    store = DeviceKittiFrames((scan, calibration(), SIZE, boxes, boxes_3d, names), 512, class_name_to_size_template_id=TEMPLATE_IDS,
                              size_templates=TEMPLATES, random_flip=True, random_shift=True, frustum_rotate=True)
    assert len(store) == 3 and store.largest_frame == 66003
    points = fst.frame_points(scan, P, R0, V2C, SIZE)
    indices = [0, 1, 2, 1, 0]
    draws = store.empty_draws(5)
    got = store.assemble(indices, seed=seed_words(5, 6), draws_out=draws)
    rows = draws['params'].cpu().numpy()
    samples = []
    for s, i in enumerate(indices):
        hot = np.zeros(3, dtype=np.float32)
        hot[NAMES.index(names[i])] = 1
        item = dict(box=boxes[i], box_3d=boxes_3d[i], one_hot=hot, class_id=NAMES.index(names[i]), size_template_id=TEMPLATE_IDS[names[i]],
                    size_residual=(boxes_3d[i][[2, 1, 0]] - TEMPLATES[names[i]]).astype(np.float32))
        samples.append(fst.sample(points, P, item, rows[s], draws['choices'][s].cpu().numpy(), draws['flip'][s].item(), draws['shift'][s].item(),
                                  frustum_rotate=True, random_flip=True, random_shift=True))
    want = fst.batch(samples)
    # the device's cos and sin stand in the recorded rows, so the truth on these rows is the kernel's arithmetic: bit for bit
    check(got, want, draws)
    assert draws['used'].sum().item() >= 1
    assert np.nonzero(fst.select(points, boxes[1], boxes_3d[1])[0])[0].max() >= 1024 * 64     # points behind the scan's first trip


def test_the_uniforms_of_device_mode(hip):
    store = make_store(1, False, False)
    s = 4096
    rng = np.random.RandomState(SEED)
    indices = rng.randint(0, 10, size=s)                                          # the tiny frames
    draws = store.empty_draws(s)
    store.assemble(indices, seed=seed_words(77, 1), draws_out=draws)
    u = draws['params'][:, :4].cpu().numpy()
    assert ((u >= 0) & (u < 1)).all()
    bound = 6 / math.sqrt(12 * s)
    print('column means of the four uniforms', u.mean(axis=0), 'bound', bound)
    assert (np.abs(u.mean(axis=0) - 0.5) <= bound).all()
    assert len(np.unique(u[:, 0])) > s - 8 and not np.array_equal(u[0], u[1]) and not np.array_equal(u[:, 0], u[:, 1])
    assert len({tuple(r) for r in u.tolist()}) == s                               # no two samples share their draws


# -------------------------------------------------------------------------------------------------------------------- 4: capture
def test_feed_replays_in_a_graph_over_two_epochs(hip):
    from pvcnn_amd import frame_store, frames
    from pvcnn_amd.data import DeviceLoader
    store = make_store(64, True, True, 0.1, (1, 2, 3))
    assert len(store) == 9
    loader = DeviceLoader(store, 4, drop_last=True)
    assert len(loader) == 2
    out = loader.static_batch()
    loader.feed()                                                                 # eager once: the scratch exists before the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        loader.feed()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loader.feed()
    seen, copies = [], (frame_store.copies_made(), frames.copies_made())
    for epoch in range(2):
        loader.new_epoch()
        for step in range(len(loader)):
            graph.replay()
            seen.append((loader.order.clone(), step * 4, loader.seed.clone(), [{k: v.clone() for k, v in part.items()} for part in out],
                         [t.clone() for t in store.draws(4)], loader.cursor.clone()))
    assert (frame_store.copies_made(), frames.copies_made()) == copies            # nothing was read on the host while replaying
    torch.cuda.synchronize()
    for order, at, seed, batch, (params, used), cursor in seen:
        assert cursor.item() == at + 4                                            # the cursor walks the epoch
        eager = store.assemble(order[at:at + 4], seed=seed)
        for x, y in zip(batch, eager):
            assert all(same(x[k], y[k]) for k in x)
        assert same(params, store.draws(4)[0]) and same(used, store.draws(4)[1])
    assert not same(seen[0][4][0], seen[1][4][0]) and not same(seen[0][2], seen[2][2])      # fresh draws on every replay


def test_a_captured_train_step_on_the_frame_store(hip):
    from pvcnn_amd import workload
    from pvcnn_amd.data import DeviceLoader
    from pvcnn_amd.dp import GradBucketReducer
    from pvcnn_amd.graph import GraphedTrainStep
    from pvcnn_amd.modules import FrustumPointNetLoss
    from pvcnn_amd.optim import FlatAdam
    from pvcnn_amd.frame_store import DeviceKittiFrames
    calib = calibration()
    # the two large frames (9 objects of 43 points and more): a frustum that repeats ONE point 1024 times has no extent, and the
    # network's coordinate normalisation divides by it -- with any store
    store = DeviceKittiFrames([(frame(4)[0], calib, SIZE) + frame(4)[1:], (frame(9, 20011, 3)[0], calib, SIZE) + frame(9, 20011, 3)[1:]],
                              1024, class_name_to_size_template_id=TEMPLATE_IDS, size_templates=TEMPLATES, random_flip=True,
                              random_shift=True, frustum_rotate=True)
    assert len(store) == 9
    loader = DeviceLoader(store, 3, drop_last=True)
    templates = workload.frustum_size_templates()
    torch.manual_seed(SEED)
    model = workload.FrustumPVCNNE(3, 12, 8, 128, templates, 1, 0.25).to(DEV).train()
    criterion = FrustumPointNetLoss(12, 8, templates).to(DEV)
    x, y = loader.static_batch()

    def fed_loss():
        loader.feed()
        return criterion(model(x), y)
    red = GradBucketReducer(model)
    step = GraphedTrainStep(model, fed_loss, FlatAdam(red, lr=1e-3), red, warmup=3)
    assert step.graph is not None
    loader.cursor.zero_()
    losses = [step().item() for _ in range(3)]
    print('losses of three captured steps fed from the frames', losses)
    assert loader.cursor.item() == 9 and all(math.isfinite(v) for v in losses)


# -------------------------------------------------------------------------------------------------------------------- 5: refusals
def test_refusals_write_nothing(hip):
    from pvcnn_amd import augment
    from pvcnn_amd.data import DeviceLoader
    from pvcnn_amd.frame_store import DeviceKittiFrames
    calib = calibration()
    options = dict(class_name_to_size_template_id=TEMPLATE_IDS, size_templates=TEMPLATES)
    scan, boxes, boxes_3d, names = frame(3)
    small = DeviceKittiFrames(None, 64, max_frame_points=64, **options)
    with pytest.raises(ValueError, match='65 in-image points'):                   # a frame over the cap
        small.add_frame(scan, calib, SIZE, boxes, boxes_3d, names)
    assert len(small) == 0 and small.num_frames == 0 and small.rows is None
    assert small.add_frame(*((frame(2)[0], calib, SIZE) + frame(2)[1:])) == 3 and len(small) == 3       # 64 points fit
    with pytest.raises(ValueError, match='no admitted object'):                   # boxes 24 px high, and classes nobody asked for
        DeviceKittiFrames([(scan, calib, SIZE, boxes * [1, 0, 1, 0] + [0, 100, 0, 124], boxes_3d, names)], 64, **options)
    with pytest.raises(ValueError, match='no admitted object'):
        DeviceKittiFrames([(scan, calib, SIZE, boxes, boxes_3d, ['Van'] * len(names))], 64, **options)
    store = make_store(64, True, True)
    with pytest.raises(ValueError, match='a Frustum-KITTI store cannot be augmented'):
        DeviceLoader(store, 4, drop_last=True, augment=augment.Augment.s3dis(rotate_max=1.0))
    out, allocations = poisoned_batch(store, 2)
    rows = torch.from_numpy(hand_rows([0, 1], np.random.RandomState(0)))
    with pytest.raises(ValueError, match='without `choices`'):                    # parity params without choices
        store.assemble([0, 1], out, params=rows)
    ch = torch.zeros((2, 64), dtype=torch.int32)
    with pytest.raises(ValueError, match='are missing'):                          # parity choices without the other draws
        store.assemble([0, 1], out, choices=ch)
    with pytest.raises(Exception, match='need `choices`'):                        # ... and the entry point says so itself
        from pvcnn_amd import frames
        x, y = out
        frames._call('frame_store_batch', store.rows, store.rows, store.uv, store.frame_offsets, store.num_frames, store.rows.shape[0],
                     store.largest_frame, store.item_f64, store.item_f32, store.item_i64, len(store), 3, 12, 1, 1, 1, 0.1, 25.0,
                     torch.zeros(2, dtype=torch.int64, device=DEV), 2, None, 2, 64, rows.to(DEV), None, None, None, seed_words(1, 2),
                     x['features'], x['one_hot_vectors'], y['mask_logits'], y['center'], y['heading_bin_id'], y['heading_residual'],
                     y['size_template_id'], y['size_residual'], y['class_id'], None, None, None, None, None)
    torch.cuda.synchronize()
    for part in out:
        for t in part.values():
            assert bool(t.isnan().all()) if t.dtype.is_floating_point else bool((t == -1).all())
    assert all(intact(a) for a in allocations)
    with pytest.raises(TypeError):
        DeviceKittiFrames.from_frustums([], 64)
