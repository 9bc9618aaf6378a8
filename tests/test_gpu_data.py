"""Device-resident datasets on the GPU (pvcnn_amd/data.py over csrc/batch.hip, through the C ABI): parity mode against the reference's
golden batches and against the torch formulation at the benched sizes; device mode's ranges, distinctness, seeding and distributions
(bounds derived from the distributions, seeds fixed: deterministic); 64-bit row addressing; the captured `feed()`; one end-to-end
GraphedTrainStep that feeds itself."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as tf

from test_data_host import GOLDEN, golden_cases, same_batch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED = 1588147245


def seed_words(a, b):
    return torch.tensor([a, b], dtype=torch.int64, device=DEV)


def flat(batch):
    out = []
    for part in batch:
        out += list(part.values()) if isinstance(part, dict) else [part]
    return out


def equal_batches(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.cpu(), y.cpu()) for x, y in zip(flat(a), flat(b)))


def indexed_s3dis(counts, num_points, device=DEV, with_normalized_coords=True):
    """An S3DIS store whose channel 0 is the row's position within its window (so an emitted column names the row it came from)."""
    from pvcnn_amd.data import DeviceS3DIS
    rng = np.random.RandomState(SEED)
    p = max(counts)
    data = rng.rand(len(counts), p, 9).astype(np.float32)
    data[:, :, 0] = np.arange(p, dtype=np.float32)[None, :]
    label = rng.randint(0, 13, size=(len(counts), p))
    return DeviceS3DIS(data, label, np.array(counts), num_points, with_normalized_coords=with_normalized_coords, device=device)


def numpy_choices(rng, counts, num_points):
    return torch.from_numpy(np.stack([rng.choice(n, num_points, replace=n < num_points) for n in counts]).astype(np.int32))


# ---------------------------------------------------------------------------------------------------------------- parity mode
def test_parity_mode_equals_the_reference_golden_batches(hip):
    golden = torch.load(GOLDEN)
    count = 0
    for name, build, indices, draws, want in golden_cases(golden):
        store = build(DEV)
        same_batch(store.assemble(indices, **draws), want, name)
        out = store.empty_batch(len(indices))                       # and into preallocated tensors
        assert store.assemble(indices, out, **draws) is out
        same_batch(out, want, name + ' (out=)')
        count += 1
    assert count == 21


def test_parity_mode_equals_the_torch_formulation_as_benched_s3dis(hip):
    rng = np.random.RandomState(SEED)
    counts = [4096, 8192] + rng.randint(4096, 8193, size=22).tolist()
    store = indexed_s3dis(counts, 4096)
    host = store.to('cpu')
    for with_norm in (True, False):
        store.with_normalized_coords = host.with_normalized_coords = with_norm
        idx = rng.permutation(len(counts))[:16].tolist()
        ch = numpy_choices(rng, [counts[i] for i in idx], 4096)
        assert equal_batches(store.assemble(idx, choices=ch), host.assemble_reference(idx, choices=ch))


def test_parity_mode_equals_the_torch_formulation_as_benched_shapenet(hip):
    from pvcnn_amd.data import DeviceShapeNet
    rng = np.random.RandomState(SEED)
    counts = rng.randint(1500, 3000, size=12).tolist()
    clouds = [np.concatenate([rng.randn(n, 6), rng.randint(0, 50, size=(n, 1))], axis=1) for n in counts]
    store = DeviceShapeNet(clouds, rng.randint(0, 16, size=12).tolist(), 2048, device=DEV)
    idx = rng.permutation(12)[:8].tolist()
    ch = torch.from_numpy(np.stack([rng.choice(counts[i], 2048, replace=True) for i in idx]).astype(np.int32))
    z = torch.from_numpy(rng.randn(8, 3, 2048))
    z[0, 0, :4] = torch.tensor([5.0, -5.0, 7.5, -9.0], dtype=torch.float64)
    assert equal_batches(store.assemble(idx, choices=ch, jitter=z), store.to('cpu').assemble_reference(idx, choices=ch, jitter=z))


def frustum_split(rng, w, lo=200, hi=3000, positive_x=False, **options):
    from pvcnn_amd.data import DeviceFrustumKitti
    classes = ('Car', 'Pedestrian', 'Cyclist')
    counts = rng.randint(lo, hi, size=w).tolist()
    clouds = [(rng.randn(n, 4) * [2, 1, 5, 1] + [0, 1, 20, 0]).astype(np.float32) for n in counts]
    if positive_x:
        clouds = [np.concatenate([np.abs(c[:, :1]) + 0.5, c[:, 1:]], axis=1) for c in clouds]
    names = [classes[i % 3] for i in range(w)]
    templates = {c: rng.rand(3) + 1 for c in classes}
    store = DeviceFrustumKitti(clouds, [rng.randint(0, 2, size=n) for n in counts], [rng.randn(8, 3) + [1, 1, 20] for _ in range(w)],
                               [np.float64(h) for h in rng.uniform(-np.pi, np.pi, size=w)], [rng.rand(3) + 1 for _ in range(w)], names,
                               [np.float64(a) for a in rng.uniform(-2, -1, size=w)], 1024, classes=classes,
                               class_name_to_size_template_id={'Car': 0, 'Pedestrian': 3, 'Cyclist': 5}, size_templates=templates,
                               device=DEV, **options)
    return store, counts


def test_parity_mode_equals_the_torch_formulation_as_benched_frustum(hip):
    rng = np.random.RandomState(SEED)
    store, counts = frustum_split(rng, 48, random_flip=True, random_shift=True, frustum_rotate=True)
    idx = rng.permutation(48)[:32].tolist()
    ch = torch.from_numpy(np.stack([rng.choice(counts[i], 1024, replace=True) for i in idx]).astype(np.int32))
    flip, shift = torch.from_numpy(rng.random_sample(32)), torch.from_numpy(rng.randn(32))
    got = store.assemble(idx, choices=ch, flip=flip, shift=shift)
    assert equal_batches(got, store.to('cpu').assemble_reference(idx, choices=ch, flip=flip, shift=shift))


# ---------------------------------------------------------------------------------------------------------------- device mode
def test_device_mode_ranges_distinctness_seeding_and_provenance(hip):
    counts = [4096, 8192, 5000, 7001, 100, 1, 4095, 6000]
    store = indexed_s3dis(counts, 4096)
    idx = list(range(len(counts)))
    a = store.assemble(idx, seed=seed_words(11, 5))
    b = store.assemble(idx, seed=seed_words(11, 5))
    c = store.assemble(idx, seed=seed_words(12, 5))
    d = store.assemble(idx, seed=seed_words(11, 6))
    assert equal_batches(a, b) and not equal_batches(a, c) and not equal_batches(a, d)
    picks = a[0][:, 0, :].cpu()                                                        # channel 0 names the row
    assert torch.equal(picks, picks.round())
    for i, n in enumerate(counts):
        row = picks[i].long()
        assert 0 <= int(row.min()) and int(row.max()) < n, (i, n)
        if n >= 4096:
            assert row.unique().numel() == 4096, (i, n)                               # without replacement
        elif n > 1:
            assert row.unique().numel() > 1
    assert sorted(picks[0].long().tolist()) == list(range(4096))                       # n == N: a permutation
    assert picks[0].long().tolist() != list(range(4096))
    # every emitted column is a stored row of the right item: the torch formulation on the recovered indices gives the same batch
    assert equal_batches(a, store.to('cpu').assemble_reference(idx, choices=picks.to(torch.int32)))
    # without a seed the words come from torch's device generator: torch.manual_seed governs the batch
    torch.manual_seed(3); e = store.assemble(idx)
    torch.manual_seed(3); f = store.assemble(idx)
    g = store.assemble(idx)
    assert equal_batches(e, f) and not equal_batches(e, g)
    # windows beyond the LDS-resident selection are refused in words
    big = indexed_s3dis([9000, 5000], 4096)
    with pytest.raises(RuntimeError, match='8192'):
        big.assemble([0, 1])
    assert big.assemble([0, 1], choices=numpy_choices(np.random.RandomState(1), [9000, 5000], 4096))[0].shape == (2, 9, 4096)


def test_device_mode_selection_is_uniform(hip):
    """T assemblies of one window of n points, N of them without replacement each: the inclusion count of a point is Binomial(T, N/n)
    (sd sqrt(T p (1 - p))), its position when included is uniform on [0, N) (sd N / sqrt(12) per draw).  Every point within 5 sd.
    With replacement (n < N) the count of a point is Binomial(T N, 1/n)."""
    n, N, T = 6000, 4096, 64
    store = indexed_s3dis([n, 3000], N)
    picks = store.assemble([0] * T, seed=seed_words(SEED, 1))[0][:, 0, :].long()        # (T, N)
    counts = torch.bincount(picks.flatten(), minlength=n).double().cpu()
    p = N / n
    print('inclusion counts: min', counts.min().item(), 'max', counts.max().item(), 'mean', T * p, 'sd', math.sqrt(T * p * (1 - p)))
    assert (counts - T * p).abs().max().item() <= 5 * math.sqrt(T * p * (1 - p))
    pos = torch.arange(N, device=DEV).expand(T, N)
    sums = torch.zeros(n, dtype=torch.float64, device=DEV).index_add_(0, picks.flatten(), pos.flatten().double()).cpu()
    mean_pos = sums / counts
    sd = N / torch.sqrt(12 * counts)
    print('mean position: worst', ((mean_pos - (N - 1) / 2).abs() / sd).max().item(), 'sd')
    assert ((mean_pos - (N - 1) / 2).abs() <= 5 * sd).all()
    picks = store.assemble([1] * T, seed=seed_words(SEED, 2))[0][:, 0, :].long()
    counts = torch.bincount(picks.flatten(), minlength=3000).double().cpu()
    q = 1 / 3000
    print('with replacement: min', counts.min().item(), 'max', counts.max().item(), 'mean', T * N * q)
    assert (counts - T * N * q).abs().max().item() <= 5 * math.sqrt(T * N * q * (1 - q))


def test_device_mode_jitter_and_flip_distributions(hip):
    """Jitter = clip(0.01 z, -0.05, 0.05): |.| <= 0.05 and variance s^2 (1 - 2 Q(c) - 2 c phi(c) + 2 c^2 Q(c)) at c = 5 (Q the normal
    tail, phi the density); the sample variance of M values has sd s^2 sqrt(2 / M) (normal kurtosis).  Flips are Bernoulli(1/2)."""
    from pvcnn_amd.data import DeviceShapeNet
    rng = np.random.RandomState(SEED)
    clouds = [np.concatenate([np.zeros((n, 3)), rng.randn(n, 3), rng.randint(0, 50, size=(n, 1))], axis=1) for n in (1800, 2500)]
    store = DeviceShapeNet(clouds, [3, 7], 2048, normalize=False, jitter=True, device=DEV)
    x, _ = store.assemble([0, 1] * 4, seed=seed_words(SEED, 3))
    j = x[:, :3].double().flatten().cpu()
    assert j.abs().max().item() <= float(np.float32(0.05)) and j.abs().max().item() > 0.03
    c, s2, m = 5.0, 1e-4, j.numel()
    tail, phi = 0.5 * math.erfc(c / math.sqrt(2)), math.exp(-c * c / 2) / math.sqrt(2 * math.pi)
    var = s2 * (1 - 2 * tail - 2 * c * phi + 2 * c * c * tail)
    got = (j * j).mean().item() - j.mean().item() ** 2
    print('jitter variance', got, 'expected', var, 'sd', s2 * math.sqrt(2 / m), 'mean', j.mean().item())
    assert abs(got - var) <= 5 * s2 * math.sqrt(2 / m)
    assert abs(j.mean().item()) <= 5 * math.sqrt(s2 / m)
    assert torch.equal(x[:, 6:].cpu().sum(dim=1), torch.ones(8, 2048)) and (x[0, 6 + 3] == 1).all() and (x[1, 6 + 7] == 1).all()
    # flip: x is positive in the store, so a flipped sample is the one whose x is negative
    store, _ = frustum_split(rng, 4, positive_x=True, random_flip=True, random_shift=True)
    b = 1024
    x = store.assemble([i % 4 for i in range(b)], seed=seed_words(SEED, 4))[0]['features']
    neg = (x[:, 0] < 0)
    assert torch.equal(neg.all(dim=1), neg.any(dim=1))                                  # a sample flips as a whole
    flips = int(neg.all(dim=1).sum())
    print('flips', flips, 'of', b)
    assert abs(flips - b / 2) <= 5 * math.sqrt(b) / 2


# ---------------------------------------------------------------------------------------------------------- 64-bit addressing
def test_rows_beyond_two_to_the_31_floats(hip):
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * 2 ** 30:
        pytest.skip('less than 24 GB of device memory free')
    per, w, N = 8000, 30000, 4096
    rows_total = per * w
    assert rows_total * 9 > 2 ** 31
    store = indexed_s3dis([per, per], N)
    rows = torch.empty((rows_total, 9), dtype=torch.float32, device=DEV)
    flat_rows = rows.view(-1)
    step = 1 << 26
    for a in range(0, flat_rows.numel(), step):                                        # element e holds e mod a prime below 2^24: exact in fp32
        e = torch.arange(a, min(a + step, flat_rows.numel()), device=DEV, dtype=torch.int64)
        flat_rows[a:a + e.numel()] = e.remainder_(16777213).float()
        del e
    store.rows = rows
    store.labels = (torch.arange(rows_total, device=DEV, dtype=torch.int64) % 251).to(torch.uint8)
    store.offsets = torch.arange(w + 1, device=DEV, dtype=torch.int64) * per
    assert store.nbytes > 2 ** 33
    idx = [w - 1, w - 2, 29900, 29831, 0, 15000]
    assert (idx[3] * per) * 9 > 2 ** 31
    ch = numpy_choices(np.random.RandomState(SEED), [per] * len(idx), N).to(DEV)
    global_rows = (torch.tensor(idx, device=DEV) * per)[:, None] + ch.long()
    want_x = rows.index_select(0, global_rows.flatten()).view(len(idx), N, 9).permute(0, 2, 1).contiguous()
    want_y = store.labels.index_select(0, global_rows.flatten()).view(len(idx), N).long()
    x, y = store.assemble(idx, choices=ch)
    assert torch.equal(x, want_x) and torch.equal(y, want_y)
    xd, yd = store.assemble(idx, seed=seed_words(SEED, 9))                            # device mode addresses the same way
    e0 = xd[:, 0, :].double()                                                          # element id of channel 0 (mod the prime) -> row
    for c in range(1, 9):
        assert torch.equal(xd[:, c, :].double(), (e0 + c).remainder(16777213))
    del store, rows
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------- loader, graphs
def test_loader_iterates_an_epoch_like_a_dataloader(hip):
    from pvcnn_amd.data import DeviceLoader
    store = indexed_s3dis([300, 500, 64, 1000, 20, 128, 700], 256)
    loader = DeviceLoader(store, 3, shuffle=True, drop_last=False)
    assert len(loader) == 3
    shapes = [(x.shape, y.shape, x.device.type) for x, y in loader]
    assert shapes == [((3, 9, 256), (3, 256), 'cuda'), ((3, 9, 256), (3, 256), 'cuda'), ((1, 9, 256), (1, 256), 'cuda')]
    assert loader.cursor.item() == 7 and sorted(loader.order.tolist()) == list(range(7))
    assert len(DeviceLoader(store, 3, drop_last=True)) == 2


def test_captured_feed_walks_the_epoch(hip):
    from pvcnn_amd.data import DeviceLoader
    rng = np.random.RandomState(SEED)
    counts = rng.randint(600, 1200, size=12).tolist()
    store = indexed_s3dis(counts, 512)
    loader = DeviceLoader(store, 4, shuffle=True, drop_last=True)
    x, y = loader.static_batch()
    ch = torch.zeros((4, 512), dtype=torch.int32, device=DEV)
    draws = [torch.from_numpy(rng.randint(0, 600, size=(4, 512)).astype(np.int32)).to(DEV) for _ in range(3)]
    want = []
    for k in range(3):                                                                  # k eager feeds
        ch.copy_(draws[k])
        loader.feed(choices=ch)
        want.append((x.clone(), y.clone()))
    assert loader.cursor.item() == 12
    order = loader.order.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        loader.feed(choices=ch)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loader.feed(choices=ch)
    loader.cursor.zero_()
    assert torch.equal(loader.order, order)
    for k in range(3):
        ch.copy_(draws[k])
        graph.replay()
        assert torch.equal(x, want[k][0]) and torch.equal(y, want[k][1]), k
        assert loader.cursor.item() == 4 * (k + 1)
    # device mode: the seed words are drawn inside the graph, so every replay has fresh numbers
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        loader.feed()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph2):
        loader.feed()
    seen = []
    for _ in range(2):
        loader.cursor.zero_()
        graph2.replay()
        seen.append(x.clone())
    assert not torch.equal(seen[0], seen[1])
    picks = seen[1][:, 0, :].cpu().to(torch.int32)
    assert equal_batches((seen[1], y), store.to('cpu').assemble_reference(order[:4].tolist(), choices=picks))


def test_graphed_train_step_feeds_itself(hip):
    """GraphedTrainStep with feed() inside loss_fn: three replays train on three consecutive batches of the epoch, with the same
    losses as a twin whose static inputs are overwritten (x.copy_) with those batches assembled ahead."""
    from pvcnn_amd import workload
    from pvcnn_amd.data import DeviceLoader
    from pvcnn_amd.dp import GradBucketReducer
    from pvcnn_amd.graph import GraphedTrainStep
    from pvcnn_amd.optim import FlatAdam
    torch.manual_seed(0)
    rng = np.random.RandomState(SEED)
    counts = rng.randint(2048, 3000, size=8).tolist()
    store = indexed_s3dis(counts, 2048)
    store.rows[:, 0] = store.rows[:, 1] * 1.5                                           # plausible coordinates in channel 0 as well
    model = workload.PVCNN(13, 6, width_multiplier=0.25).to(DEV).train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    twin = copy.deepcopy(model)
    loader = DeviceLoader(store, 2, shuffle=False, drop_last=True)
    loader.order = torch.tensor([0, 1] * 4 + [2, 3, 4, 5, 6, 7], dtype=torch.int64, device=DEV)     # the warm-up sees one batch only
    ch = torch.from_numpy(rng.randint(0, 2048, size=(2, 2048)).astype(np.int32)).to(DEV)
    batches = [tuple(t.clone() for t in store.assemble(loader.order[8 + 2 * k:10 + 2 * k], choices=ch)) for k in range(3)]
    warm = store.assemble([0, 1], choices=ch)

    def fed_loss():
        x, y = loader.feed(choices=ch)
        return tf.cross_entropy(model(x), y)
    red = GradBucketReducer(model)
    step = GraphedTrainStep(model, fed_loss, FlatAdam(red, lr=2e-3, weight_decay=1e-5), red, warmup=3)
    assert step.graph is not None and 6 <= loader.cursor.item() <= 8                   # the eager warm-up steps; the capture runs nothing
    loader.cursor.fill_(8)
    got = [step().item() for _ in range(3)]
    assert loader.cursor.item() == 14

    sx, sy = warm[0].clone(), warm[1].clone()
    red2 = GradBucketReducer(twin)
    step2 = GraphedTrainStep(twin, lambda: tf.cross_entropy(twin(sx), sy), FlatAdam(red2, lr=2e-3, weight_decay=1e-5), red2, warmup=3)
    want = []
    for bx, by in batches:
        sx.copy_(bx); sy.copy_(by)
        want.append(step2().item())
    print('losses fed in the graph', got, 'fed by copy', want)
    assert all(math.isfinite(v) for v in got)
    assert got == want
