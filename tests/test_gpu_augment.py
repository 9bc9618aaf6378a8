"""Batch augmentation on the GPU (pvcnn_amd/augment.py over csrc/augment.hip, through the C ABI): parity mode against the torch
formulation, bit for bit, on plain tensors and on offset, batch-strided views inside poisoned allocations; device mode as parity mode
on its own draws; ranges and distributions of the draws (bounds derived from the stated distributions and n, seeds fixed:
deterministic); the captured `DeviceLoader.feed(augment=...)`; the unchanged loader; refusals."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as tf

import embedded
from pvcnn_amd.augment import PARAMS, Augment
from test_gpu_data import equal_batches, indexed_s3dis, seed_words

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED = 1588147245

ALL_ON = dict(rotate_max=math.pi, perturb_sigma=0.06, perturb_clip=0.18, flip_prob=(0.5, 0.25, 0.75), scale=(0.8, 1.25), translate=0.2,
              jitter_sigma=0.01, jitter_clip=0.015, dropout_max=0.875)
STAGES = [ALL_ON] + [{k: ALL_ON[k] for k in keys} for keys in (['rotate_max'], ['perturb_sigma', 'perturb_clip'], ['flip_prob'], ['scale'],
                                                              ['translate'], ['jitter_sigma', 'jitter_clip'], ['dropout_max'])]


def numpy_draws(rng, aug, b, n):
    """(params (B, 24) fp64, jitter (B, 3, N) fp32, keep (B, N) fp32) drawn with numpy from the stated distributions."""
    raw = np.zeros((b, PARAMS))
    raw[:, 14] = rng.uniform(-aug.rotate_max, aug.rotate_max, b)
    raw[:, 15:18] = np.clip(aug.perturb_sigma * rng.randn(b, 3), -aug.perturb_clip, aug.perturb_clip)
    raw[:, 18:21] = rng.random_sample((b, 3))
    raw[:, :9] = aug.compose_reference(raw).reshape(b, 9)
    raw[:, 9] = rng.uniform(aug.scale[0], aug.scale[1], b)
    raw[:, 10:13] = rng.uniform(-aug.translate, aug.translate, (b, 3))
    raw[:, 13] = rng.random_sample(b) * aug.dropout_max
    return (torch.from_numpy(raw), torch.from_numpy(rng.randn(b, 3, n).astype(np.float32)),
            torch.from_numpy(rng.random_sample((b, n)).astype(np.float32)))


def batch(rng, b, c, n):
    return torch.from_numpy(rng.randn(b, c, n).astype(np.float32)), torch.from_numpy(rng.randint(0, 50, size=(b, n)))


def identity_params(b):
    p = torch.zeros((b, PARAMS), dtype=torch.float64)
    p[:, 0] = p[:, 4] = p[:, 8] = p[:, 9] = 1.0
    return p


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b.cpu())


# ------------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize('b,c,n,shapenet', [(3, 9, 257, False), (2, 6, 1, True), (1, 22, 4096, True), (2, 9, 70001, False),
                                            (4, 6, 65536, True)])               # the last: B N = 2^18, where the 16-byte path begins
def test_parity_mode_equals_the_torch_formulation(hip, b, c, n, shapenet):
    rng = np.random.RandomState(SEED)
    x, y = batch(rng, b, c, n)
    xd, yd = x.to(DEV), y.to(DEV)
    for ranges in STAGES:
        aug = Augment.shapenet(**ranges) if shapenet else Augment.s3dis(**ranges)
        params, jitter, keep = numpy_draws(rng, aug, b, n)
        keep[:, -1] = 0.0                                                               # the last point is dropped whenever dropout is on
        want_x, want_y = aug.augment_reference(x, y, params, jitter, keep)
        got_x, got_y = aug.augment(xd, yd, params=params, jitter=jitter, keep=keep)
        assert same_bits(got_x, want_x) and same_bits(got_y, want_y), sorted(ranges)
        assert same_bits(aug.augment(xd, params=params, jitter=jitter, keep=keep), want_x), sorted(ranges)         # without targets
        if not aug.dropout_on:                                                          # in place, where that is allowed
            xi = xd.clone()
            assert aug.augment(xi, params=params, jitter=jitter, out=xi) is xi and same_bits(xi, want_x), sorted(ranges)
        elif n > 1:
            assert not torch.equal(want_x, aug.augment_reference(x, y, params, jitter, torch.ones(b, n))[0])     # points were dropped


# ------------------------------------------------------------------------------------------------------------- 2. offset views
def embed_targets(t, off, extra):
    """t (B, N) int64 -> (view, whole): rows N + extra apart, `off` elements behind the start of a -1-filled allocation's middle."""
    b, n = t.shape
    whole = torch.full((4096 + off + b * (n + extra) + 4096,), -1, dtype=torch.int64, device=t.device)
    view = whole[4096 + off:4096 + off + b * (n + extra)].view(b, n + extra)[:, extra // 2:extra // 2 + n]
    view.copy_(t)
    return view, whole


def targets_intact(whole, view):
    first = (view.data_ptr() - whole.data_ptr()) // 8
    mask = torch.ones(whole.numel(), dtype=torch.bool, device=whole.device)
    idx = (torch.arange(view.shape[0], device=whole.device)[:, None] * view.stride(0) + torch.arange(view.shape[1], device=whole.device)) + first
    mask[idx.reshape(-1)] = False
    return bool((whole[mask] == -1).all())


@pytest.mark.parametrize('b,c,n', [(3, 9, 256), (2, 6, 37), (2, 6, 131072)])
def test_offset_batch_strided_views_inside_poisoned_allocations(hip, b, c, n):
    rng = np.random.RandomState(SEED + 1)
    x, y = batch(rng, b, c, n)
    aug = Augment(layout=[('position', 0), ('direction', 3)], **ALL_ON)
    params, jitter, keep = numpy_draws(rng, aug, b, n)
    want_x, want_y = aug.augment_reference(x, y, params, jitter, keep)
    for off in (0, 1, 2, 3):                                                            # off 0, B N = 2^18: the 16-byte path; else scalar
        src, src_whole = embedded.embed_rows(x.to(DEV), off, 4)
        dst, dst_whole = embedded.embed_rows(torch.zeros_like(x, device=DEV), (off + 1) % 4 if off else 0, 2)
        tsrc, tsrc_whole = embed_targets(y.to(DEV), off, 6)
        tdst, tdst_whole = embed_targets(torch.zeros_like(y, device=DEV), off % 2, 2)
        assert src.stride(0) == (c + 4) * n and dst.stride(0) == (c + 2) * n and tsrc.stride(0) == n + 6
        assert n % 4 or (src.data_ptr() % 16 == 0) == (off == 0)
        got = aug.augment(src, tsrc, out=dst, out_targets=tdst, params=params, jitter=jitter, keep=keep)
        assert got[0] is dst and got[1] is tdst
        assert same_bits(dst, want_x) and same_bits(tdst, want_y), off
        assert embedded.rows_intact(src_whole, src) and embedded.rows_intact(dst_whole, dst), off
        assert targets_intact(tsrc_whole, tsrc) and targets_intact(tdst_whole, tdst), off
        assert same_bits(src, x) and same_bits(tsrc, y)
        # device mode through the same views: its own draws, fed back, give the same bits on plain tensors
        dst.zero_(); tdst.zero_()
        _, draws = aug.augment(src, tsrc, out=dst, out_targets=tdst, seed=seed_words(SEED, off), return_draws=True)
        again = aug.augment(x.to(DEV), y.to(DEV), **draws)
        assert same_bits(dst, again[0]) and same_bits(tdst, again[1]), off
        assert embedded.rows_intact(dst_whole, dst) and targets_intact(tdst_whole, tdst), off


def test_batch_stride_beyond_two_to_the_31_elements(hip):
    """Sample addressing is 64-bit: the second sample of `src` starts more than 2^31 floats behind the first (untouched memory in
    between: torch.empty does not write it)."""
    rng = np.random.RandomState(SEED + 2)
    b, c, n = 2, 9, 515
    x, y = batch(rng, b, c, n)
    aug = Augment.s3dis(**ALL_ON)
    params, jitter, keep = numpy_draws(rng, aug, b, n)
    stride = 2 ** 31 + 4099
    whole = torch.empty((stride + c * n,), dtype=torch.float32, device=DEV)
    src = whole.as_strided((b, c, n), (stride, n, 1))
    src.copy_(x)
    got_x, got_y = aug.augment(src, y.to(DEV), params=params, jitter=jitter, keep=keep)
    want_x, want_y = aug.augment_reference(x, y, params, jitter, keep)
    assert same_bits(got_x, want_x) and same_bits(got_y, want_y)
    back = torch.empty_like(whole).as_strided((b, c, n), (stride, n, 1))
    aug.augment(got_x, params=identity_params(b), jitter=torch.zeros(b, 3, n), keep=torch.ones(b, n), out=back)       # and as a destination
    assert same_bits(back, want_x)
    del whole, src, back
    torch.cuda.empty_cache()


# --------------------------------------------------------------------------------------------------------------- 3. device mode
def test_device_mode_is_parity_mode_on_its_own_draws(hip):
    rng = np.random.RandomState(SEED + 3)
    for b, c, n, shapenet in ((4, 9, 1000, False), (3, 22, 515, True)):
        x, y = (t.to(DEV) for t in batch(rng, b, c, n))
        aug = Augment.shapenet(**ALL_ON) if shapenet else Augment.s3dis(**ALL_ON)
        (got_x, got_y), draws = aug.augment(x, y, seed=seed_words(SEED, 7), return_draws=True)
        assert draws['params'].shape == (b, PARAMS) and draws['jitter'].shape == (b, 3, n) and draws['keep'].shape == (b, n)
        again_x, again_y = aug.augment(x, y, **draws)
        assert same_bits(got_x, again_x) and same_bits(got_y, again_y)
        want_x, want_y = aug.augment_reference(x.cpu(), y.cpu(), draws['params'].cpu(), draws['jitter'].cpu(), draws['keep'].cpu())
        assert same_bits(got_x, want_x) and same_bits(got_y, want_y)
        assert not torch.equal(got_x[:, :3], x[:, :3]) and torch.equal(got_x[:, 6:, 0], x[:, 6:, 0])
        # the composed matrix: entries of magnitude <= 1, each fewer than 50 fp64 roundings from the truth
        p = draws['params'].cpu().numpy()
        err = np.abs(p[:, :9].reshape(b, 3, 3) - aug.compose_reference(p)).max()
        print('Rp against compose_reference: max abs error', err)
        assert err <= 1e-12
        assert np.array_equal(p[:, 21:], np.zeros((b, 3)))


def test_stages_that_are_off_are_exact_identities(hip):
    rng = np.random.RandomState(SEED + 4)
    x, y = (t.to(DEV) for t in batch(rng, 5, 9, 300))
    (got_x, got_y), draws = Augment.s3dis().augment(x, y, seed=seed_words(SEED, 8), return_draws=True)
    p = draws['params'].cpu()
    assert torch.equal(p[:, :18].view(torch.int64), identity_params(5)[:, :18].view(torch.int64))             # bit for bit: no -0.0
    assert draws['jitter'] is None and draws['keep'] is None
    assert torch.equal(got_x.view(torch.int32), x.view(torch.int32)) and torch.equal(got_y, y)
    for ranges in STAGES[1:]:                                                           # one stage on: the others stay exact
        aug = Augment.s3dis(**ranges)
        p = aug.draw(64, seed_words(SEED, 9)).cpu()
        on = set(ranges)
        if not on & {'rotate_max', 'perturb_sigma', 'flip_prob'}:
            assert torch.equal(p[:, :9], identity_params(64)[:, :9])
        if on == {'flip_prob'}:
            assert torch.equal(p[:, :9].abs(), identity_params(64)[:, :9]) and (p[:, 0] == -1).any() and (p[:, 0] == 1).any()
        if 'rotate_max' not in on:
            assert (p[:, 14] == 0).all()
        if 'perturb_sigma' not in on:
            assert (p[:, 15:18] == 0).all()
        if 'scale' not in on:
            assert (p[:, 9] == 1).all()
        if 'translate' not in on:
            assert (p[:, 10:13] == 0).all()
        if 'dropout_max' not in on:
            assert (p[:, 13] == 0).all()
        assert not torch.signbit(p[:, :14]).logical_and(p[:, :14] == 0).any()


# ------------------------------------------------------------------------------------------------------------- 4. distributions
def normal_tail(k):
    return 0.5 * math.erfc(k / math.sqrt(2)), math.exp(-k * k / 2) / math.sqrt(2 * math.pi)


def clipped_normal_moments(sigma, clip):
    """(variance, fourth moment) of clip(sigma Z, +-clip): with k = clip / sigma, Q the normal tail and phi the density,
    E[Z^2; |Z| < k] = (1 - 2 Q) - 2 k phi, E[Z^4; |Z| < k] = 3 ((1 - 2 Q) - 2 k phi) - 2 k^3 phi, plus the two atoms at +-k."""
    k = clip / sigma
    q, phi = normal_tail(k)
    m2 = (1 - 2 * q) - 2 * k * phi
    return sigma ** 2 * (m2 + 2 * k * k * q), sigma ** 4 * (3 * m2 - 2 * k ** 3 * phi + 2 * k ** 4 * q)


def uniform_moments(lo, hi):
    half = (hi - lo) / 2
    return half ** 2 / 3, half ** 4 / 5


def check_moments(name, sample, mean, var, m4):
    """The sample mean within 6 sd / sqrt(n) of `mean`; the mean squared deviation from `mean` within 6 sqrt((m4 - var^2) / n) of `var`
    (its exact standard error: m4 is the fourth central moment)."""
    s = sample.double().flatten().cpu()
    n = s.numel()
    got_mean, got_var = s.mean().item(), ((s - mean) ** 2).mean().item()
    print(f'{name}: n {n} mean {got_mean:.6g} (exact {mean:.6g}, se {math.sqrt(var / n):.3g}) '
          f'variance {got_var:.6g} (exact {var:.6g}, se {math.sqrt((m4 - var * var) / n):.3g})')
    assert abs(got_mean - mean) <= 6 * math.sqrt(var / n), name
    assert abs(got_var - var) <= 6 * math.sqrt((m4 - var * var) / n), name


def check_uniform(name, sample, lo, hi):
    assert lo <= sample.min().item() and sample.max().item() <= hi, name
    check_moments(name, sample, (lo + hi) / 2, *uniform_moments(lo, hi))


def test_per_cloud_draws_ranges_and_distributions(hip):
    b = 4096
    ranges = dict(ALL_ON, perturb_clip=0.09)                                            # 1.5 sigma: both clips are hit often
    aug = Augment.s3dis(**ranges)
    params = aug.draw(b, seed_words(SEED, 11))
    assert torch.equal(params, aug.draw(b, seed_words(SEED, 11)))                       # the same seed: the same bits
    other_stream, other_key = aug.draw(b, seed_words(SEED, 12)), aug.draw(b, seed_words(SEED + 1, 11))
    assert not torch.equal(params, other_stream) and not torch.equal(params, other_key)
    assert not (params[:, 9:21] == other_stream[:, 9:21]).all(dim=0).any()              # every column is drawn anew
    assert torch.unique(params, dim=0).shape[0] == b                                    # no two clouds share a row
    for col in list(range(9, 21)):
        assert torch.unique(params[:, col]).numel() > b // 2 or col in (15, 16, 17), col
    p = params.cpu()
    check_uniform('theta', p[:, 14], -math.pi, math.pi)
    for k, name in enumerate('abc'):
        a = p[:, 15 + k]
        assert a.abs().max().item() <= 0.09 and (a == 0.09).any() and (a == -0.09).any(), name
        check_moments('perturbation ' + name, a, 0.0, *clipped_normal_moments(0.06, 0.09))
    for k, prob in enumerate(ALL_ON['flip_prob']):
        check_uniform(f'flip uniform {k}', p[:, 18 + k], 0.0, 1.0)
        freq = (p[:, 18 + k] < prob).double().mean().item()
        print(f'flip {k}: frequency {freq:.4f} of p {prob}')
        assert abs(freq - prob) <= 6 * math.sqrt(prob * (1 - prob) / b)
    check_uniform('scale', p[:, 9], 0.8, 1.25)
    for k in range(3):
        check_uniform(f'translation {k}', p[:, 10 + k], -0.2, 0.2)
    check_uniform('dropout ratio', p[:, 13], 0.0, 0.875)
    # the matrix is the composition of the raw draws, flips included
    rp = p[:, :9].reshape(b, 3, 3).numpy()
    assert np.abs(rp - aug.compose_reference(p.numpy())).max() <= 1e-12
    det = np.linalg.det(rp)
    flips = (p[:, 18:21].numpy() < np.array(ALL_ON['flip_prob'])).sum(axis=1)
    assert np.abs(det - (-1.0) ** flips).max() <= 1e-12


def test_per_point_draws_ranges_and_distributions(hip):
    b, c, n = 2, 9, 65536
    sigma, clip = 0.01, 0.015
    aug = Augment.s3dis(jitter_sigma=sigma, jitter_clip=clip, dropout_max=0.875)
    x = torch.zeros((b, c, n), dtype=torch.float32, device=DEV)
    x[:, 3:] = torch.from_numpy(np.random.RandomState(SEED + 5).randn(b, c - 3, n).astype(np.float32)).to(DEV)
    y = torch.arange(n, device=DEV).repeat(b, 1)
    (got_x, got_y), draws = aug.augment(x, y, seed=seed_words(SEED, 13), return_draws=True)
    (same_x, _), same = aug.augment(x, y, seed=seed_words(SEED, 13), return_draws=True)
    (other_x, _), other = aug.augment(x, y, seed=seed_words(SEED, 14), return_draws=True)
    assert torch.equal(got_x, same_x) and all(torch.equal(draws[k], same[k]) for k in draws)
    assert not torch.equal(got_x, other_x) and not any(torch.equal(draws[k], other[k]) for k in draws)
    z, u, ratio = draws['jitter'], draws['keep'], draws['params'][:, 13]
    assert not torch.equal(z[0], z[1]) and not torch.equal(z[:, 0], z[:, 1]) and not torch.equal(u[0], u[1])
    check_moments('jitter normals', z, 0.0, 1.0, 3.0)
    check_uniform('keep uniforms', u, 0.0, 1.0)
    assert u.max().item() < 1.0
    dropped = u.double() <= ratio[:, None]
    dropped[:, 0] = False
    for i in range(b):                                                                  # a point is dropped with probability ratio (+ 2^-24)
        r, freq = ratio[i].item(), dropped[i].double().mean().item()
        print(f'cloud {i}: ratio {r:.4f} dropped {freq:.4f}')
        assert 0.0 < r < 0.875 and abs(freq - r) <= 6 * math.sqrt(r * (1 - r) / n) + 1 / n
    # what the points carry: the rotation, scale and translation are off and the coordinates are zero, so channels 0..2 ARE the jitter
    j = got_x[:, :3]
    bound = float(np.float32(clip))
    assert j.abs().max().item() <= bound and (j == bound).any() and (j == -bound).any()
    want_j = (sigma * z.double()).clamp(-clip, clip).float()
    kept = ~dropped[:, None, :].expand(b, 3, n)
    assert torch.equal(j[kept], want_j[kept])
    check_moments('jitter of the kept points', j[kept], 0.0, *clipped_normal_moments(sigma, clip))
    # a dropped point is point 0: every channel, the jitter, the target
    assert torch.equal(got_x, torch.where(dropped[:, None, :], got_x[:, :, :1], torch.cat([want_j, x[:, 3:]], dim=1)))
    assert torch.equal(got_y, torch.where(dropped, torch.zeros_like(y), y))
    assert dropped.any(dim=1).all() and not torch.equal(got_x[:, 3:], x[:, 3:])


# ------------------------------------------------------------------------------------------------------------ 5. loader, graphs
def s3dis_loader(augment, batch_size=4, num_points=512):
    from pvcnn_amd.data import DeviceLoader
    rng = np.random.RandomState(SEED)
    store = indexed_s3dis(rng.randint(600, 1200, size=12).tolist(), num_points)
    return store, DeviceLoader(store, batch_size, shuffle=True, drop_last=True, augment=augment)


def captured(fn):
    """fn once on a side stream (the warm-up torch asks for), then captured; -> the graph."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def test_captured_feed_augments_without_synchronisation(hip):
    aug = Augment.s3dis(**ALL_ON)
    store, loader = s3dis_loader(aug)
    x, y = loader.static_batch()
    graph = captured(loader.feed)                                                       # a synchronisation would fail the capture
    seen = []
    loader.cursor.zero_()
    for k in range(3):
        graph.replay()
        assert loader.cursor.item() == 4 * (k + 1)                                      # the cursor advances by B per replay
        seen.append((x.clone(), y.clone()))
    loader.cursor.zero_()
    graph.replay()                                                                      # the same items again: fresh draws
    assert not torch.equal(x, seen[0][0]) and not any(torch.equal(seen[0][0], s[0]) for s in seen[1:])
    # pinned seed words: the replay is the eager call, which is the plain assembly augmented with the same words
    pinned = captured(lambda: loader.feed(seed=loader.seed))
    words = seed_words(SEED, 21)
    loader.seed.copy_(words)
    loader.cursor.zero_()
    pinned.replay()
    got = (x.clone(), y.clone())
    assert loader.cursor.item() == 4 and torch.equal(loader.seed, words)
    loader.cursor.zero_()
    x.zero_(); y.zero_()
    out = loader.feed(seed=words)
    assert out[0] is x and out[1] is y and equal_batches(out, got)
    plain = store.assemble(None, seed=words, order=loader.order, cursor=torch.zeros(1, dtype=torch.int64, device=DEV), batch_size=4)
    assert equal_batches(aug.augment(plain[0], plain[1], seed=words), got) and not torch.equal(plain[0][:, :3], got[0][:, :3])
    assert torch.equal(plain[0][:, 3:, 0], got[0][:, 3:, 0])                            # the other channels pass through (point 0 is never dropped)
    # torch.manual_seed governs the words
    for _ in range(2):
        loader.cursor.zero_()
        torch.manual_seed(5)
        seen.append(tuple(t.clone() for t in loader.feed()))
    assert equal_batches(seen[-1], seen[-2])
    # ragged epochs go through __iter__
    from pvcnn_amd.data import DeviceLoader
    shapes = [(bx.shape, by.shape) for bx, by in DeviceLoader(store, 5, drop_last=False, augment=aug)]
    assert shapes == [((5, 9, 512), (5, 512)), ((5, 9, 512), (5, 512)), ((2, 9, 512), (2, 512))]


def test_graphed_train_step_feeds_and_augments_itself(hip):
    """The reduced-width PVCNN of test_gpu_data.py::test_graphed_train_step_feeds_itself, its batches augmented inside the graph."""
    from pvcnn_amd import workload
    from pvcnn_amd.data import DeviceLoader
    from pvcnn_amd.dp import GradBucketReducer
    from pvcnn_amd.graph import GraphedTrainStep
    from pvcnn_amd.optim import FlatAdam
    torch.manual_seed(0)
    rng = np.random.RandomState(SEED)
    store = indexed_s3dis(rng.randint(2048, 3000, size=8).tolist(), 2048)
    store.rows[:, 0] = store.rows[:, 1] * 1.5                                           # plausible coordinates in channel 0 as well
    model = workload.PVCNN(13, 6, width_multiplier=0.25).to(DEV).train()
    loader = DeviceLoader(store, 2, shuffle=False, drop_last=True,
                          augment=Augment.s3dis(rotate_max=math.pi, scale=(0.9, 1.1), jitter_sigma=0.01, jitter_clip=0.05, dropout_max=0.5))
    loader.order = torch.tensor([0, 1] * 4 + [2, 3, 4, 5, 6, 7], dtype=torch.int64, device=DEV)

    def fed_loss():
        x, y = loader.feed()
        return tf.cross_entropy(model(x), y)
    red = GradBucketReducer(model)
    step = GraphedTrainStep(model, fed_loss, FlatAdam(red, lr=2e-3, weight_decay=1e-5), red, warmup=3)
    assert step.graph is not None
    loader.cursor.fill_(8)
    losses = [step().item() for _ in range(3)]
    print('losses of three captured, augmented steps', losses)
    assert loader.cursor.item() == 14 and all(math.isfinite(v) for v in losses)


# -------------------------------------------------------------------------------------------------------- 6. unchanged behaviour
def test_a_loader_without_augment_is_the_plain_assembly(hip):
    from pvcnn_amd.data import DeviceLoader, DeviceShapeNet
    rng = np.random.RandomState(SEED)
    clouds = [np.concatenate([rng.randn(n, 6), rng.randint(0, 50, size=(n, 1))], axis=1) for n in rng.randint(300, 600, size=10)]
    shapenet = DeviceShapeNet(clouds, rng.randint(0, 16, size=10).tolist(), 256, device=DEV)
    for store in (s3dis_loader(None)[0], shapenet):
        loader = DeviceLoader(store, 4, shuffle=True, drop_last=True)
        assert loader.augment is None
        for k in range(2):
            words = seed_words(SEED + k, 31)
            got = tuple(t.clone() for t in loader.feed(seed=words))
            want = store.assemble(None, seed=words, order=loader.order, cursor=torch.tensor([4 * k], device=DEV), batch_size=4)
            assert equal_batches(got, want) and loader.cursor.item() == 4 * (k + 1)
        loader.cursor.zero_()
        torch.manual_seed(9)
        got = tuple(t.clone() for t in loader.feed())
        torch.manual_seed(9)
        words = torch.zeros(2, dtype=torch.int64, device=DEV).random_(0, 2 ** 62)       # what feed() draws
        assert equal_batches(got, store.assemble(None, seed=words, order=loader.order, cursor=None, batch_size=4))


# ------------------------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_write_nothing(hip):
    rng = np.random.RandomState(SEED + 6)
    x, y = (t.to(DEV) for t in batch(rng, 2, 9, 64))
    before_x, before_y = x.clone(), y.clone()
    out, out_y = torch.full_like(x, 7.0), torch.full_like(y, -7)
    drop = Augment.s3dis(dropout_max=0.5)
    params, jitter, keep = numpy_draws(rng, drop, 2, 64)
    with pytest.raises((RuntimeError, ValueError)):                                     # aliased with dropout on
        drop.augment(x, y, out=x, out_targets=out_y, params=params, keep=keep)
    with pytest.raises((RuntimeError, ValueError)):
        drop.augment(x, y, out=out, out_targets=y, seed=seed_words(1, 2))
    flat = torch.zeros(2 * 9 * 64 + 128, dtype=torch.float32, device=DEV)
    flat[:2 * 9 * 64] = x.flatten()
    lo, hi = flat[:2 * 9 * 64].view(2, 9, 64), flat[128:].view(2, 9, 64)               # overlapping, not the same view
    flat_before = flat.clone()
    for aug in (drop, Augment.s3dis(scale=(0.5, 2.0))):
        with pytest.raises((RuntimeError, ValueError), match='overlaps'):
            aug.augment(lo, out=hi, params=params, keep=keep)
    assert torch.equal(flat, flat_before)
    with pytest.raises((RuntimeError, ValueError), match='channels 7..9'):              # a triple that runs past C
        Augment(layout=[('position', 7)]).augment(x, y, out=out, out_targets=out_y)
    with pytest.raises((RuntimeError, ValueError), match='params of shape'):            # params of the wrong shape
        drop.augment(x, y, out=out, out_targets=out_y, params=params[:, :12], keep=keep)
    with pytest.raises((RuntimeError, ValueError), match='params of shape'):
        drop.augment(x, y, out=out, out_targets=out_y, params=params[:1], keep=keep)
    with pytest.raises((RuntimeError, ValueError), match='`keep`'):                     # a stage without its draws
        drop.augment(x, y, out=out, out_targets=out_y, params=params)
    with pytest.raises((RuntimeError, ValueError)):                                     # seed words on the host
        drop.augment(x, y, out=out, out_targets=out_y, seed=torch.zeros(2, dtype=torch.int64))
    with pytest.raises((RuntimeError, ValueError)):                                     # a transposed view: samples not contiguous
        Augment.s3dis().augment(x.permute(0, 2, 1).contiguous().permute(0, 2, 1), out=out)
    torch.cuda.synchronize()
    assert torch.equal(x, before_x) and torch.equal(y, before_y)
    assert (out == 7.0).all() and (out_y == -7).all()
