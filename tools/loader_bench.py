#!/usr/bin/env python3
"""Measure the device-side batch assembly (pvcnn_amd/data.py) and, for scale, the host path it replaces.

  python tools/loader_bench.py assembly            # 1. the assembly launches alone, us per batch, three as-benched shapes, both modes
  python tools/loader_bench.py step                # 2. same-call A/B: captured PVCNN step with feed() inside vs static inputs
  python tools/loader_bench.py host [--procs 16]   # 3. numpy restatement of the three __getitem__ bodies + collate, items/s

Every GPU figure is the median of `--rounds` timed runs of `--iters` launches between two events, after a warm-up; one JSON line each.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 1588147245
HBM_BYTES_PER_S = 8e12


def synthetic_stores(device):
    import torch  # noqa: F401
    from pvcnn_amd.data import DeviceFrustumKitti, DeviceS3DIS, DeviceShapeNet
    rng = np.random.RandomState(SEED)
    n = rng.randint(4096, 8193, size=256)
    s3dis = DeviceS3DIS(rng.rand(256, 8192, 9).astype(np.float32), rng.randint(0, 13, size=(256, 8192)), n, 4096, device=device)
    counts = rng.randint(2000, 3000, size=256)
    shapenet = DeviceShapeNet([np.concatenate([rng.randn(c, 6), rng.randint(0, 50, size=(c, 1))], axis=1) for c in counts],
                              rng.randint(0, 16, size=256), 2048, device=device)
    counts = rng.randint(200, 3000, size=512)
    classes = ('Car', 'Pedestrian', 'Cyclist')
    frustum = DeviceFrustumKitti([rng.randn(c, 4).astype(np.float32) for c in counts], [rng.randint(0, 2, size=c) for c in counts],
                                 [rng.randn(8, 3) + [1, 1, 20] for _ in counts], [np.float64(h) for h in rng.uniform(-3, 3, size=512)],
                                 [rng.rand(3) + 1 for _ in counts], [classes[i % 3] for i in range(512)],
                                 [np.float64(a) for a in rng.uniform(-2, -1, size=512)], 1024, classes=classes,
                                 class_name_to_size_template_id={'Car': 0, 'Pedestrian': 3, 'Cyclist': 5},
                                 size_templates={c: rng.rand(3) + 1 for c in classes}, random_flip=True, random_shift=True,
                                 frustum_rotate=True, device=device)
    return {'s3dis': (s3dis, 16), 'shapenet': (shapenet, 8), 'frustum': (frustum, 32)}


def time_launches(fn, iters, rounds):
    import torch
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return statistics.median(out), min(out), max(out)


def batch_bytes(store, batch):
    flat = []
    for part in batch:
        flat += list(part.values()) if isinstance(part, dict) else [part]
    written = sum(t.numel() * t.element_size() for t in flat)
    rows = flat[0].shape[0] * store.num_points
    return written + rows * (store.channels * 4 + store._label_bytes())


def bench_assembly(args):
    import torch
    from pvcnn_amd.data import DeviceLoader
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(SEED)
    for name, (store, b) in synthetic_stores(dev).items():
        loader = DeviceLoader(store, b, shuffle=True, drop_last=True)
        out = loader.static_batch()
        n = store.num_points
        draws = {'choices': torch.from_numpy(rng.randint(0, 200, size=(b, n)).astype(np.int32)).to(dev)}
        if name == 'shapenet':
            draws['jitter'] = torch.from_numpy(rng.randn(b, 3, n)).to(dev)
        if name == 'frustum':
            draws['flip'], draws['shift'] = torch.from_numpy(rng.rand(b)).to(dev), torch.from_numpy(rng.randn(b)).to(dev)
        for mode, kw in (('device', {}), ('parity', draws)):
            graph = torch.cuda.CUDAGraph()                      # as it runs inside a captured step: no Python between launches
            loader.feed(**kw)
            torch.cuda.synchronize()
            with torch.cuda.graph(graph):
                loader.feed(**kw)
                loader.cursor.zero_()

            med, lo, hi = time_launches(graph.replay, args.iters, args.rounds)
            nbytes = batch_bytes(store, out)
            print(json.dumps({'what': 'assembly', 'dataset': name, 'mode': mode, 'batch': b, 'points': n, 'us_per_batch': round(med, 2),
                              'us_min': round(lo, 2), 'us_max': round(hi, 2), 'bytes': nbytes,
                              'fraction_of_8TBps': round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 4),
                              'note': 'graph of feed + cursor reset: includes the seed draw (device mode) and two tiny torch launches'}))


def bench_step(args):
    import torch
    import torch.nn.functional as tf
    from pvcnn_amd import workload
    from pvcnn_amd.data import DeviceLoader
    from pvcnn_amd.dp import GradBucketReducer
    from pvcnn_amd.graph import GraphedTrainStep
    from pvcnn_amd.optim import FlatAdam
    dev = torch.device('cuda:0')
    store, b = synthetic_stores(dev)['s3dis']
    loader = DeviceLoader(store, b, shuffle=True, drop_last=True)
    x, y = loader.static_batch()
    loader.feed()
    steps = {}
    for name in ('static', 'feed'):
        torch.manual_seed(0)
        model = workload.PVCNN(13, 6, width_multiplier=args.width).to(dev).train()
        red = GradBucketReducer(model)

        def loss_fn(model=model, name=name):
            if name == 'feed':
                loader.feed()
                loader.cursor.zero_()
            return tf.cross_entropy(model(x), y)
        steps[name] = GraphedTrainStep(model, loss_fn, FlatAdam(red, lr=1e-3), red)
    res = {k: [] for k in steps}
    for _ in range(args.rounds):                                # interleaved: same call, same box, same clocks
        for name, step in steps.items():
            res[name].append(time_launches(step, args.iters, 1)[0])
    med = {k: statistics.median(v) for k, v in res.items()}
    print(json.dumps({'what': 'step', 'width': args.width, 'batch': b, 'us_static': round(med['static'], 1), 'us_feed': round(med['feed'], 1),
                      'delta_us': round(med['feed'] - med['static'], 1), 'delta_pct': round(100 * (med['feed'] / med['static'] - 1), 2)}))


# ---- 3. the host path: the three __getitem__ bodies restated in numpy, plus the collate's stacking ----
def _host_worker(job):
    kind, items, seed = job
    rng = np.random.RandomState(seed)
    t0 = time.perf_counter()
    if kind == 's3dis':
        data, label = rng.rand(8192, 9).astype(np.float32), rng.randint(0, 13, size=8192)
        batch = []
        for _ in range(items):
            n = rng.randint(4096, 8193)
            ch = np.random.choice(n, 4096, replace=n < 4096)
            batch.append((data[ch, ...].transpose(), label[ch]))
            if len(batch) == 16:
                np.stack([b[0] for b in batch]); np.stack([b[1] for b in batch]); batch = []
    elif kind == 'shapenet':
        coords, normal, label = (rng.randn(2500, 3).astype(np.float32), rng.randn(2500, 3).astype(np.float32), rng.randint(0, 50, size=2500))
        batch = []
        for _ in range(items):
            ch = np.random.choice(2500, 2048, replace=True)
            c = coords[ch, :].transpose()
            c = np.clip(0.01 * np.random.randn(*c.shape), -0.05, 0.05).astype(np.float32) + c
            hot = np.zeros((16, 2048), dtype=np.float32)
            hot[3, :] = 1.0
            batch.append((np.concatenate([c, normal[ch, :].transpose(), hot]), label[ch].transpose()))
            if len(batch) == 8:
                np.stack([b[0] for b in batch]); np.stack([b[1] for b in batch]); batch = []
    else:
        cloud, mask = rng.randn(1500, 4).astype(np.float32), rng.randint(0, 2, size=1500)
        batch = []
        for _ in range(items):
            ang = np.pi / 2.0 + rng.uniform(-2, -1)
            pc = np.copy(cloud)
            pc[:, [0, 2]] = np.dot(pc[:, [0, 2]], [[np.cos(ang), np.sin(ang)], [-np.sin(ang), np.cos(ang)]])
            ch = np.random.choice(1500, 1024, replace=True)
            pc = pc[ch, :]
            if np.random.random() > 0.5:
                pc[:, 0] = -pc[:, 0]
            pc[:, 2] += np.clip(np.random.randn() * 20.0 * 0.05, 16.0, 24.0)
            batch.append((pc.astype(np.float32).T, mask[ch].astype(np.int64)))
            if len(batch) == 32:
                np.stack([b[0] for b in batch]); np.stack([b[1] for b in batch]); batch = []
    return time.perf_counter() - t0


def bench_host(args):
    import multiprocessing as mp
    with mp.get_context('spawn').Pool(args.procs) as pool:
        for kind in ('s3dis', 'shapenet', 'frustum'):
            pool.map(_host_worker, [(kind, 50, i) for i in range(args.procs)])                      # warm the workers
            t0 = time.perf_counter()
            pool.map(_host_worker, [(kind, args.items, i) for i in range(args.procs)])
            wall = time.perf_counter() - t0
            print(json.dumps({'what': 'host', 'dataset': kind, 'procs': args.procs, 'items_per_s': round(args.procs * args.items / wall, 1),
                              'note': 'numpy __getitem__ + stacking only: no pickling to the parent, no pin, no H2D copy'}))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['assembly', 'step', 'host'])
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--width', type=float, default=1.0)
    ap.add_argument('--procs', type=int, default=16)
    ap.add_argument('--items', type=int, default=4000)
    a = ap.parse_args()
    {'assembly': bench_assembly, 'step': bench_step, 'host': bench_host}[a.what](a)
