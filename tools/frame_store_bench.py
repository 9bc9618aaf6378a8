#!/usr/bin/env python3
"""Measure the Frustum-KITTI batch cut out of the frames (pvcnn_amd/frame_store.py) against the packed store's batch (pvcnn_amd/data.py).

  python tools/frame_store_bench.py alone    # 1. a replayed graph of feed() + cursor reset, us per batch, both stores interleaved
  python tools/frame_store_bench.py step     # 2. same-call A/B/C: the captured cfg5 step with static inputs, the packed store's
                                             #    feed() and the frame store's feed() inside

Synthetic frames of about 20 k in-image points (the test suite's image, calibration and point distribution), `--objects` objects each;
both stores are built from the same frames, B = 32, num_points = 1024, flip, shift and frustum rotation on, device mode.  Every figure
is the median of `--rounds` timed runs of `--iters` replays between two events, after a warm-up; one JSON line each.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 1588147245
SIZE = (1242, 375)
P = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
R0 = np.array([[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459], [0.007402527, 0.004351614, 0.9999631]])
V2C = np.array([[0.007533745, -0.9999714, -0.000616602, -0.004069766], [0.01480249, 0.0007280733, -0.9998902, -0.07631618],
                [0.9998621, 0.00752379, 0.01480755, -0.2717806]])
NAMES = ('Car', 'Pedestrian', 'Cyclist')
TEMPLATES = {'Car': np.array([3.9, 1.6, 1.56]), 'Pedestrian': np.array([0.8, 0.6, 1.73]), 'Cyclist': np.array([1.76, 0.6, 1.73])}
TEMPLATE_IDS = {'Car': 0, 'Pedestrian': 3, 'Cyclist': 5}


def synthetic_stores(args, device):
    """(DeviceKittiFrames, DeviceFrustumKitti) over the same frames; the objects sit around points of the sweep."""
    import torch
    from pvcnn_amd import frames
    from pvcnn_amd.data import DeviceFrustumKitti
    from pvcnn_amd.frame_store import DeviceKittiFrames
    calib = frames.Calibration(P, R0, V2C)
    options = dict(class_name_to_size_template_id=TEMPLATE_IDS, size_templates=TEMPLATES, random_flip=True, random_shift=True,
                   frustum_rotate=True)
    store = DeviceKittiFrames(None, args.points, **options)
    packed, in_image = [], []
    for f in range(args.frames):
        rng = np.random.RandomState(SEED + f)
        scan = (rng.rand(args.scan, 4) * [65, 50, 3.5, 1] + [-5, -25, -2.5, 0]).astype(np.float32)
        dev_scan = torch.from_numpy(scan).to(device)
        rows, uv, seen = (t.cpu().numpy() for t in frames.project_scan(dev_scan, calib, SIZE))
        inside = np.nonzero(seen)[0]
        in_image.append(len(inside))
        boxes, boxes_3d, names = [], [], []
        for i in range(args.objects):
            j = inside[rng.randint(len(inside))]
            (u, v), (x, y, z) = uv[j], rows[j, :3].astype(np.float64)
            boxes.append([u - 75, v - 50, u + 75, v + 50])
            boxes_3d.append([1.6, 1.7, 4.0, x, y + 0.8, z, rng.uniform(-np.pi, np.pi)])
            names.append(NAMES[i % 3])
        store.add_frame(dev_scan, calib, SIZE, boxes, boxes_3d, names)
        packed.append(frames.extract_frustums(dev_scan, calib, boxes, SIZE, classes=names, boxes_3d=boxes_3d))
    packed = DeviceFrustumKitti.from_frustums(packed, args.points, classes=NAMES, **options)
    assert len(packed) == len(store)
    counts = (packed.offsets[1:] - packed.offsets[:-1]).cpu().numpy()
    print(json.dumps({'what': 'stores', 'frames': args.frames, 'items': len(store), 'in_image_points_per_frame': int(np.mean(in_image)),
                      'points_per_frustum': int(counts.mean()), 'frame_store_bytes': store.nbytes, 'packed_store_bytes': packed.nbytes}))
    return store, packed


def time_launches(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def interleaved(fns, args):
    """name -> (median, min, max) us per call: `--rounds` rounds, every round times each of `fns` once, in turn."""
    import torch
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(args.rounds):
        for name, fn in fns.items():
            res[name].append(time_launches(fn, args.iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in res.items()}


def bench_alone(args):
    import torch
    from pvcnn_amd.data import DeviceLoader
    dev = torch.device('cuda:0')
    store, packed = synthetic_stores(args, dev)
    graphs = {}
    for name, s in (('packed', packed), ('frames', store)):
        loader = DeviceLoader(s, args.batch, shuffle=True, drop_last=True)
        loader.static_batch()
        loader.feed()
        loader.cursor.zero_()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()                      # as it runs inside a captured step: no Python between launches
        with torch.cuda.graph(graph):
            loader.feed()
            loader.cursor.zero_()
        graphs[name] = (graph, loader)
    res = interleaved({k: g.replay for k, (g, _) in graphs.items()}, args)
    used = store.draws(args.batch)[1].float().mean().item()
    walked = args.batch * store.largest_frame * 32
    print(json.dumps({'what': 'alone', 'batch': args.batch, 'points': args.points,
                      'us_packed': [round(v, 2) for v in res['packed']], 'us_frames': [round(v, 2) for v in res['frames']],
                      'delta_us': round(res['frames'][0] - res['packed'][0], 2), 'perturbed_boxes_accepted': round(used, 3),
                      'bytes_walked_per_batch': walked,
                      'note': 'graph of feed + cursor reset: includes the seed draw and two tiny torch launches; [median, min, max]'}))


def bench_step(args):
    import torch
    from pvcnn_amd import workload
    from pvcnn_amd.data import DeviceLoader
    from pvcnn_amd.dp import GradBucketReducer
    from pvcnn_amd.graph import GraphedTrainStep
    from pvcnn_amd.modules import FrustumPointNetLoss
    from pvcnn_amd.optim import FlatAdam
    dev = torch.device('cuda:0')
    store, packed = synthetic_stores(args, dev)
    templates = workload.frustum_size_templates()
    autocast = lambda: torch.autocast('cuda', dtype=torch.bfloat16)
    steps = {}
    for name, s in (('static', packed), ('packed', packed), ('frames', store)):
        loader = DeviceLoader(s, args.batch, shuffle=True, drop_last=True)
        x, y = loader.static_batch()
        loader.feed()
        loader.cursor.zero_()
        torch.manual_seed(0)
        model = workload.FrustumPVCNNE(3, 12, 8, 512, templates, 1, args.width).to(dev).train()
        criterion = FrustumPointNetLoss(12, 8, templates).to(dev)
        red = GradBucketReducer(model)

        def loss_fn(model=model, name=name, loader=loader, criterion=criterion, x=x, y=y):
            if name != 'static':
                loader.feed()
                loader.cursor.zero_()
            return criterion(model(x), y)
        steps[name] = GraphedTrainStep(model, loss_fn, FlatAdam(red, lr=1e-3, weight_decay=1e-5), red, autocast=autocast, warmup=3)
    res = interleaved(steps, args)
    med = {k: v[0] for k, v in res.items()}
    print(json.dumps({'what': 'step', 'config': 'cfg5', 'width': args.width, 'batch': args.batch, 'points': args.points,
                      'us_static': round(med['static'], 1), 'us_packed_feed': round(med['packed'], 1), 'us_frames_feed': round(med['frames'], 1),
                      'frames_minus_packed_us': round(med['frames'] - med['packed'], 1),
                      'frames_minus_packed_pct_of_step': round(100 * (med['frames'] - med['packed']) / med['packed'], 2),
                      'frames_minus_static_us': round(med['frames'] - med['static'], 1),
                      'ranges': {k: [round(v[1], 1), round(v[2], 1)] for k, v in res.items()}}))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['alone', 'step'])
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--points', type=int, default=1024)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--objects', type=int, default=8)
    ap.add_argument('--scan', type=int, default=34000, help='points per synthetic sweep (about 59 %% of them project into the image)')
    ap.add_argument('--width', type=float, default=1.0)
    a = ap.parse_args()
    {'alone': bench_alone, 'step': bench_step}[a.what](a)
