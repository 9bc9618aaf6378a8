"""The KITTI frame stage (pvcnn_amd.frames, csrc/frames.hip) at a real frame's size against numpy on the same machine's host.

    python tools/frames_bench.py [--points 120000] [--boxes 16] [--num-points 1024] [--iters 200] [--rounds 3]

A seeded synthetic frame (1242 x 375 image, a KITTI calibration, `--points` scan points in the sweep's range, `--boxes` 2-D boxes of
60 .. 300 px that hold points).  Measured, every shape warmed up first, `--rounds` rounds each so that the spread is on the table:
  * frame_batch eager: `--iters` calls between two device events, and the same calls on the host clock ending in a synchronise (the
    host's cost per launch is in the second and not in the first where the device runs ahead);
  * frame_batch replayed from a captured graph (static scan buffer, count word, box table, outputs): between two device events;
  * extract_frustums (rgb-detection form and ground-truth form): host clock around calls that end in their own device-to-host copy;
  * the numpy truth (tests/frames_truth.py: `batch` and `extract` on the same frame): host clock, 3 calls.
With each: native calls (through backend._run) and kernel launches per call.  One JSON line per measurement; the outputs of the device
path are compared with the truth's before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import frames_truth as ft                                               # noqa: E402
from pvcnn_amd import frames                                            # noqa: E402

SIZE = (1242, 375)
P = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
R0 = np.array([[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459], [0.007402527, 0.004351614, 0.9999631]])
V2C = np.array([[0.007533745, -0.9999714, -0.000616602, -0.004069766], [0.01480249, 0.0007280733, -0.9998902, -0.07631618],
                [0.9998621, 0.00752379, 0.01480755, -0.2717806]])
KERNELS = {'frame_project': 1, 'frame_count': 2, 'frame_pack': 1, 'frame_batch': 1, 'frame_rotate_rows': 1}


def make_frame(n, m, seed=1588147245):
    rng = np.random.RandomState(seed)
    scan = (rng.rand(n, 4) * [140, 100, 3.5, 1] + [-70, -50, -2.5, 0]).astype(np.float32)      # a full sweep: half of it behind the camera
    boxes = np.zeros((m, 4))
    for i in range(m):
        w, h = rng.uniform(60, 300), rng.uniform(60, 200)
        x0, y0 = rng.uniform(0, SIZE[0] - w), rng.uniform(100, SIZE[1] - h)
        boxes[i] = [x0, y0, x0 + w, y0 + h]
    rows, uv, seen = ft.project(scan, P, R0, V2C, SIZE)
    boxes_3d = np.zeros((m, 7))
    for i in range(m):
        sel = np.nonzero(ft.in_box(uv, seen, boxes[i]))[0]
        c = rows[sel[len(sel) // 2], :3].astype(np.float64)
        boxes_3d[i] = [1.6, 1.7, 4.0, c[0], c[1] + 0.8, c[2], rng.uniform(-np.pi, np.pi)]
    return scan, boxes, boxes_3d, rng.randint(0, 3, size=m), rng.rand(m)


def between_events(fn, n):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1000 / n


def host_clock(fn, n, sync=True):
    if sync:
        torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e6 / n


def launches(fn):
    calls = []
    from pvcnn_amd.modules.functional import backend as seam          # every native call of the frame stage goes through its _run
    orig = seam._run
    seam._run = lambda f, label, *a: (calls.append(label), orig(f, label, *a))[1]
    try:
        fn()
    finally:
        seam._run = orig
    return {'native_calls': len(calls), 'kernel_launches': sum(KERNELS[c] for c in calls)}


def report(name, times, extra):
    print(json.dumps({'measurement': name, 'us_per_call': [round(t, 1) for t in times], 'us_median': round(sorted(times)[len(times) // 2], 1),
                      **extra}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--boxes', type=int, default=16)
    ap.add_argument('--num-points', type=int, default=1024)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('frames_bench needs a GPU: nothing is measured on the host alone')
    dev = torch.device('cuda:0')
    scan, boxes, boxes_3d, class_ids, scores = make_frame(a.points, a.boxes)
    calib = frames.Calibration(P, R0, V2C)
    shape = {'points': a.points, 'boxes': a.boxes, 'num_points': a.num_points, 'device': torch.cuda.get_device_name(0)}
    classes = [('Car', 'Pedestrian', 'Cyclist')[i] for i in class_ids]

    # results first: parity batch and both extractions against the truth
    counts = ft.extract(scan, P, R0, V2C, boxes, SIZE)['counts'][:, 0]
    rng = np.random.RandomState(3)
    ch = np.stack([rng.choice(max(int(k), 1), a.num_points) for k in counts]).astype(np.int32)
    want = ft.batch(scan, P, R0, V2C, boxes, SIZE, class_ids, scores, ch, a.num_points)
    got = frames.frame_batch(scan, calib, boxes, SIZE, class_ids, scores=scores, num_points=a.num_points, choices=ch)
    ok = np.array_equal(got[0]['features'].cpu().numpy(), want[0]) and np.array_equal(got[2].cpu().numpy(), want[4])
    for b3 in (None, boxes_3d):
        t = ft.extract(scan, P, R0, V2C, boxes, SIZE, boxes_3d=b3)
        g = frames.extract_frustums(scan, calib, boxes, SIZE, classes=classes, boxes_3d=b3)
        ok = ok and np.array_equal(g.rows.cpu().numpy(), t['rows']) and np.array_equal(g.kept.cpu().numpy(), t['kept'])
        ok = ok and (b3 is None or np.array_equal(g.labels.cpu().numpy(), t['labels']))
    print(json.dumps({'measurement': 'equal_to_the_truth', 'ok': bool(ok), 'selected_per_box': counts.tolist(), **shape}), flush=True)
    if not ok:
        raise SystemExit('the device path differs from the truth: nothing is timed')

    x = torch.from_numpy(scan).to(dev)
    table = torch.from_numpy(frames.box_table(calib, boxes, class_ids, scores)).to(dev)
    count = torch.tensor([a.points], dtype=torch.int32, device=dev)
    seed = torch.tensor([11, 5], dtype=torch.int64, device=dev)
    kw = dict(num_points=a.num_points, seed=seed, count=count)
    out = frames.frame_batch(x, calib, table, SIZE, **kw)

    def eager():
        frames.frame_batch(x, calib, table, SIZE, out=out, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            eager()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eager()
    for _ in range(10):
        eager()
        graph.replay()
    n_batch = launches(eager)
    report('frame_batch_eager_device_events', [between_events(eager, a.iters) for _ in range(a.rounds)], {**n_batch, **shape})
    report('frame_batch_eager_host_clock', [host_clock(eager, a.iters) for _ in range(a.rounds)], {**n_batch, **shape})
    report('frame_batch_graph_replay_device_events', [between_events(graph.replay, a.iters) for _ in range(a.rounds)],
           {'graph_launches': 1, 'kernel_launches': n_batch['kernel_launches'], **shape})

    for name, b3 in (('extract_frustums_rgb_detection', None), ('extract_frustums_ground_truth', boxes_3d)):
        def extract():
            frames.extract_frustums(x, calib, boxes, SIZE, classes=classes, boxes_3d=b3)
        for _ in range(5):
            extract()
        report(name + '_host_clock', [host_clock(extract, max(a.iters // 4, 1)) for _ in range(a.rounds)],
               {**launches(extract), 'device_to_host_copies': 1, **shape})

    host = {'host_cpus_visible': os.cpu_count(), 'numpy': np.__version__}
    report('numpy_truth_batch_host_clock', [host_clock(lambda: ft.batch(scan, P, R0, V2C, boxes, SIZE, class_ids, scores, ch, a.num_points), 3,
                                                       sync=False) for _ in range(a.rounds)], {**host, **shape})
    report('numpy_truth_extract_host_clock', [host_clock(lambda: ft.extract(scan, P, R0, V2C, boxes, SIZE), 3, sync=False)
                                              for _ in range(a.rounds)], {**host, **shape})


if __name__ == '__main__':
    main()
