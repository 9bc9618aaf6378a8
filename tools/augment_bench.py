"""Time `DeviceLoader.feed()` with and without `augment=` on the device (profiles/augment.md is written from this tool's output).

Per workload (S3DIS B=16, C=9, N=4096; ShapeNet B=8, C=22, N=2048): 50 calls between two device events, three rounds, the two arms
alternating, eagerly and as replays of a captured graph; the draw and apply launches back to back, with the bytes the apply launch
moves; the kernels one `feed()` launches in each arm.  An optional argument, the path of an earlier revision's data.py, adds that
revision's loader as a third arm ('before').  Prints one JSON line per workload.  Needs a GPU: there is no CPU path to time.
Kernel durations come from a run of their own:  rocprofv3 --kernel-trace --stats -- python tools/augment_bench.py"""
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pvcnn_amd.augment import PARAMS, Augment                                   # noqa: E402
from pvcnn_amd.data import DeviceLoader, DeviceS3DIS, DeviceShapeNet            # noqa: E402

CALLS, ROUNDS, SEED = 50, 3, 1588147245
ALL_ON = dict(rotate_max=math.pi, perturb_sigma=0.06, perturb_clip=0.18, flip_prob=(0.5, 0.5, 0.0), scale=(0.8, 1.25), translate=0.2,
              jitter_sigma=0.01, jitter_clip=0.05, dropout_max=0.875)


def timed(fn, calls=CALLS):
    """Microseconds per call of `calls` calls between two device events."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls


def kernels_of(fn):
    """Names of the device kernels one call of fn launches (torch's profiler)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'Memcpy' not in e.name and 'Memset' not in e.name]
    return [name.split('(')[0].split('<')[0].replace('void ', '') for name in names]


def replayed(fn):
    """fn captured into a graph (after torch's side-stream warm-up) -> a function that replays it."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def workload(name, device):
    rng = np.random.RandomState(SEED)
    if name == 's3dis':
        counts = rng.randint(4096, 8193, size=32)
        p = int(counts.max())
        store = DeviceS3DIS(rng.rand(len(counts), p, 9).astype(np.float32), rng.randint(0, 13, size=(len(counts), p)), counts, 4096,
                            device=device)
        return store, 16, Augment.s3dis(**ALL_ON)
    counts = rng.randint(1500, 3000, size=32)
    clouds = [np.concatenate([rng.randn(n, 6), rng.randint(0, 50, size=(n, 1))], axis=1) for n in counts]
    return DeviceShapeNet(clouds, rng.randint(0, 16, size=len(counts)).tolist(), 2048, device=device), 8, Augment.shapenet(**ALL_ON)


def feeder(loader):
    def feed():
        loader.cursor.zero_()
        loader.feed()
    return feed


def main():
    if not torch.cuda.is_available():
        raise SystemExit('augment_bench needs a GPU')
    device = torch.device('cuda', 0)
    for name in ('s3dis', 'shapenet'):
        store, b, aug = workload(name, device)
        arms = {'plain': DeviceLoader(store, b, drop_last=True), 'augment': DeviceLoader(store, b, drop_last=True, augment=aug)}
        if len(sys.argv) > 1:                                                    # an earlier revision's data.py: its loader as a third arm
            import importlib.util
            spec = importlib.util.spec_from_file_location('pvcnn_amd._data_before', sys.argv[1])
            before = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(before)
            arms = {'before': before.DeviceLoader(store, b, drop_last=True), **arms}
        feeds = {k: feeder(v) for k, v in arms.items()}
        for fn in feeds.values():                                                # warm-up: code objects, the staging batch
            timed(fn, 10)
        rounds = {k: [] for k in feeds}
        for _ in range(ROUNDS):
            for k, fn in feeds.items():
                rounds[k].append(timed(fn))
        # the same calls captured: what a GraphedTrainStep replays (no host work between the launches)
        replays = {k: replayed(fn) for k, fn in feeds.items()}
        for fn in replays.values():
            timed(fn, 10)
        replay_rounds = {k: [] for k in replays}
        for _ in range(ROUNDS):
            for k, fn in replays.items():
                replay_rounds[k].append(timed(fn))
        # the apply launch alone, on the loader's own tensors
        loader = arms['augment']
        staging, out = loader._staging, loader.static_batch()
        params = aug.draw(b, loader.seed)
        apply = lambda: aug.augment(staging[0], staging[1], out=out[0], out_targets=out[1], seed=loader.seed, params_out=params)
        draw_and_apply = [timed(apply) for _ in range(ROUNDS)]
        draw_only = [timed(lambda: aug.draw(b, loader.seed, params)) for _ in range(ROUNDS)]
        _, c, n = out[0].shape
        moved = 2 * b * c * n * 4 + 2 * b * n * 8 + b * PARAMS * 8
        try:
            launched = {k: kernels_of(fn) for k, fn in feeds.items()}
        except Exception as exc:                                                 # the profiler is optional: say so instead of guessing
            launched = {'error': repr(exc)}
        apply_us = min(draw_and_apply) - min(draw_only)
        print(json.dumps({'workload': name, 'B': b, 'C': c, 'N': n, 'calls': CALLS, 'feed_us': rounds,
                          'added_us_per_call': [a - p for a, p in zip(rounds['augment'], rounds['plain'])],
                          'replay_us': replay_rounds,
                          'added_us_per_replay': [a - p for a, p in zip(replay_rounds['augment'], replay_rounds['plain'])],
                          'draw_and_apply_us': draw_and_apply, 'draw_us': draw_only, 'apply_bytes': moved,
                          'apply_us_back_to_back': apply_us, 'fraction_of_8TBps': moved / (apply_us * 1e-6) / 8e12 if apply_us > 0 else None,
                          'kernels_per_feed': launched}))


if __name__ == '__main__':
    main()
