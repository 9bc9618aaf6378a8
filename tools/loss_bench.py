"""The segmentation criterion: torch.nn.functional.cross_entropy against PF.cross_entropy (csrc/xent.hip).

    python tools/loss_bench.py [--iters 200] [--steps 20] [--rounds 3] [--skip-step]

Same process, same call, the two criteria ALTERNATING round by round; every shape is warmed up first; a round is timed between two
device events.  torch's criterion is timed `--rounds` times so that its own spread is on the table: the fused one counts as faster
only where every one of its rounds beats every one of torch's by more than that spread.  Two measurements:
  * forward + backward of the criterion alone at the S3DIS, ShapeNet and Frustum-mask shapes, replayed from a captured hipGraph
    (what a GraphedTrainStep pays: device time and launch boundaries) and issued eagerly (which adds the host's cost per launch),
    with the launches per forward + backward: the kernels torch.profiler sees on the device, and for the fused criterion also the
    native calls through backend._run;
  * the cfg2 training step (PVCNN 1xC, B=16, N=4096, FlatAdam) replayed from its graph with each criterion inside.
One JSON line per measurement."""
import argparse
import copy
import json
import os
import sys

import torch
import torch.nn.functional as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pvcnn_amd import workload                                          # noqa: E402
import pvcnn_amd.modules.functional as PF                               # noqa: E402
from pvcnn_amd.modules.functional import backend as seam                # noqa: E402

SHAPES = [(16, 13, 4096), (8, 50, 2048), (32, 2, 1024)]
ARMS = (('torch', tf.cross_entropy), ('fused', PF.cross_entropy))


def between_events(fn, n):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / n


def verdict(base, new):
    spread = max(base) - min(base)
    return {'torch_spread': round(spread, 4), 'gain_median': round(sorted(base)[len(base) // 2] - sorted(new)[len(new) // 2], 4),
            'faster_in_every_round_by_more_than_the_spread': bool(min(base) - max(new) > spread)}


def device_kernels(fn):
    """Kernels one call of fn launches, as torch.profiler sees them on the device (None where the profiler gives no device events)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                 and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower()]
        return names or None
    except Exception:                                                    # noqa: BLE001 -- the count is then reported as not measured
        return None


def native_calls(fn):
    labels, run = [], seam._run

    def logged(f, label, ref, *args):
        labels.append(label)
        return run(f, label, ref, *args)
    seam._run = logged
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        seam._run = run
    return labels


def criterion_alone(shape, args, dev):
    b, c, s = shape
    g = torch.Generator().manual_seed(0)
    x = (4.0 * torch.randn(b, c, s, generator=g)).to(dev).requires_grad_()
    y = torch.randint(0, c, (b, s), generator=g).to(dev)
    assert PF.cross_entropy_is_fused(x, y)

    def once(fn):
        x.grad = None
        fn(x, y).backward()
    graphs = {}
    for name, fn in ARMS:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                once(fn)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            once(fn)
    for name, fn in ARMS:                                                # warm both modes of both arms
        between_events(lambda: once(fn), 20)
        between_events(graphs[name].replay, 20)
    us = {f'{name}_{mode}': [] for name, _ in ARMS for mode in ('replay', 'eager')}
    for _ in range(args.rounds):
        for name, fn in ARMS:
            us[f'{name}_replay'].append(1e3 * between_events(graphs[name].replay, args.iters))
        for name, fn in ARMS:
            us[f'{name}_eager'].append(1e3 * between_events(lambda: once(fn), args.iters))
    kernels = {name: device_kernels(lambda: once(fn)) for name, fn in ARMS}
    out = {'measurement': 'criterion forward + backward', 'shape': list(shape), 'iters_per_round': args.iters, 'rounds': args.rounds,
           'device': torch.cuda.get_device_name(0), 'unit': 'us per forward + backward'}
    out.update({k: [round(v, 3) for v in vs] for k, vs in us.items()})
    out['replay'] = verdict(us['torch_replay'], us['fused_replay'])
    out['eager'] = verdict(us['torch_eager'], us['fused_eager'])
    for name, _ in ARMS:
        out[f'{name}_device_kernels'] = None if kernels[name] is None else len(kernels[name])
        out[f'{name}_device_kernel_names'] = None if kernels[name] is None else sorted(set(n[:60] for n in kernels[name]))
    out['fused_native_calls'] = native_calls(lambda: once(PF.cross_entropy))
    return out


def replayed_step(args, dev):
    from pvcnn_amd.dp import GradBucketReducer
    from pvcnn_amd.graph import GraphedTrainStep
    from pvcnn_amd.optim import FlatAdam
    torch.manual_seed(0)
    base = workload.PVCNN(13, 6, width_multiplier=1).to(dev).train()
    x, y = workload.make_s3dis_batch(16, 4096, device=dev, seed=workload.SEED)
    steps, losses = {}, {}
    for name, fn in ARMS:
        model = copy.deepcopy(base)
        reducer = GradBucketReducer(model)
        opt = FlatAdam(reducer, lr=1e-3, weight_decay=1e-5)
        steps[name] = GraphedTrainStep(model, (lambda m, f: lambda: f(m(x), y))(model, fn), opt, reducer, warmup=3)
        assert steps[name].mode == 'graph'
        between_events(steps[name], 5)
    ms = {name: [] for name, _ in ARMS}
    for _ in range(args.rounds):
        for name, _ in ARMS:
            ms[name].append(between_events(steps[name], args.steps))
            losses[name] = steps[name].loss.item()
    out = {'measurement': 'cfg2 step replayed from its graph (PVCNN 1xC, B=16, N=4096, FlatAdam)', 'steps_per_round': args.steps,
           'rounds': args.rounds, 'device': torch.cuda.get_device_name(0), 'unit': 'ms per step',
           'torch': [round(v, 4) for v in ms['torch']], 'fused': [round(v, 4) for v in ms['fused']], 'last_loss': losses}
    out.update(verdict(ms['torch'], ms['fused']))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200, help='criterion forward + backward passes per round')
    ap.add_argument('--steps', type=int, default=20, help='replayed training steps per round')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--skip-step', action='store_true', help='the criterion alone, without the cfg2 step')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'loss_bench needs a GPU'
    dev = torch.device('cuda:0')
    for shape in SHAPES:
        print(json.dumps(criterion_alone(shape, args, dev)), flush=True)
    if not args.skip_step:
        print(json.dumps(replayed_step(args, dev)), flush=True)


if __name__ == '__main__':
    main()
