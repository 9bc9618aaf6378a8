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
One JSON line per measurement.

    python tools/loss_bench.py --dml [--dml-iters 2000] [--rounds 3]

The four terms of a deep-mutual-learning step (train_dml.py:125-137) at the recipe's shape, S3DIS B=16, C=13, N=4096, forward + both
backwards: (a) as before csrc/dml.hip -- modules.CrossEntropyLoss twice plus the torch kl_loss twice, in a fresh child process started
with PVCNN_FUSED_DML=0 -- against (b) modules.DMLPairLoss on the pair kernels in this process.  Both processes stay up and take their
rounds in turn (a, b, a, b, ...), each round replayed from a captured graph and issued eagerly, with the launches per pass.

    python tools/loss_bench.py --lovasz [--iters 200] [--steps 20] [--rounds 3] [--skip-step]

The Lovasz-Softmax criterion (csrc/lovasz.hip) against the batched torch composition of the same definition -- what every call the
kernels do not serve runs -- by the first method above (one process, alternating rounds, replayed and eager, launch counts) at the
S3DIS (16, 13, 4096), PVCNN++ (8, 13, 8192) and ShapeNet (8, 50, 2048) shapes; then the cfg2 step replayed from its graph with
modules.CrossEntropyLoss and with modules.CrossEntropyLovasz inside: what adding the IoU surrogate to the criterion costs a step."""
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
LOVASZ_SHAPES = [(16, 13, 4096), (8, 13, 8192), (8, 50, 2048)]


def between_events(fn, n):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / n


def verdict(base, new, name='torch'):
    spread = max(base) - min(base)
    return {f'{name}_spread': round(spread, 4), 'gain_median': round(sorted(base)[len(base) // 2] - sorted(new)[len(new) // 2], 4),
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
    from pvcnn_amd.modules.functional import loss as criteria
    labels, run = [], seam._run

    def logged(f, label, ref, *args):
        labels.append(label)
        return run(f, label, ref, *args)
    looked_up = criteria._native()                                       # (the criteria keep the seam they looked up once)
    seam._run, criteria._NATIVE = logged, (looked_up[0], logged, looked_up[2])
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        seam._run, criteria._NATIVE = run, looked_up
    return labels


def lovasz_arms():
    from pvcnn_amd.modules.functional import loss as criteria

    def composition(x, y):
        return criteria._lovasz_softmax(x, y, 'present', True, -100, False, None, False)
    return (('composition', composition), ('fused', PF.lovasz_softmax))


def criterion_alone(shape, args, dev, arms=ARMS, is_fused=PF.cross_entropy_is_fused):
    ARMS, (base, new) = arms, (arms[0][0], arms[1][0])
    b, c, s = shape
    g = torch.Generator().manual_seed(0)
    x = (4.0 * torch.randn(b, c, s, generator=g)).to(dev).requires_grad_()
    y = torch.randint(0, c, (b, s), generator=g).to(dev)
    assert is_fused(x, y)

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
    out['replay'] = verdict(us[f'{base}_replay'], us[f'{new}_replay'], base)
    out['eager'] = verdict(us[f'{base}_eager'], us[f'{new}_eager'], base)
    for name, _ in ARMS:
        out[f'{name}_device_kernels'] = None if kernels[name] is None else len(kernels[name])
        out[f'{name}_device_kernel_names'] = None if kernels[name] is None else sorted(set(n[:60] for n in kernels[name]))
    out[f'{new}_native_calls'] = native_calls(lambda: once(arms[1][1]))
    return out


def replayed_step(args, dev, arms=ARMS):
    ARMS, (base_arm, new_arm) = arms, (arms[0][0], arms[1][0])
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
           base_arm: [round(v, 4) for v in ms[base_arm]], new_arm: [round(v, 4) for v in ms[new_arm]], 'last_loss': losses}
    out.update(verdict(ms[base_arm], ms[new_arm], base_arm))
    return out


def _dml_arm(dev):
    """(once, graph, launch counts) of this process's arm: PVCNN_FUSED_DML=0 in the environment makes it the composed one."""
    import pvcnn_amd.modules as M
    from pvcnn_amd.modules.functional import loss as L
    b, c, s = SHAPES[0]
    g = torch.Generator().manual_seed(0)
    x0 = (4.0 * torch.randn(b, c, s, generator=g)).to(dev).requires_grad_()
    x1 = (4.0 * torch.randn(b, c, s, generator=g)).to(dev).requires_grad_()
    y = torch.randint(0, c, (b, s), generator=g).to(dev)
    if L.dml_enabled:
        pair = M.DMLPairLoss()
        assert PF.dml_pair_loss_is_fused(x0, x1, y)
    else:
        criterion, criterion_dml = M.CrossEntropyLoss(), M.KLLoss()
        assert PF.cross_entropy_is_fused(x0, y) and not PF.kl_loss_is_fused(x0, x1)

        def pair(outputs, outputs_student, targets):
            return (criterion(outputs, targets) + criterion_dml(outputs_student, outputs),
                    criterion(outputs_student, targets) + criterion_dml(outputs, outputs_student))

    def once():
        x0.grad = x1.grad = None
        loss, loss_student = pair(x0, x1, y)
        loss.backward()
        loss_student.backward()
        return loss, loss_student
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            once()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        losses = once()
    between_events(once, 500)
    between_events(graph.replay, 500)
    kernels = device_kernels(once)
    info = {'arm': 'fused' if L.dml_enabled else 'composed', 'device': torch.cuda.get_device_name(0),
            'device_kernels': None if kernels is None else len(kernels),
            'device_kernel_names': None if kernels is None else sorted(set(n[:60] for n in kernels)),
            'native_calls': native_calls(once), 'losses': [v.item() for v in losses]}
    return once, graph, info


def _dml_round(once, graph, iters):
    return {'replay': round(1e3 * between_events(graph.replay, iters), 3), 'eager': round(1e3 * between_events(once, iters), 3)}


def dml_child(args, dev):
    """The composed arm: set up, say so, then one round per line on stdin until it closes."""
    once, graph, info = _dml_arm(dev)
    print(json.dumps(info), flush=True)
    for _ in sys.stdin:
        print(json.dumps(_dml_round(once, graph, args.dml_iters)), flush=True)


def dml_pair(args, dev):
    import subprocess
    env = dict(os.environ, PVCNN_FUSED_DML='0')
    child = subprocess.Popen([sys.executable, os.path.abspath(__file__), '--dml-child', '--dml-iters', str(args.dml_iters)], env=env,
                             stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    try:
        base = json.loads(child.stdout.readline())
        once, graph, mine = _dml_arm(dev)
        assert base['arm'] == 'composed' and mine['arm'] == 'fused', (base['arm'], mine['arm'])
        rounds = {'composed': [], 'fused': []}
        for _ in range(args.rounds):
            child.stdin.write('round\n')
            child.stdin.flush()
            rounds['composed'].append(json.loads(child.stdout.readline()))
            rounds['fused'].append(_dml_round(once, graph, args.dml_iters))
    finally:
        child.stdin.close()
        child.wait(timeout=60)
    out = {'measurement': 'DML criterion pair, forward + both backwards', 'shape': list(SHAPES[0]), 'iters_per_round': args.dml_iters,
           'rounds': args.rounds, 'device': mine['device'], 'unit': 'us per forward + both backwards', 'composed': base, 'fused': mine}
    for mode in ('replay', 'eager'):
        a, b = [r[mode] for r in rounds['composed']], [r[mode] for r in rounds['fused']]
        spread = max(a) - min(a)
        out[mode] = {'composed': a, 'fused': b, 'composed_spread': round(spread, 3),
                     'gain_median': round(sorted(a)[len(a) // 2] - sorted(b)[len(b) // 2], 3),
                     'faster_in_every_round_by_more_than_the_spread': bool(min(a) - max(b) > spread)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200, help='criterion forward + backward passes per round')
    ap.add_argument('--steps', type=int, default=20, help='replayed training steps per round')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--skip-step', action='store_true', help='the criterion alone, without the cfg2 step')
    ap.add_argument('--dml', action='store_true', help='the deep-mutual-learning criterion pair only: composed (child process) against fused')
    ap.add_argument('--dml-iters', type=int, default=2000, help='DML forward + backward passes per round')
    ap.add_argument('--dml-child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--lovasz', action='store_true', help='the Lovasz-Softmax criterion: the torch composition against the fused kernels')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'loss_bench needs a GPU'
    dev = torch.device('cuda:0')
    if args.dml_child:
        return dml_child(args, dev)
    if args.dml:
        print(json.dumps(dml_pair(args, dev)), flush=True)
        return
    if args.lovasz:
        import pvcnn_amd.modules as M
        for shape in LOVASZ_SHAPES:
            print(json.dumps(criterion_alone(shape, args, dev, lovasz_arms(), PF.lovasz_softmax_is_fused)), flush=True)
        if not args.skip_step:
            print(json.dumps(replayed_step(args, dev, (('cross_entropy', M.CrossEntropyLoss()), ('cross_entropy_lovasz', M.CrossEntropyLovasz())))),
                  flush=True)
        return
    for shape in SHAPES:
        print(json.dumps(criterion_alone(shape, args, dev)), flush=True)
    if not args.skip_step:
        print(json.dumps(replayed_step(args, dev)), flush=True)


if __name__ == '__main__':
    main()
