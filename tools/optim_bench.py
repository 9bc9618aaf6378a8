"""The optimizer step alone, on the parameters of the benched cfg2 PVCNN with synthetic gradients, in us per step:

    python tools/optim_bench.py [--steps 50] [--rounds 3] [--warmup 10]

  a  FlatAdam, one group, no option: the one-group kernel (what bench.py's step runs)
  b  FlatAdam, two groups (weights with decay / BatchNorm and biases without): the grouped kernel
  c  b + max_grad_norm + skip_nonfinite: the norm pass in front of it
  d  what one writes without them: torch.nn.utils.clip_grad_norm_ + torch.optim.Adam(the same groups, capturable=True)

Same process, the candidates ALTERNATING round by round, every one warmed up first; a round is `--steps` optimizer steps between two
device events.  Two ways of issuing them: `eager` (one Python call per step: what an eager loop pays, host time included) and `graph`
(ONE step captured in a hipGraph and replayed `--steps` times: what a captured training step pays, since FlatAdam exists for those).
Candidate a is timed in every round so that its own spread is on the table.  Also printed: the native calls and kernel launches per
step of a, b and c (every entry point is one launch; the call of the last bucket launches the counter's increment as well).
One JSON line."""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pvcnn_amd import optim as flat_optim                               # noqa: E402
from pvcnn_amd import workload                                          # noqa: E402
from pvcnn_amd.dp import GradBucketReducer                              # noqa: E402
from pvcnn_amd.optim import FlatAdam                                    # noqa: E402

HYPER = dict(lr=1e-3, weight_decay=1e-5)
MAX_NORM = 1.0


def groups_of(model):
    params = list(model.parameters())
    return [dict(params=[p for p in params if p.dim() > 1]), dict(params=[p for p in params if p.dim() <= 1], weight_decay=0.0)]


def timed(step, steps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        step()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / steps


def captured(step, warmup):
    """One optimizer step as a graph -> its replay (None where the step cannot be captured)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph):
            step()
    except Exception as exc:                                            # noqa: BLE001 -- reported in the JSON line
        torch.cuda.synchronize()
        return None, f'{type(exc).__name__}: {str(exc)[:160]}'
    return graph.replay, None


def census(opt):
    labels = {}
    run = flat_optim._run

    def logged(fn, label, ref, *args):
        labels[label] = labels.get(label, 0) + 1
        return run(fn, label, ref, *args)
    flat_optim._run = logged
    try:
        opt.step()
        torch.cuda.synchronize()
    finally:
        flat_optim._run = run
    return labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'optim_bench needs a GPU'
    assert args.steps >= 50 and args.rounds >= 3, 'at least three rounds of 50 steps'
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    base = workload.PVCNN(13, 6, width_multiplier=1).to(dev)
    models = {k: copy.deepcopy(base) for k in 'abcd'}
    gen = torch.Generator(device=dev).manual_seed(1)
    grads = [torch.randn(p.shape, device=dev, generator=gen) * 1e-2 for p in base.parameters()]
    reds = {k: GradBucketReducer(models[k]) for k in 'abc'}
    opts = {'a': FlatAdam(reds['a'], **HYPER),
            'b': FlatAdam(reds['b'], param_groups=groups_of(models['b']), **HYPER),
            'c': FlatAdam(reds['c'], param_groups=groups_of(models['c']), max_grad_norm=MAX_NORM, skip_nonfinite=True, **HYPER)}
    for k in 'abc':                                                     # the gradients where reducer.finish() leaves them
        for p, g in zip(models[k].parameters(), grads):
            p.grad = g.clone()
        reds[k].finish()
    for p, g in zip(models['d'].parameters(), grads):
        p.grad = g.clone()
    torch_adam = torch.optim.Adam(groups_of(models['d']), capturable=True, **HYPER)
    params_d = list(models['d'].parameters())

    def step_d():
        torch.nn.utils.clip_grad_norm_(params_d, MAX_NORM)
        torch_adam.step()
    steps = {'a': opts['a'].step, 'b': opts['b'].step, 'c': opts['c'].step, 'd': step_d}
    out = {'device': torch.cuda.get_device_name(0), 'parameters': sum(p.numel() for p in base.parameters()),
           'tensors': len(grads), 'buckets': len(reds['a'].buckets), 'runs_per_bucket': [t.shape[0] for t in opts['b'].run_tables],
           'steps_per_round': args.steps, 'rounds': args.rounds}
    for mode in ('eager', 'graph'):
        calls, errors = {}, {}
        for k in 'abcd':
            if mode == 'eager':
                for _ in range(args.warmup):
                    steps[k]()
                calls[k] = steps[k]
            else:
                calls[k], err = captured(steps[k], 3)
                if err:
                    errors[k] = err
                else:
                    for _ in range(args.warmup):
                        calls[k]()
        torch.cuda.synchronize()
        us = {k: [] for k in 'abcd'}
        for _ in range(args.rounds):
            for k in 'abcd':
                if calls[k] is not None:
                    us[k].append(round(timed(calls[k], args.steps), 3))
        out[mode] = {'us_per_step': us, 'a_spread_us': round(max(us['a']) - min(us['a']), 3),
                     'b_minus_a_us_median': round(sorted(us['b'])[len(us['b']) // 2] - sorted(us['a'])[len(us['a']) // 2], 3),
                     'c_faster_than_d_in_every_round': bool(us['d']) and all(c < d for c, d in zip(us['c'], us['d']))}
        if errors:
            out[mode]['not_captured'] = errors
    for k in 'abc':
        labels = census(opts[k])
        out[f'native_calls_{k}'] = labels
        out[f'kernel_launches_{k}'] = sum(labels.values()) + 1          # + the step counter's increment behind the last bucket
    out['grad_norm_c'] = opts['c'].grad_norm.item()
    out['skipped_steps_c'] = opts['c'].skipped_steps.item()
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
