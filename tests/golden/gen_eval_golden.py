#!/usr/bin/env python3
"""Generate tests/golden/eval_votes.pt from the REFERENCE ITSELF (evaluation loops and meters), run where the reference tree is mounted.

Producers of the expected values:
  * evaluate/s3dis/eval.py     update_scene_predictions, update_stats
  * evaluate/shapenet/eval.py  update_shape_predictions, update_stats
  * meters/s3dis.py, meters/shapenet.py
imported from the reference tree.  Those eval functions are plain Python loops under @numba.jit(); numba is replaced by a stand-in
module whose jit() returns the function unchanged.  Nothing of pvcnn_amd takes part in producing the expected values.
Run:  python tests/golden/gen_eval_golden.py [reference root]     (rewrites eval_votes.pt)
"""
import importlib
import importlib.util
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
SEED = 1588147245


def _stand_in_numba():
    fake = types.ModuleType('numba')

    def jit(*args, **kwargs):
        if len(args) == 1 and callable(args[0]) and not kwargs:
            return args[0]
        return lambda f: f
    fake.jit = jit
    return fake


def load_reference():
    sys.modules.setdefault('numba', _stand_in_numba())
    mods = {}
    for name in ('s3dis', 'shapenet'):
        spec = importlib.util.spec_from_file_location(f'ref_eval_{name}', os.path.join(REF, 'evaluate', name, 'eval.py'))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        mods[f'eval_{name}'] = m
    sys.path.insert(0, REF)
    try:
        mods['meter_s3dis'] = importlib.import_module('meters.s3dis').MeterS3DIS
        mods['meter_shapenet'] = importlib.import_module('meters.shapenet').MeterShapeNet
    finally:
        sys.path.remove(REF)
    return types.SimpleNamespace(**mods)


def quantised_conf(rng, shape, levels=7):
    """confidences drawn from a few values: equal confidences inside a call and across calls; some 0 and some negative (never win)"""
    vals = np.array([0.0, -0.25, 0.125, 0.25, 0.5, 0.75, 1.0][:levels], dtype=np.float32)
    return vals[rng.randint(0, levels, size=shape)]


def s3dis_case(ref, rng, num_windows, max_points, num_points, scene_points, batch_size, num_classes, all_to_one=False):
    # windows overlap: each maps max_points slots onto the scene; some scene points are never mapped (they stay -1)
    scene_num_points = rng.randint(max_points // 2, max_points + 1, size=num_windows).astype(np.int64)
    covered = scene_points - max(1, scene_points // 10)
    mapping = rng.randint(0, covered, size=(num_windows, max_points)).astype(np.int64)
    if all_to_one:
        mapping[:] = 3
    extra = math.ceil(max_points / num_points)
    V = extra * num_points
    conf = np.zeros(scene_points, dtype=np.float32)
    pred = np.full(scene_points, -1, dtype=np.int64)
    calls = []
    for lo in range(0, num_windows, batch_size):
        hi = min(lo + batch_size, num_windows)
        bs = hi - lo
        shuffled = np.zeros((bs, V), dtype=np.int64)
        for r in range(bs):
            idx = np.tile(np.arange(scene_num_points[lo + r]), math.ceil(V / scene_num_points[lo + r]))[:V]
            rng.shuffle(idx)
            shuffled[r] = idx
        bc = quantised_conf(rng, (bs, V))
        bp = rng.randint(0, num_classes, size=(bs, V)).astype(np.int64)
        ref.eval_s3dis.update_scene_predictions(bc, bp, shuffled, conf, pred, mapping, V, bs, lo)
        calls.append(dict(conf=torch.from_numpy(bc), pred=torch.from_numpy(bp), shuffled=torch.from_numpy(shuffled), min_window_index=lo))
    gt = rng.randint(0, num_classes, size=scene_points).astype(np.int64)
    stats = np.zeros((3, num_classes, 2))
    ref.eval_s3dis.update_stats(stats, gt, pred, 1, scene_points)
    return dict(mapping=torch.from_numpy(mapping), scene_num_points=torch.from_numpy(scene_num_points), num_points=num_points,
                calls=calls, confidences=torch.from_numpy(conf), predictions=torch.from_numpy(pred), ground_truth=torch.from_numpy(gt),
                stats=torch.from_numpy(stats), num_classes=num_classes)


def shapenet_case(ref, rng, total_points, num_points, start_class, end_class, calls_n=2):
    conf = np.zeros(total_points, dtype=np.float32)
    pred = np.full(total_points, -1, dtype=np.int64)
    V = math.ceil(total_points / num_points) * num_points
    calls = []
    for _ in range(calls_n):
        idx = np.tile(np.arange(total_points), math.ceil(V / total_points))[:V]
        rng.shuffle(idx)
        vc = quantised_conf(rng, (V,))
        vp = rng.randint(start_class, end_class, size=V).astype(np.int64)
        ref.eval_shapenet.update_shape_predictions(vc, vp, idx, conf, pred, V)
        calls.append(dict(conf=torch.from_numpy(vc), pred=torch.from_numpy(vp), shuffled=torch.from_numpy(idx)))
    gt = rng.randint(start_class, end_class - 1, size=total_points).astype(np.int64)     # end_class - 1 absent from the target
    stats = np.zeros((4, 2))
    ref.eval_shapenet.update_stats(stats, gt, pred, 2, start_class, end_class)
    return dict(calls=calls, confidences=torch.from_numpy(conf), predictions=torch.from_numpy(pred), ground_truth=torch.from_numpy(gt),
                start_class=start_class, end_class=end_class, stats=torch.from_numpy(stats))


def tied_logits(gen, b, c, n):
    x = torch.randint(-3, 4, (b, c, n), generator=gen).float() * 0.5          # a handful of values: many exact ties in a column
    return x


def meter_s3dis_case(ref, gen, batches, num_classes=13):
    data = []
    meters = {m: ref.meter_s3dis(metric=m, num_classes=num_classes) for m in ('overall', 'class', 'iou')}
    for b, n in batches:
        x = tied_logits(gen, b, num_classes, n)
        t = torch.randint(0, num_classes - 1, (b, n), generator=gen)                 # class C-1 never a target (seen 0)
        for m in meters.values():
            m.update(x, t)
        data.append(dict(outputs=x, targets=t))
    return dict(batches=data, num_classes=num_classes, results={k: m.compute() for k, m in meters.items()},
                counts=[*meters['iou'].total_seen, *meters['iou'].total_positive, *meters['iou'].total_correct,
                        meters['overall'].total_seen_num, meters['overall'].total_correct_num])


def meter_shapenet_case(ref, gen, batches):
    meter = ref.meter_shapenet()
    table = meter.part_class_to_shape_part_classes
    data = []
    for b, n in batches:
        x = tied_logits(gen, b, meter.num_classes, n)
        t = torch.empty((b, n), dtype=torch.int64)
        for i in range(b):
            s, e = table[int(torch.randint(0, len(table), (1,), generator=gen))]
            hi = e - 1 if i % 2 == 0 and e - s > 2 else e                            # a part class absent from the target
            t[i] = torch.randint(s, hi, (n,), generator=gen)
            if i % 3 == 0:                                                           # ... and from the prediction: union 0 -> IoU 1
                x[i, hi:e] = -10.0
        meter.update(x, t)
        data.append(dict(outputs=x, targets=t))
    return dict(batches=data, result=meter.compute())


def main():
    ref = load_reference()
    rng = np.random.RandomState(SEED)
    gen = torch.Generator().manual_seed(SEED)
    out = {
        's3dis': [s3dis_case(ref, rng, 7, 40, 16, 120, 3, 5),
                  s3dis_case(ref, rng, 5, 64, 32, 300, 2, 6),
                  s3dis_case(ref, rng, 4, 24, 8, 10, 4, 3, all_to_one=True)],
        'shapenet': [shapenet_case(ref, rng, 50, 16, 8, 12), shapenet_case(ref, rng, 33, 32, 30, 36, calls_n=3)],
        'meter_s3dis': meter_s3dis_case(ref, gen, [(2, 100), (3, 57), (1, 1)]),
        'meter_shapenet': meter_shapenet_case(ref, gen, [(5, 64), (4, 33)]),
    }
    # the index builder of s3dis_file_votes: the reference loop's shuffles from a seeded RandomState
    r2 = np.random.RandomState(7)
    snp = np.array([30, 17, 64, 5], dtype=np.int64)
    want = []
    for w in range(len(snp)):
        idx = np.tile(np.arange(snp[w]), math.ceil(64 / snp[w]))[:64]
        r2.shuffle(idx)
        want.append(idx)
    out['shuffle'] = dict(seed=7, scene_num_points=torch.from_numpy(snp), V=64, indices=torch.from_numpy(np.stack(want)),
                          next_draw=float(r2.random_sample()))
    path = os.path.join(HERE, 'eval_votes.pt')
    torch.save(out, path)
    print(f'wrote {path} ({os.path.getsize(path)} bytes)')


if __name__ == '__main__':
    main()
