#!/usr/bin/env python3
"""Time one pvcnn_amd.kitti.get_official_eval_result call on a synthetic validation-sized input (profiles/kitti_ap.md).

The images come from the generator of tests/golden/gen_kitti_ap_golden.py (its distribution, its seed; the redraw conditions of the
fixture are not applied: they need the reference).  Warm, HIP events around the call, the median of the repeats; the call includes the
host-side packing of the annotations and the final copies.
Run:  python tools/kitti_ap_time.py [images=3769] [repeats=7]
"""
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    images = int(sys.argv[1]) if len(sys.argv) > 1 else 3769
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    spec = importlib.util.spec_from_file_location('gen_kitti_ap_golden', os.path.join(ROOT, 'tests', 'golden', 'gen_kitti_ap_golden.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    from pvcnn_amd import kitti
    rng = np.random.RandomState(gen.SEED)
    pairs = [gen.draw_image(rng) for _ in range(images)]
    gt_annos, dt_annos = [p[0] for p in pairs], [p[1] for p in pairs]
    kitti.get_official_eval_result(gt_annos, dt_annos, [0, 1, 2])                      # warm-up: library load, allocator
    device_ms, wall_ms = [], []
    for _ in range(repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start.record()
        _, results, _ = kitti.get_official_eval_result(gt_annos, dt_annos, [0, 1, 2])
        end.record()
        torch.cuda.synchronize()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        device_ms.append(start.elapsed_time(end))
    print(json.dumps({'images': images, 'ground_truths': int(sum(len(a['name']) for a in gt_annos)),
                      'detections': int(sum(len(a['name']) for a in dt_annos)), 'repeats': repeats,
                      'event_ms_median': float(np.median(device_ms)), 'event_ms_all': [round(v, 3) for v in device_ms],
                      'wall_ms_median': float(np.median(wall_ms)), 'device': torch.cuda.get_device_name(0),
                      'car_bbox_ap': [round(float(v), 2) for v in results['Car']['bbox']]}))


if __name__ == '__main__':
    main()
