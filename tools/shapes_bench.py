"""The two launches of the ShapeNet front end (pvcnn_amd.shapes, csrc/shapes.hip) at the sizes a user runs, against the numpy truth on
the same machine's host.

    python tools/shapes_bench.py [--k 16] [--runs 20] [--rounds 3] [--truth-clouds 8] [--truth-queries 256] [--out FILE]

Two seeded inputs:
  * split : a synthetic ShapeNet-sized split, 2,874 clouds (the size of the test split), n uniform in [512, 2947], points on a unit
            sphere's surface squashed to an ellipsoid, packed as data._Store packs them;
  * cloud : one cloud of 65,536 points of the same kind.
Per input and launch (k_nearest, shape_normals with curvature and the outward mode, cloud_centroids): every shape warmed up first, then
`--rounds` rounds of `--runs` launches between two device events, the stream synchronised before and after; all rounds are printed.
Before anything is timed the device results are checked against tests/shapes_truth.py on the truth's subset: the neighbour tables must
be equal, the normals must meet the inequalities.  Next to the device times: the host clock of the numpy truth (k_nearest_definition +
covariances: fp32 distances, a stable sort, fp64 covariance, eigh) on a stated subset -- the first `--truth-clouds` clouds of the split,
`--truth-queries` query rows of the large cloud -- and that figure scaled to the whole input by the distances it would take.
One JSON line per measurement."""
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

import shapes_truth as T                                                # noqa: E402
from pvcnn_amd.modules.functional.backend import _backend as be         # noqa: E402

SEED = 1588147245


def surface(rng, n):
    u = rng.randn(n, 3)
    return ((u / np.linalg.norm(u, axis=1, keepdims=True)) * [1.0, 0.6, 0.3]).astype(np.float32)


def between_events(fn, runs):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(runs):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / runs


def report(name, **fields):
    print(json.dumps({'measurement': name, **fields}), flush=True)


def measure(tag, rows_np, offsets_np, a, truth_rows):
    """truth_rows: (first row, one past the last row) of the packed rows the truth is computed on (whole clouds), or query rows."""
    dev = torch.device('cuda:0')
    rows, offsets = torch.from_numpy(rows_np).to(dev), torch.from_numpy(offsets_np).to(dev)
    r, w = rows_np.shape[0], offsets_np.size - 1
    sizes = np.diff(offsets_np)
    shape = {'input': tag, 'rows': int(r), 'clouds': int(w), 'k': a.k, 'distances': int((sizes.astype(np.float64) ** 2).sum()),
             'device': torch.cuda.get_device_name(0)}
    knn = torch.empty((r, a.k), dtype=torch.int32, device=dev)
    ref = torch.empty((w, 3), device=dev)
    normals, curvature = torch.empty((r, 3), device=dev), torch.empty((r,), device=dev)
    launches = {'k_nearest': lambda: be.k_nearest(rows, offsets, a.k, out=knn),
                'cloud_centroids': lambda: be.cloud_centroids(rows, offsets, out=ref),
                'shape_normals': lambda: be.shape_normals(rows, offsets, knn, ref, 1, out=normals, out_curvature=curvature)}
    for fn in launches.values():                                       # results first; this is also the warm-up of every shape
        fn()
        fn()
    torch.cuda.synchronize()

    # the truth on its subset, timed on the host clock, and the device results against it
    t0 = time.perf_counter()
    if w > 1:
        lo, hi = truth_rows
        sub_off = offsets_np[(offsets_np >= lo) & (offsets_np <= hi)] - lo
        want = T.k_nearest_definition(rows_np[lo:hi], sub_off, a.k)
        t1 = time.perf_counter()
        T.covariances(rows_np[lo:hi], sub_off, want)
        t2 = time.perf_counter()
        ok = np.array_equal(knn[lo:hi].cpu().numpy(), want)
        T.check_normals(rows_np[lo:hi], sub_off, want, normals[lo:hi].cpu().numpy(), curvature[lo:hi].cpu().numpy(), mode=1,
                        ref=ref.cpu().numpy()[:sub_off.size - 1])
        done = float((np.diff(sub_off).astype(np.float64) ** 2).sum())
        subset = f'the first {sub_off.size - 1} clouds ({hi - lo} rows)'
    else:
        queries = truth_rows
        want = T.k_nearest_rows(rows_np, queries, a.k)
        t1 = time.perf_counter()
        full = knn.cpu().numpy()
        ok = np.array_equal(full[queries], want)
        t2 = t1
        T.check_normals(rows_np, offsets_np, full, normals.cpu().numpy(), curvature.cpu().numpy(), mode=1, ref=ref.cpu().numpy())
        done = float(len(queries)) * r
        subset = f'{len(queries)} query rows of the cloud (selection instead of a full sort; neighbour table only)'
    report('equal_to_the_truth', ok=bool(ok), subset=subset, **shape)
    if not ok:
        raise SystemExit('the device path differs from the truth: nothing is timed')
    report('numpy_truth_host_clock', subset=subset, k_nearest_s=round(t1 - t0, 4), covariance_eigh_s=round(t2 - t1, 4),
           k_nearest_scaled_to_the_input_s=round((t1 - t0) * shape['distances'] / done, 2), host_cpus_visible=os.cpu_count(),
           numpy=np.__version__, **shape)

    for name, fn in launches.items():
        times = [between_events(fn, a.runs) for _ in range(a.rounds)]
        report(name + '_device_events', ms_per_launch=[round(t, 4) for t in times], ms_median=round(sorted(times)[len(times) // 2], 4),
               runs_per_round=a.runs, **shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--k', type=int, default=16)
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--clouds', type=int, default=2874)
    ap.add_argument('--large', type=int, default=65536)
    ap.add_argument('--truth-clouds', type=int, default=8)
    ap.add_argument('--truth-queries', type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('shapes_bench needs a GPU: nothing is measured on the host alone')
    if a.runs < 20:
        raise SystemExit('at least 20 runs per round')
    rng = np.random.RandomState(SEED % (2 ** 31))
    sizes = rng.randint(512, 2948, size=a.clouds)
    offsets = T.offsets_of(sizes)
    rows = np.concatenate([surface(rng, n) for n in sizes])
    measure('split', rows, offsets, a, (0, int(offsets[min(a.truth_clouds, a.clouds)])))
    large = surface(rng, a.large)
    measure('cloud', large, T.offsets_of([a.large]), a, np.sort(rng.choice(a.large, size=a.truth_queries, replace=False)))


if __name__ == '__main__':
    main()
